"""The LauraTTS engine's two attention forms and the decoding-step block around the step form, per op against float64, through the two
test entries that run the engine's own launch code: LauraEngine.attention (fc_laura_attention: launch_attn_full as run_stack_full fills
it) and LauraEngine.step_block (fc_laura_step_block: the loop body of the kernel chain's run_step).  The references, input recipes and
bars are tests/test_laura_attention_host.py's, which proves on the CPU that they follow the reference model and that the inputs expose
a shifted relative position, a dropped pos_bias_v and a dropped last key at 100 x the bar.

Models: tinylaura as it is (LM at head dimension 64, codec_encoder at 32); tinylaura32 (its LM with 4 heads: head dimension 32, which
no other test of the suite gives the LM -- attn_step_kernel<32>, att_unit<32> of the persistent step, the GEMV's key-range combination at
DK = 32); tinylaura320 (LM width 320, 10 heads: a width the configuration accepts and whose linear_out GEMV used to refuse 13 rows and
more, the range weights not fitting the reduction scratch they were kept in).

  * full-sequence attention, four stacks (head dimension 64 / 32, plain and causal), T in FULL_T (128 = max_positions: the position-table
    clamp; T % 16 and T % 4 != 0; five and more key tiles), B = 3 with lengths (T, 1, T // 2 + 1), causal with a bidirectional prefix of
    0, 1, 5, 16, 17, len; rows < len against the reference, every element finite; planted keys 0, len - 1, 15, 16 that win by > 50;
  * masked keys add exactly nothing: values at positions >= len scaled by 1e3 (finite: 0 x NaN is NaN in the P.V MFMA, and the engine
    zeroes its padding upstream) leave rows < len bitwise equal;
  * step attention alone: q, the caches after the scatter and the raw partials from step_block, combined in float64 on the host,
    against the float64 reference of the same q and caches; head dimension 32 / 64, key ranges 1, 2, 3, 8, rows 1, 3, 16, 17, 33, 64,
    positions from STEP_POS (empty ranges report (-inf, 0) and a zero context; ranges that end inside a quad; a second 128-key pass);
    planted keys at the first / last key of a range and at key 127 / 128 of a long one;
  * the whole step block: new x and the scattered K / V column; stale cache contents (NaN behind pos) change no bit; a row's result
    does not depend on the row count, its column block or the `wide` instantiations;
  * the LM at head dimension 32 end to end: persistent step = kernel chain (the shape of test_laura.py's test), forced-token
    log-probabilities against LauraOracle within LOGP_TOL in both forms, no fallback;
  * tinylaura320: decode_codec on the kernel chain at 16 rows and a 64-slot session against LauraOracle within LOGP_TOL.

Measured on an MI355X (max over the cases of each group: engine vs float64 / torch float32 vs float64; then the smallest bar any case of
the group had, each bar being its own case's 12 x torch float32 within floor and cap):
  full form              text_encoder 1.7e-6 / 2.7e-6, 2.9e-6   codec_encoder 1.8e-6 / 1.9e-6, 2.7e-6   codec_lm 1.8e-6 / 1.6e-6, 3.0e-6
                         tinylaura32 codec_lm 1.7e-6 / 2.1e-6, 3.0e-6
  full form, planted     text_encoder 1.7e-6 / 2.2e-6, 9.3e-6   codec_encoder 3.1e-6 / 3.0e-6, 7.8e-6   codec_lm 2.6e-6 / 2.8e-6, 7.5e-6
                         tinylaura32 codec_lm 2.6e-6 / 1.9e-6, 8.0e-6
  step attention         tinylaura 1.1e-6 / 2.4e-6, 1.3e-6   tinylaura32 8.2e-7 / 1.8e-6, 1.4e-6   tinylaura320 1.6e-6 / 1.4e-6, 5.7e-6
  step attention, planted  tinylaura 8.9e-7 / 1.7e-6, 2.2e-6   tinylaura32 7.1e-7 / 1.6e-6, 2.2e-6
  step block, new x      tinylaura 5.1e-7 / 1.3e-6, 2.7e-6   tinylaura32 5.6e-7 / 7.2e-7, 2.8e-6   tinylaura320 5.1e-7 / 7.1e-7, 4.2e-6
  step block, q / k / v  tinylaura 5.3e-7 / 1.2e-6, 2.1e-6   tinylaura32 5.0e-7 / 1.3e-6, 1.9e-6   tinylaura320 6.7e-7 / 1.2e-6, 4.1e-6
  tinylaura32 end to end   max |logp persistent - chain| 1.9e-6 (B = 5 and 16); max |logp - oracle| 2.9e-6, chain and persistent
  tinylaura320             max |logp - oracle| 1.9e-6 at 16 rows on the chain and in the 64-slot session
Every engine figure is at torch float32's own level; nothing was found in the <32> instantiations or at the edges above.
"""
import math

import numpy as np
import pytest
import torch

from test_laura import LOGP_TOL
from test_laura_attention_host import (BIDIR, FULL_MAXPOS, FULL_STACKS, FULL_T, PLANT_KEYS, PLANT_T, STEP_MAXPOS, STEP_MODELS, attention_ref,
                                       bar, bidir_of, block_cases, block_params, combine_partials, engine_key_ranges, full_inputs, key_range,
                                       max_err, model, oracle_context32, rows_below, step_attention_ref, step_block_ref, step_cases,
                                       step_inputs, step_rounds)

from funcodec_amd.synth import synthetic_text

pytestmark = pytest.mark.gpu

_models = {}
WORST = {}            # group -> [engine error, torch float32 error, smallest bar]: printed by every test for the docstring's table


def gen_model(name, max_positions):
    from funcodec_amd.laura import LauraGenMI355X
    key = (name, max_positions)
    if key not in _models:
        _, spec, sd = model(name)
        m = LauraGenMI355X(spec, "cuda:0", max_positions=max_positions)
        m.load_state_dict(sd)
        _models[key] = m
    return _models[key]


def note(group, err, e32, tol):
    w = WORST.setdefault(group, [0.0, 0.0, math.inf])
    w[0], w[1], w[2] = max(w[0], err), max(w[1], e32), min(w[2], tol)


def show(group):
    e, e32, tol = WORST[group]
    print(f"measured {group}: engine {e:.2e} / torch float32 {e32:.2e} / smallest bar {tol:.2e}")


# ---- full-sequence attention ---------------------------------------------------------------------------------------------------------
def check_full(eng, mname, stack, causal, T, plant, bid_v, group):
    prm = block_params(mname, stack, 0)
    qkv, lens, _ = full_inputs(mname, stack, T, plant)
    bid = bidir_of(bid_v, lens) if causal else None
    got = eng.attention(stack, 0, qkv, lens, causal=causal, bidir=bid).cpu()
    assert got.shape == (3, T, prm.d) and bool(torch.isfinite(got).all()), (T, plant, bid_v)
    ref = attention_ref(qkv, lens, prm, causal, bid)
    rows = rows_below(lens, T)
    e32 = max_err(oracle_context32(qkv, lens, prm, causal, bid), ref, rows)
    err, tol = max_err(got, ref, rows), bar(ref, e32)
    note(group, err, e32, tol)
    assert err <= tol, (mname, stack, T, plant, bid_v, err, e32, tol)
    return qkv, lens, bid, got


@pytest.mark.parametrize("mname,stack,causal", FULL_STACKS)
def test_full_attention_against_float64(mname, stack, causal):
    eng = gen_model(mname, FULL_MAXPOS).engine
    group = f"full {mname} {stack}"
    for T in FULL_T:
        for bid_v in (BIDIR if causal else (None,)):
            check_full(eng, mname, stack, causal, T, None, bid_v, group)
    show(group)


@pytest.mark.parametrize("mname,stack,causal", FULL_STACKS)
def test_full_attention_with_a_dominant_key(mname, stack, causal):
    eng = gen_model(mname, FULL_MAXPOS).engine
    group = f"full planted {mname} {stack}"
    for T in PLANT_T:
        for plant in PLANT_KEYS:
            for bid_v in (BIDIR if causal else (None,)):
                check_full(eng, mname, stack, causal, T, plant, bid_v, group)
    show(group)


@pytest.mark.parametrize("mname,stack,causal", FULL_STACKS)
def test_masked_keys_add_exactly_nothing(mname, stack, causal):
    eng = gen_model(mname, FULL_MAXPOS).engine
    for T in (3, 17, 33, 128):
        for bid_v in ((0, 5, "len") if causal else (None,)):
            qkv, lens, _ = full_inputs(mname, stack, T)
            bid = bidir_of(bid_v, lens) if causal else None
            base = eng.attention(stack, 0, qkv, lens, causal=causal, bidir=bid).cpu()
            loud = qkv.clone()
            for b, L in enumerate(lens):
                loud[b, L:] *= 1e3
            assert not torch.equal(loud, qkv)
            got = eng.attention(stack, 0, loud, lens, causal=causal, bidir=bid).cpu()
            assert bool(torch.isfinite(got).all())
            rows = rows_below(lens, T)
            assert torch.equal(got[rows], base[rows]), (T, bid_v)


# ---- the decoding step -----------------------------------------------------------------------------------------------------------------
def run_block(eng, mname, B, NS, rnd=0, plant=None):
    x, kc, vc, pos, planted = step_inputs(mname, B, NS or engine_key_ranges(mname, B), rnd, plant)
    out = [t.cpu() for t in eng.step_block(0, x, kc, vc, pos, key_ranges=NS)]
    return (x, kc, vc, pos), out


@pytest.mark.parametrize("mname,rows", sorted({(m, B) for m, B, _, _ in step_cases()}))
def test_step_attention_alone_against_float64(mname, rows):
    eng = gen_model(mname, STEP_MAXPOS).engine
    prm = block_params(mname, "codec_lm", 0)
    H, dk = prm.H, prm.dk
    n_empty = 0
    for m, B, NS, plant in step_cases():
        if (m, B) != (mname, rows):
            continue
        group = f"step attention {mname}" + (" planted" if plant else "")
        for rnd in range(step_rounds(B)):
            (x, kc, vc, pos), (x2, q, part, kc2, vc2) = run_block(eng, mname, B, NS, rnd, plant)
            assert part.shape == (B, H, NS, dk + 2)
            for b in range(B):
                for r in range(NS):
                    k0, k1 = key_range(pos[b] + 1, NS, r)
                    if k1 > k0:
                        assert bool(torch.isfinite(part[b, :, r]).all()), (B, NS, b, r)
                        continue
                    n_empty += 1
                    assert bool((part[b, :, r, dk] == -math.inf).all()) and bool((part[b, :, r, dk + 1] == 0).all()), (B, NS, b, r)
                    assert bool((part[b, :, r, :dk] == 0).all()), (B, NS, b, r)
            got = combine_partials(part)
            ref = step_attention_ref(q, kc2, vc2, pos, prm)
            e32 = max_err(step_attention_ref(q, kc2, vc2, pos, prm, torch.float32), ref)
            err, tol = max_err(got, ref), bar(ref, e32)
            note(group, err, e32, tol)
            assert err <= tol, (mname, B, NS, plant, rnd, err, e32, tol)
    assert n_empty > 0
    for group in sorted(g for g in WORST if g.startswith(f"step attention {mname}")):
        show(group)


@pytest.mark.parametrize("mname", STEP_MODELS + ("tinylaura320",))
def test_step_block_against_float64(mname):
    eng = gen_model(mname, STEP_MAXPOS).engine
    prm = block_params(mname, "codec_lm", 0)
    for m, B, NS in block_cases():
        if m != mname:
            continue
        for rnd in range(step_rounds(B)):
            (x, kc, vc, pos), (x2, q, part, kc2, vc2) = run_block(eng, mname, B, NS, rnd)
            ref = step_block_ref(x, kc, vc, pos, prm)
            r32 = step_block_ref(x, kc, vc, pos, prm, torch.float32)
            rows = torch.arange(B)
            col = torch.tensor(pos)
            pairs = {"x": (x2, ref[0], r32[0]), "q": (q, ref[1], r32[1]), "k column": (kc2[rows, :, col], ref[2], r32[2]),
                     "v column": (vc2[rows, col], ref[3], r32[3])}
            for what, (got, r64, f32) in pairs.items():
                e32 = max_err(f32, r64)
                err, tol = max_err(got, r64), bar(r64, e32)
                note(f"step block {mname} {what}", err, e32, tol)
                assert err <= tol, (mname, B, NS, rnd, what, err, e32, tol)
            # the scatter wrote column pos and nothing else
            keep = torch.ones(B, kc.shape[2], dtype=torch.bool)
            keep[rows, col] = False
            assert torch.equal(kc2.transpose(1, 2)[keep], kc.transpose(1, 2)[keep]) and torch.equal(vc2[keep], vc[keep]), (B, NS)
    for what in ("x", "q", "k column", "v column"):
        show(f"step block {mname} {what}")


@pytest.mark.parametrize("mname", STEP_MODELS)
def test_stale_cache_contents_behind_pos_change_no_bit(mname):
    eng = gen_model(mname, STEP_MAXPOS).engine
    for B, NS in ((3, 8), (16, 2), (17, 3), (33, 1)):
        x, kc, vc, pos, _ = step_inputs(mname, B, NS)
        clean = eng.step_block(0, x, kc, vc, pos, key_ranges=NS)
        kn, vn = kc.clone(), vc.clone()
        for b in range(B):
            kn[b, :, pos[b] + 1:] = math.nan
            vn[b, pos[b] + 1:] = math.nan
        assert bool(torch.isnan(kn).any())
        stale = eng.step_block(0, x, kn, vn, pos, key_ranges=NS)
        for a, c, what in zip(clean[:3], stale[:3], ("x", "q", "partials")):
            assert bool(torch.isfinite(c).all() if what != "partials" else not torch.isnan(c).any()), (B, NS, what)
            assert torch.equal(a, c), (B, NS, what)


@pytest.mark.parametrize("mname", STEP_MODELS + ("tinylaura320",))
def test_a_row_of_the_step_block_depends_on_nothing_but_itself(mname):
    """alone, as row 5 of 16, as row 37 of 64 (column block 2), and through the `wide` instantiations at 1 and at 16 rows: one set of bits"""
    eng = gen_model(mname, STEP_MAXPOS).engine
    NS = 2
    d = block_params(mname, "codec_lm", 0).d
    for p in (0, 5, 129, 300):
        rng = np.random.Generator(np.random.PCG64([17, p]))
        mine = (torch.from_numpy(rng.standard_normal((1, d))).float(), torch.from_numpy(2.4 * rng.standard_normal((1, d, STEP_MAXPOS))).float(),
                torch.from_numpy(rng.standard_normal((1, STEP_MAXPOS, d))).float())
        alone = eng.step_block(0, *mine, [p], key_ranges=NS)
        runs = {"wide alone": eng.step_block(0, *mine, [p], key_ranges=NS, wide=True)}
        for B, row, wide in ((16, 5, False), (16, 5, True), (64, 37, False)):
            xs, ks, vs, pos, _ = step_inputs(mname, B, NS, 0, None)
            xs[row], ks[row], vs[row], pos[row] = mine[0][0], mine[1][0], mine[2][0], p
            out = eng.step_block(0, xs, ks, vs, pos, key_ranges=NS, wide=wide)
            runs[f"row {row} of {B}" + (" wide" if wide else "")] = tuple(t[row: row + 1] for t in out)
        for name, out in runs.items():
            for a, c, what in zip(alone, out, ("x", "q", "partials", "k cache", "v cache")):
                assert torch.equal(a, c), (p, name, what)


# ---- the LM at head dimension 32, end to end ---------------------------------------------------------------------------------------------
def forced_logp_against_oracle(mname, m, B, steps, seed):
    """decode_codec with forced tokens: the per-step log-probabilities, and the oracle's one-pass scores of the same sequences"""
    from laura_oracle import LauraOracle
    cfg, spec, sd = model(mname)
    orc = LauraOracle(cfg, sd)
    lens = [6 + (5 * i) % 11 for i in range(B)]
    text = torch.from_numpy(synthetic_text(cfg, B, lens, 17 + seed))
    rng = np.random.Generator(np.random.PCG64(40 + seed))
    forced = rng.integers(0, spec.codebook_size, size=(B, steps, spec.predict_nq)).astype(np.int64)
    with torch.no_grad():
        outs = orc.encode(text, lens)
        refs = []
        for b in range(B):
            seq = orc.llm_input(outs[b, : lens[b]], torch.from_numpy(forced[b]))
            refs.append(orc.lm_score_all(seq, 1 + lens[b])[lens[b] + 1: lens[b] + 1 + steps])
    return outs, lens, torch.from_numpy(forced), refs


@pytest.mark.parametrize("B,steps", [(5, 30), (16, 30)])
def test_persistent_step_equals_the_kernel_chain_at_head_dimension_32(B, steps):
    """test_laura.py::test_persistent_step_equals_the_kernel_chain on tinylaura32, with the same assertions"""
    cfg, spec, _ = model("tinylaura32")
    m = gen_model("tinylaura32", STEP_MAXPOS)
    lens = [12 + (5 * i) % 23 for i in range(B)]
    text = synthetic_text(cfg, B, lens, 17)
    rng = np.random.Generator(np.random.PCG64(4))
    forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(B, steps, spec.predict_nq)).astype(np.int64))
    cont = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(B, 9, spec.predict_nq)).astype(np.int64))
    cl = [9 - (i % 4) for i in range(B)]
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(text), torch.tensor(lens))
        assert m.engine.set_persistent_step(True), "the persistent step must be available for this model on MI355X"
        tp, lp, sp = m.engine.decode_codec(outs, lens, steps, sampling=False, forced=forced, return_logp=True, continual=cont, continual_lengths=cl)
        tp2, lp2, sp2 = m.engine.decode_codec(outs, lens, steps, sampling=False, forced=forced, return_logp=True, continual=cont, continual_lengths=cl)
        gp = m.engine.decode_codec(outs, lens, steps, sampling=False)
        kp = m.engine.decode_codec(outs, lens, steps, sampling=25, seed=11)
        assert not m.engine.set_persistent_step(False)
        tc, lc, sc = m.engine.decode_codec(outs, lens, steps, sampling=False, forced=forced, return_logp=True, continual=cont, continual_lengths=cl)
        gc = m.engine.decode_codec(outs, lens, steps, sampling=False)
        m.engine.set_persistent_step(True)
    assert lp == lc == [c + steps for c in cl] and torch.equal(tp, tc)
    assert torch.equal(sp, sp2) and torch.equal(tp, tp2)                      # run-to-run bit-identical
    err = float((sp - sc).abs().max())
    print("tinylaura32 B", B, "max |logp persistent - chain|", err)
    assert err < 2e-5, err
    assert gp[1] == gc[1] and torch.equal(gp[0], gc[0])                       # greedy generations identical
    assert all(0 <= v <= steps for v in kp[1]) and int(kp[0].max()) < spec.codebook_size
    assert m.engine.persistent_step_fallbacks == 0


@pytest.mark.parametrize("B", [5, 16])
def test_head_dimension_32_step_log_probabilities_against_the_oracle(B):
    m = gen_model("tinylaura32", STEP_MAXPOS)
    steps = 30
    outs, lens, forced, refs = forced_logp_against_oracle("tinylaura32", m, B, steps, B)
    for persistent in (False, True):
        assert m.engine.set_persistent_step(persistent) == persistent
        _, out_lens, slp = m.engine.decode_codec(outs, lens, steps, sampling=False, forced=forced, return_logp=True)
        assert all(v == steps for v in out_lens)
        slp = slp.cpu()
        err = max(float((slp[b] - refs[b]).abs().max()) for b in range(B))
        print("tinylaura32 B", B, "persistent" if persistent else "chain", "max |logp - oracle|", err)
        assert err < LOGP_TOL, (B, persistent, err)
    assert m.engine.persistent_step_fallbacks == 0


# ---- a width whose range weights did not fit the reduction scratch -----------------------------------------------------------------------
def test_width_320_decodes_16_rows_on_the_chain_and_64_slots():
    m = gen_model("tinylaura320", STEP_MAXPOS)
    B, steps = 16, 8
    outs, lens, forced, refs = forced_logp_against_oracle("tinylaura320", m, B, steps, 0)
    assert not m.engine.set_persistent_step(False)
    try:
        _, out_lens, slp = m.engine.decode_codec(outs, lens, steps, sampling=False, forced=forced, return_logp=True)
        assert all(v == steps for v in out_lens)
        slp = slp.cpu()
        err = max(float((slp[b] - refs[b]).abs().max()) for b in range(B))
        print("tinylaura320 decode_codec, 16 rows on the chain: max |logp - oracle|", err)
        assert err < LOGP_TOL, err
        # the same rows in a 64-slot session (the chain over four column blocks), one step(8); the other slots hold them again
        s = m.engine.open_decode(64, max_positions=64, wide=True)
        for slot in range(64):
            b = slot % B
            s.start(slot, outs[b, : lens[b]], lens[b], steps, sampling=False, forced=forced[b])
        st = s.step(steps)
        assert all(st.get(slot) == "done" for slot in range(64)), st
        worst = 0.0
        for slot in range(64):
            tok, n, lp = s.take(slot, return_logp=True)
            assert n == steps
            worst = max(worst, float((lp.cpu()[:steps] - refs[slot % B]).abs().max()))
        s.free()
        print("tinylaura320 64-slot session: max |logp - oracle|", worst)
        assert worst < LOGP_TOL, worst
    finally:
        m.engine.set_persistent_step(True)
