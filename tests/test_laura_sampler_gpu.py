"""The LauraTTS device sampler on the GPU, per draw, through LauraEngine.sample (fc_laura_sample: the engine's own launch_sample on the
caller's logits and state).  The reference, the recipes, the rounding bands and the proof that both have teeth are
tests/test_laura_sampler_host.py's; every case there is a row here, 64 rows to a launch.

Models: tinylaura (nq = 2), tinylaurauni (nq = 1), and tinylaura320 for the next-step embedding alone (LM width 320: three k parts, 240
working threads in embed_next).

  * picks: every group's pick of every case lies in sample_ref's accepted set (one id for every planted case), in table form and, for
    the cases it can express (no rules, one mode per launch), in call form, where the Philox row word is the batch row;
  * bookkeeping: step, n_gen, done, pos, n_done and the token rows exactly as bookkeeping_ref says; nothing else in the token buffer moves;
  * form independence: a row alone, as row 5 of 16, as row 37 of 64, through row0 / nrows, and in call form at batch row b = table form
    with rng_row = b: the same bits in tokens, state, score, log-probability row, next_emb and xs; a row0 / nrows launch leaves the other
    rows' state, tokens and outputs untouched;
  * score: against float64 from the same logits and final picks, bar nq x 1e-5 x max(1, 1 / T) (test_laura_rules_gpu.py); the same bits
    in greedy, drawing and forced form for the same final picks;
  * log-softmax rows: against float64, bar = test_laura_attention_host.bar (12 x torch float32's own error, floor and cap); rows of
    inactive utterances untouched;
  * next embedding: next_emb bitwise the float32 sum of the chosen codebook rows in k order; xs against float64 Linear + LayerNorm
    (eps 1e-5) + ReLU + x sqrt(d) under the same bar, at LM width 128 and 320.

What the tests found (read in the code first, then seen on the MI355X, 2026-10-21, with the two fixes taken out of the build):
  * signed zeros: the radix select's integer key ordered -0.0 below +0.0, so a -0.0 at a lower index lost the top-k cut to a +0.0 at a
    higher one: "signed zeros k1 ids(3, 7) -+" picked 7 for the documented 3, "signed zeros k2 ids(700, 20, 300) +-+" 700 for 300.  The
    key now maps -0.0 to +0.0's.
  * an id without mass at the top of the draw: at u = 1 - 2^-24 the walk's own sums, rounded in another order than the scan's, can pass
    the last entry with mass, and the walk then ran over the ids behind it to the end of its chunk (or, over the lane's chunks, to its
    last chunk).  Where those ids fill a chunk of their own (ids 1020 .. 1024 of 1025 candidates, CH = 5) nothing happens; where they share
    the last chunk or lane with ids that have mass, 21 of the 64 "u top ..., mass ends inside the last chunk" / "u top top100, ... ids with
    mass" rows (as the recipes stood that day; their logits are seeded, not fixed by hand) drew an id of probability exactly 0 (id 1019; ids 0 .. 4 of a top-100 with 97 .. 99 ids of mass).  The walk now steps
    back to the last entry with positive mass.
Neither changes a bit of a draw whose candidates hold no -0.0 and whose walk ends on an entry with mass: the existing sampler, rules
and score tests pass unchanged.

Measured on an MI355X (max over the cases of each group: engine vs float64 / torch float32 vs float64, then the smallest bar any case
of the group had; the score has no torch counterpart, its bar is nq x 1e-5 x max(1, 1 / T)):
  score, table form      tinylaurauni 1.7e-6, 1.0e-5   tinylaura 5.3e-6, 2.0e-5      (616 rows per model in 10 launches)
  score, call form       nq 1 7.4e-7, 1.0e-5           nq 2 1.6e-6, 2.0e-5           (241 / 240 rows in 36 launches)
  score, forced forms    nq 1 6.5e-7, 1.0e-5           nq 2 1.2e-6, 2.0e-5           (the same bits in modes 0 .. 3)
  log-softmax rows       tinylaurauni 3.8e-6 / 3.9e-6, 8.7e-6   tinylaura 7.7e-6 / 7.7e-6, 9.5e-6   (4 inactive rows untouched per model)
  xs (fused input layer) tinylaurauni 8.9e-6 / 1.8e-5, 1.0e-4   tinylaura 8.5e-6 / 1.8e-5, 1.8e-4   tinylaura320 1.6e-5 / 3.1e-5, 3.8e-4
Every pick of every row lay in its accepted set (one id for each planted row); next_emb bitwise in every row.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_laura_attention_host import bar, model_cfg
from test_laura_sampler_host import (EOS, K, R_ROWS, all_cases, bookkeeping_ref, case, log_softmax_ref, neutral, random_cases, random_group,
                                     ref_of, sample_ref, score_ref)

from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
from funcodec_amd.synth import make_laura_state_dict

pytestmark = pytest.mark.gpu

MODEL_OF = {2: "tinylaura", 1: "tinylaurauni"}
FILL = -7.0
_engines = {}
WORST = {}


def engine(name):
    from funcodec_amd.laura import LauraGenMI355X
    if name not in _engines:
        cfg = model_cfg(name) if name == "tinylaura320" else laura_recipe_config(name)
        spec, sd = laura_spec_from_config(cfg), make_laura_state_dict(cfg, 3)
        m = LauraGenMI355X(spec, "cuda:0", max_positions=128)
        m.load_state_dict(sd)
        _engines[name] = (m, spec, {k: torch.as_tensor(v) for k, v in sd.items()})
    m, spec, sd = _engines[name]
    return m.engine, spec, sd


def note(group, err, e32, tol):
    w = WORST.setdefault(group, [0.0, 0.0, math.inf])
    w[0], w[1], w[2] = max(w[0], err), max(w[1], e32), min(w[2], tol)


def show(group):
    e, e32, tol = WORST[group]
    print(f"measured {group}: engine {e:.2e} / torch float32 {e32:.2e} / smallest bar {tol:.2e}")


def table_row(c):
    p = c["prm"]
    return dict(mode=p["mode"], k=p["k"], p=p["p"], max_steps=p["max_steps"], seed=p["seed"], forced_on=int(bool(p["forced_on"] and c["forced"] is not None)),
                rng_row=p["rng_row"], temperature=p["temperature"], min_length=p["min_length"], top_p=p["top_p"],
                repeat_window=p["repeat_window"], repeat_count=p["repeat_count"])


def pack(cases, R, steps):
    """the tensors of one launch: logits [B, V], tokens [B, R, nq] (each row's history at tok_off, -1 elsewhere: an id no draw returns),
    forced [B, steps, nq] or None, the state lists"""
    B, nq = len(cases), cases[0]["nq"]
    logits = torch.from_numpy(np.stack([c["logits"].reshape(-1) for c in cases]))
    tokens = torch.full((B, R, nq), -1, dtype=torch.int64)
    forced = None
    if any(c["forced"] is not None for c in cases):
        forced = torch.zeros((B, steps, nq), dtype=torch.int64)
    for b, c in enumerate(cases):
        gen = c["state"]["gen"]
        tokens[b, c["tok_off"]: c["tok_off"] + gen] = torch.from_numpy(c["history"])
        if c["forced"] is not None and gen < steps:
            forced[b, gen] = torch.tensor(c["forced"])
    state = dict(step=[c["state"]["step"] for c in cases], n_gen=[c["state"]["gen"] for c in cases], done=[c["state"]["done"] for c in cases],
                 pos=[c["state"]["pos"] for c in cases], tok_off=[c["tok_off"] for c in cases])
    return logits, tokens, forced, state


def launch(eng, cases, R=R_ROWS, logp=False, score=True, **kw):
    """table form: one launch of the cases as its rows"""
    logits, tokens, forced, state = pack(cases, R, R)
    out = eng.sample(logits, tokens, rows=[table_row(c) for c in cases], forced=forced, logp=logp, score=score, fill=FILL, **state, **kw)
    out["tokens_in"] = tokens
    return out


def check_rows(cases, out, refs=None, what="table"):
    """picks in the accepted sets, bookkeeping and token rows exact.  -> the observed final picks per row (None: the row wrote none)"""
    tokens, want_tokens = out["tokens"].cpu(), out["tokens_in"].clone()
    ended, picks_of, bad = 0, [], []                 # bad: every pick outside its set, so that one run names all of them
    for b, c in enumerate(cases):
        ref = refs[b] if refs else ref_of(c)
        st, prm, who = c["state"], c["prm"], (what, b, c["name"])
        active = not st["done"] and st["gen"] < prm["max_steps"]
        picks = None
        if active and out["n_gen"][b] == st["gen"] + 1:
            picks = [int(v) for v in tokens[b, c["tok_off"] + st["gen"]]]
            bad += [who + (k, t, sorted(ref["final"][k])) for k, t in enumerate(picks) if t not in ref["final"][k]]
        elif active and not any(EOS in s for s in ref["final"]):
            bad.append(who + ("the row ended without an acceptable <eos>", [sorted(s)[:4] for s in ref["final"]]))
        book = bookkeeping_ref(picks if picks is not None else [EOS], prm, st, c["tok_off"])
        got = dict(step=out["step"][b], gen=out["n_gen"][b], done=out["done"][b], pos=out["pos"][b])
        assert got == {k: book[k] for k in got}, who + (got, book)
        if book["write"] is not None:
            want_tokens[b, book["write"]] = torch.tensor(picks)
        ended += book["ended"]
        picks_of.append(picks)
    assert not bad, bad
    assert torch.equal(tokens, want_tokens), (what, "a token row moved that the bookkeeping does not write")
    assert out["n_done"] == ended, (what, out["n_done"], ended)
    return picks_of


def check_score(cases, out, picks_of, group, refs=None):
    sc = out["score"].cpu()
    for b, c in enumerate(cases):
        st, prm = c["state"], c["prm"]
        active = not st["done"] and st["gen"] < prm["max_steps"]
        row = sc[b].clone()
        if active:
            ref = refs[b] if refs else ref_of(c)
            final = picks_of[b] if picks_of[b] is not None else [next(iter(s)) for s in ref["final"]]
            if picks_of[b] is None and not all(len(s) == 1 for s in ref["final"]):
                row[st["gen"]] = FILL
            else:
                want = score_ref(ref, final)
                got = float(row[st["gen"]])
                tol = c["nq"] * 1e-5 * max(1.0, 1.0 / prm["temperature"])
                if math.isinf(want):
                    assert got == want, (c["name"], got, want)
                else:
                    note(group, abs(got - want), 0.0, tol)
                    assert abs(got - want) <= tol, (c["name"], got, want, tol)
                row[st["gen"]] = FILL
        assert bool((row == FILL).all()), (c["name"], "a score entry outside the row's step was written")


def check_embedding(name, cases, out, picks_of, group):
    """next_emb bitwise, xs against float64; rows that append no token keep the fill"""
    _, spec, sd = engine(name)
    cb = sd["quantizer_codebook.embed"].float()
    W, bias = sd["codec_lm.encoder.embed.0.weight"], sd["codec_lm.encoder.embed.0.bias"]
    g, beta = sd["codec_lm.encoder.embed.1.weight"], sd["codec_lm.encoder.embed.1.bias"]
    d = spec.codec_lm.d_model
    nemb, xs = out["next_emb"].cpu(), out["xs"].cpu()
    rows = [b for b in range(len(cases)) if picks_of[b] is not None]
    for b in range(len(cases)):
        if picks_of[b] is None:
            assert bool((nemb[b] == FILL).all()) and bool((xs[b] == FILL).all()), (cases[b]["name"], "written without a new token")
    want = torch.stack([sum_in_k_order(cb, picks_of[b]) for b in rows])
    assert torch.equal(nemb[rows], want), "next_emb is the float32 sum of the chosen codebook rows in k order"

    def layer(x, dt):
        y = F.layer_norm(F.linear(x.to(dt), W.to(dt), bias.to(dt)), (d,), g.to(dt), beta.to(dt), 1e-5)
        return (F.relu(y) if spec.codec_lm.embed_relu else y) * math.sqrt(d)
    ref = layer(want, torch.float64)
    e32 = float((layer(want, torch.float32).double() - ref).abs().max())
    err, tol = float((xs[rows].double() - ref).abs().max()), bar(ref, e32)
    note(group, err, e32, tol)
    assert err <= tol, (group, err, e32, tol)


def sum_in_k_order(cb, picks):
    s = cb[0, picks[0]].clone()
    for k in range(1, len(picks)):
        s = s + cb[k, picks[k]]
    return s


def batches(cases, n=64):
    return [cases[i: i + n] for i in range(0, len(cases), n)]


# ---- picks, bookkeeping, score, next embedding: every case, table form ------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2])
def test_every_case_in_table_form(nq):
    name = MODEL_OF[nq]
    eng, _, _ = engine(name)
    cases = all_cases(nq)
    for part in batches(cases):
        out = launch(eng, part)
        picks_of = check_rows(part, out)
        check_score(part, out, picks_of, f"score {name}")
        check_embedding(name, part, out, picks_of, f"xs {name}")
    print(f"{len(cases)} rows in {len(batches(cases))} launches")
    show(f"score {name}")
    show(f"xs {name}")


def call_form_groups(nq):
    """the cases the call form can express (no rules, nothing forced), by (mode, k, p); seed and max_steps become the launch's"""
    groups = {}
    for c in all_cases(nq):
        p = c["prm"]
        if (p["temperature"], p["min_length"], p["top_p"], p["repeat_window"]) == (1.0, 0, 0.0, 0) and c["forced"] is None:
            groups.setdefault((p["mode"], p["k"], p["p"]), []).append(c)
    return groups


@pytest.mark.parametrize("nq", [1, 2])
def test_every_expressible_case_in_call_form(nq):
    eng, _, _ = engine(MODEL_OF[nq])
    n = launches = 0
    for (mode, k, p), cases in sorted(call_form_groups(nq).items()):
        for part in batches(cases):
            seed, max_steps = 900 + launches, max(c["prm"]["max_steps"] for c in part)
            part = [dict({kk: v for kk, v in c.items() if kk != "_ref"}, prm=dict(c["prm"], seed=seed, max_steps=max_steps)) for c in part]
            refs = [sample_ref(c["logits"], c["prm"], c["state"], c["history"], None, batch_row=b) for b, c in enumerate(part)]
            R = max(c["tok_off"] for c in part) + max_steps
            logits, tokens, _, state = pack(part, R, max_steps)
            out = eng.sample(logits, tokens, mode=mode, k=k, p=p, seed=seed, max_steps=max_steps, score=True, fill=FILL, **state)
            out["tokens_in"] = tokens
            picks_of = check_rows(part, out, refs, "call")
            check_score(part, out, picks_of, f"score call form nq{nq}", refs)
            n += len(part)
            launches += 1
    print(f"{n} rows in {launches} call-form launches")
    show(f"score call form nq{nq}")
    assert n >= 100


# ---- form independence --------------------------------------------------------------------------------------------------------------------
def chosen_rows(nq):
    """a few rows of every kind: each mode, rules on, a redraw, forced, <eos>, done"""
    want = ("random softmax sd2.0 T1.0 #0", "random top25 sd2.0 T0.75 #1", "random nucleus0.8 sd5.0 T2.0 #0", "random top25p0.9 sd0.5 T1.0 #0",
            "random greedy sd2.0 T1.0 #0", "random repeat softmax sd2.0 W8", "random masked top25 sd2.0 #0", "forced on top25", "done row softmax",
            "<eos> ends the row greedy", "top100 last-but-one candidate", "step 0 softmax")
    by_name = {c["name"]: c for c in all_cases(nq)}
    return [by_name[n] for n in want]


def row_bits(out, b, c, steps_row):
    """everything a launch produced for row b"""
    lp = out["logp"][b, steps_row].cpu() if out["logp"] is not None else None
    return (out["tokens"][b].cpu(), out["step"][b], out["n_gen"][b], out["done"][b], out["pos"][b], out["score"][b].cpu(), lp,
            out["next_emb"][b].cpu(), out["xs"][b].cpu())


def same_bits(a, b):
    return all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("nq", [1, 2])
def test_a_row_does_not_depend_on_its_launch(nq):
    eng, _, _ = engine(MODEL_OF[nq])
    filler = [c for c in random_cases(nq) if c["state"]["gen"] < 8][:64]
    R = 16
    chosen = chosen_rows(nq)
    assert len(chosen) == 12 and all(c["tok_off"] + c["prm"]["max_steps"] <= R for c in chosen), "every chosen row fits the R token rows"
    for c in chosen:
        g = c["state"]["gen"]
        alone = launch(eng, [c], R=R, logp=True)
        base = row_bits(alone, 0, c, g)
        for B, at in ((16, 5), (64, 37)):
            rows = filler[:B]
            rows = rows[:at] + [c] + rows[at + 1:]
            out = launch(eng, rows, R=R, logp=True)
            assert same_bits(row_bits(out, at, c, g), base), (c["name"], B, at)
            # the same row through row0 / nrows: the other rows' state, tokens and outputs stay as they were
            one = launch(eng, rows, R=R, logp=True, row0=at, nrows=1)
            assert same_bits(row_bits(one, at, c, g), base), (c["name"], "row0", at)
            others = [b for b in range(B) if b != at]
            assert torch.equal(one["tokens"].cpu()[others], one["tokens_in"][others]), c["name"]
            for key in ("step", "n_gen", "done", "pos"):
                src = "gen" if key == "n_gen" else key
                assert [one[key][b] for b in others] == [rows[b]["state"][src] for b in others], (c["name"], key)
            for key in ("score", "logp", "next_emb", "xs"):
                assert bool((one[key].cpu()[others] == FILL).all()), (c["name"], key)
        # call form at batch row b = table form with rng_row = b
        p = c["prm"]
        if (p["temperature"], p["min_length"], p["top_p"], p["repeat_window"]) == (1.0, 0, 0.0, 0):
            at = 9
            twin = dict({k: v for k, v in c.items() if k != "_ref"}, prm=dict(p, rng_row=at))
            base9 = row_bits(launch(eng, [twin], R=R, logp=True), 0, twin, g)
            rows = [twin] * 16
            ms = p["max_steps"]
            logits, tokens, forced, state = pack(rows, R, ms)
            out = eng.sample(logits, tokens, mode=p["mode"], k=p["k"], p=p["p"], seed=p["seed"], max_steps=ms, forced=forced, logp=True, score=True,
                             fill=FILL, **state)
            got = row_bits(out, at, twin, g)
            ref = list(base9)
            ref[5] = ref[5][:ms]                                          # the call form's score row has max_steps entries
            assert same_bits(got, tuple(ref)), (c["name"], "call form")


# ---- the score: one function of the logits and the final picks ---------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2])
def test_score_is_the_same_bits_in_every_form(nq):
    eng, _, _ = engine(MODEL_OF[nq])
    rng = np.random.Generator(np.random.PCG64(41 + nq))
    drawn = [case(f"score row {i}", np.stack([random_group(rng, (0.5, 2.0, 5.0)[i % 3]) for _ in range(nq)]),
                  neutral(mode=1 + i % 3, k=25, p=0.8, temperature=(1.0, 0.75, 2.0)[i % 3]), gen=i % 3, seed=70 + i, rng_row=i) for i in range(48)]
    out = launch(eng, drawn, R=16)
    picks_of = check_rows(drawn, out)
    base = out["score"].cpu()
    for mode in (0, 1, 2, 3):
        forced = [dict({k: v for k, v in c.items() if k != "_ref"}, prm=dict(c["prm"], mode=mode, seed=c["prm"]["seed"] + 1), forced=picks_of[b])
                  for b, c in enumerate(drawn)]
        got = launch(eng, forced, R=16)
        assert check_rows(forced, got) == picks_of
        assert torch.equal(got["score"].cpu(), base), f"forced picks in mode {mode}"
    check_score(drawn, out, picks_of, f"score forms nq{nq}")
    show(f"score forms nq{nq}")


# ---- the log-softmax rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2])
def test_log_softmax_rows_against_float64(nq):
    name = MODEL_OF[nq]
    eng, spec, _ = engine(name)
    fits = [c for c in all_cases(nq) if c["tok_off"] + c["prm"]["max_steps"] <= 8]
    inactive = [c for c in fits if c["state"]["done"] or c["state"]["gen"] >= c["prm"]["max_steps"]]
    assert {c["name"] for c in inactive} >= {"done row greedy", "done row softmax", "gen at max_steps greedy", "gen at max_steps softmax"}
    cases = inactive + [c for c in fits if not any(c is i for i in inactive)][::3][:124]
    group = f"log-softmax {name}"
    untouched = 0
    for part in batches(cases):
        out = launch(eng, part, R=8, logp=True)
        lp = out["logp"].cpu()
        for b, c in enumerate(part):
            st = c["state"]
            rows = lp[b].clone()
            if not st["done"] and st["gen"] < c["prm"]["max_steps"]:
                ref = torch.from_numpy(log_softmax_ref(c["logits"]))
                l32 = torch.from_numpy(c["logits"].reshape(-1))
                e32 = float((torch.log_softmax(l32, 0).double() - ref).abs().max())
                err, tol = float((rows[st["gen"]].double() - ref).abs().max()), bar(ref, e32)
                note(group, err, e32, tol)
                assert err <= tol, (c["name"], err, e32, tol)
                rows[st["gen"]] = FILL
            else:
                untouched += 1
            assert bool((rows == FILL).all()), (c["name"], "a log-probability row outside the row's step was written")
    assert untouched == len(inactive) >= 4, "rows of ended utterances and of utterances at max_steps were among the rows checked"
    show(group)


# ---- the next-step embedding at LM width 320 -------------------------------------------------------------------------------------------------
def test_next_embedding_at_width_320():
    eng, spec, _ = engine("tinylaura320")
    assert spec.codec_lm.d_model == 320 and spec.predict_nq == 2
    cases = [c for c in random_cases(2) if c["state"]["gen"] < 8][:64]
    out = launch(eng, cases, R=16)
    picks_of = check_rows(cases, out)
    check_embedding("tinylaura320", cases, out, picks_of, "xs tinylaura320")
    show("xs tinylaura320")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_bad_shapes_are_refused():
    from funcodec_amd.engine import EngineError
    eng, spec, _ = engine("tinylaura")
    c = random_cases(2)[0]
    logits, tokens, _, state = pack([c], 8, 8)
    row = table_row(c)
    with pytest.raises(EngineError, match="logits"):
        eng.sample(logits[:, :-1], tokens, rows=[row], **state)
    with pytest.raises(EngineError, match="tokens"):
        eng.sample(logits, tokens[:, :, :1], rows=[row], **state)
    with pytest.raises(EngineError, match="max_steps"):
        eng.sample(logits, tokens, rows=[dict(row, max_steps=9)], **state)
    with pytest.raises(EngineError, match="token rows"):
        eng.sample(logits, tokens, rows=[dict(row, max_steps=8)], **dict(state, tok_off=[1]))
    with pytest.raises(EngineError, match="row0"):
        eng.sample(logits, tokens, rows=[row], row0=1, **state)
    with pytest.raises(EngineError, match="forced"):
        eng.sample(logits, tokens, rows=[row], forced=torch.full((1, 8, 2), K + 1), **state)
    with pytest.raises(EngineError, match="finite"):
        eng.sample(torch.full_like(logits, math.inf), tokens, rows=[row], **state)
    with pytest.raises(EngineError, match="modes"):
        eng.sample(logits, tokens, rows=[dict(row, mode=4)], **state)
