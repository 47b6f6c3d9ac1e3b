"""Wide decoding sessions of the LauraTTS engine on the GPU: up to 64 slots (LauraEngine.open_decode(wide=True)), the decoding step's
GEMV over column blocks of 16 rows.  What is pinned:

* per op: rows [16 j, 16 j + r) of a 17 / 32 / 33 / 64-row step-form Linear are, bit for bit, the call on those rows alone, in both
  LDS staging forms, and the whole result stands against torch.nn.functional.linear as the 16-row call does (2e-5 of the largest
  output, the bar of test_laura_music.py::test_music_step_form_linears_against_torch);
* a wide session of <= 16 slots is the session without the flag, bit for bit;
* a slot's bits depend neither on its column block nor on what the other 32 slots do;
* S = 17 and S = 64 against the reference's golden (forced tokens, LOGP_TOL) and against decode_codec on each prompt alone: greedy
  tokens and lengths equal, log-probabilities within 2e-5 (the bar of test_chain_and_persistent_step_agree for two summation orders of
  one step: the key-range split NS of a wide session is not that of one row).  Measured on MI355X: max |logp - alone| = 1.9e-6 at
  S = 17 and at S = 64; max |logp - golden| = 1.9e-6 (forced tokens) at both; per op, max |y - torch| <= 1.5e-6 against bars of
  3.8e-5 .. 6.2e-5;
* start_many / start_from / fork / rewind / rules / scores on slots >= 16 equal the same calls on slots < 16 of a session of the same
  width; refusals name the slot and change nothing; generate_many(slots=20) gives the tokens of generate_many(slots=4).
"""
import numpy as np
import pytest
import torch

from helpers import golden

from test_laura import LOGP_TOL, MAN, case_inputs, laura_engine
from test_laura_slots_gpu import B3, EOS, prompts, run_to_end, same, texts_of

pytestmark = pytest.mark.gpu

ENC = "codec_lm.encoder.encoders."
KINDS = [ENC + "0.self_attn.linear_qkv", ENC + "1.self_attn.linear_out", ENC + "2.feed_forward.w_1", ENC + "0.feed_forward.w_2",
         "codec_lm.decoder"]


def weights(sd, n):
    if n.endswith("linear_qkv"):
        p = n[: -len(".linear_qkv")]
        return (torch.cat([torch.from_numpy(sd[f"{p}.linear_{k}.weight"]) for k in "qkv"]),
                torch.cat([torch.from_numpy(sd[f"{p}.linear_{k}.bias"]) for k in "qkv"]))
    return torch.from_numpy(sd[n + ".weight"]), torch.from_numpy(sd[n + ".bias"])


def check_blocks(eng, sd, name, rows, seed):
    """the two assertions of test 1 for one Linear at one row count, in both staging forms"""
    W, b = weights(sd, name)
    rng = np.random.Generator(np.random.PCG64(seed))
    x = torch.from_numpy(rng.standard_normal((1, rows, W.shape[1])).astype(np.float32))
    ref = torch.nn.functional.linear(x, W, b)
    bar = 2e-5 * max(1.0, float(ref.abs().max()))
    for stage in ("auto", "windowed"):
        got = eng.linear(name, x, step_form=True, gemv_stage=stage).cpu()
        assert got.shape == ref.shape
        for r0 in range(0, rows, 16):
            r1 = min(rows, r0 + 16)
            alone = eng.linear(name, x[:, r0: r1].contiguous(), step_form=True, gemv_stage=stage).cpu()
            assert torch.equal(got[:, r0: r1], alone), (name, rows, stage, "column block", r0 // 16)
        err = float((got - ref).abs().max())
        print(name, "rows", rows, stage, "max |y - torch|", err, "bar", bar)
        assert err <= bar, (name, rows, stage, err)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [17, 32, 33, 64])
def test_a_column_block_is_the_16_row_call_bit_for_bit(rows):
    sd = case_inputs(B3)[3]
    eng = laura_engine(B3).engine
    assert weights(sd, "codec_lm.decoder")[0].shape[0] == 2050           # ends in a partial tile
    for i, n in enumerate(KINDS):
        check_blocks(eng, sd, n, rows, 100 * rows + i)


def test_music_column_blocks_through_the_windows():
    """K = 4096 (w_2: the <16, 4, 4> windows) and its w_1 at 33 rows: three column blocks, the last of one row."""
    from funcodec_amd.laura_config import laura_recipe_config
    from funcodec_amd.synth import make_laura_state_dict
    from test_laura_music import music_engine
    sd = make_laura_state_dict(laura_recipe_config("lauramusic"), 10)
    eng = music_engine(10).engine
    for i, n in enumerate([ENC + "0.feed_forward.w_1", ENC + "0.feed_forward.w_2"]):
        assert weights(sd, n)[0].shape[1] == (1024, 4096)[i]
        check_blocks(eng, sd, n, 33, 7 + i)


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling,seed", [(False, 0), (True, 1234)])
def test_a_narrow_wide_session_is_the_narrow_session(sampling, seed):
    eng, P, spec = prompts(B3)

    def run(**kw):
        s = eng.open_decode(3, max_positions=64, **kw)
        for b, p in enumerate(P):
            s.start(b, p, p.shape[0], 12, sampling=sampling, seed=seed + b)
            s.step(1)
        r = run_to_end(s, [0, 1, 2])
        s.free()
        return r

    wide, narrow = run(wide=True), run()
    for b in range(3):
        assert same(wide[b], narrow[b]), b


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling,seed", [(False, 0), (True, 99)])
def test_a_slot_depends_neither_on_its_column_block_nor_on_its_neighbours(sampling, seed):
    eng, P, spec = prompts(B3)
    Q = texts_of(EOS)
    A, steps, mine = P[0], 12, (3, 19, 32)                # slot 32 is alone in column block 2
    pool = [P[1], P[2], Q[0], Q[1]]

    s = eng.open_decode(33, max_positions=64, wide=True)
    for slot in mine:
        s.start(slot, A, A.shape[0], steps, sampling=sampling, seed=seed)
    quiet = run_to_end(s, mine)
    s.free()
    ref = quiet[3]
    assert same(quiet[19], ref) and same(quiet[32], ref), "the same prompt in column blocks 0, 1 and 2"

    others = [i for i in range(33) if i not in mine]
    s = eng.open_decode(33, max_positions=64, wide=True)
    for i in others[::2]:                                 # half the crowd starts before A
        p = pool[i % 4]
        s.start(i, p, p.shape[0], 30, sampling=True, seed=5 + i)
    s.step(2)
    for slot in mine:
        s.start(slot, A, A.shape[0], steps, sampling=sampling, seed=seed)
    short = others[1::4]
    for i in short:                                       # max_length 3: these end while A runs
        p = pool[i % 4]
        s.start(i, p, p.shape[0], 3, sampling=7, seed=11 + i)
    s.step(3)
    for i in others[3::4]:                                # these start three steps after A
        p = pool[i % 4]
        s.start(i, p, p.shape[0], 30, sampling=0.8, seed=3 + i)
    st = s.step(1)
    for i in short:                                       # taken and restarted with another prompt
        assert st[i] == "done", (i, st)
        assert s.take(i)[1] <= 3
        p = pool[(i + 1) % 4]
        s.start(i, p, p.shape[0], 30, sampling=True, seed=8 + i)
    crowded = run_to_end(s, mine)
    s.free()
    for slot in mine:
        assert same(crowded[slot], ref), (slot, "among 30 other prompts that start, end and restart around it")


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [17, 64])
def test_wide_slots_against_the_golden_and_the_one_utterance_call(S):
    eng, P, spec = prompts(B3)
    c = MAN["cases"][B3]
    g = golden(B3)
    nq, M = spec.predict_nq, c["max_length"]
    at = sorted({0, 16, S - 1})                           # at S = 17 slot 16 is the last one
    s = eng.open_decode(S, max_positions=64, wide=True)
    for b, slot in enumerate(at):
        forced = np.zeros((M, nq), np.int64)
        t = g[f"tokens_{b}"].astype(np.int64)
        forced[: t.shape[0]] = t
        s.start(slot, P[b], P[b].shape[0], M, sampling=False, forced=torch.from_numpy(forced))
    got = run_to_end(s, at)
    worst = 0.0
    for b, slot in enumerate(at):
        ref_lp = torch.from_numpy(g[f"logp_{b}"])
        n = min(ref_lp.shape[0], g[f"tokens_{b}"].shape[0] + 1, M)
        err = float((got[slot][2].cpu()[:n] - ref_lp[:n]).abs().max())
        worst = max(worst, err)
        assert err < LOGP_TOL, (S, slot, err)
    print("S", S, "forced, max |logp - golden|", worst)
    # greedy, every slot running: slot i holds prompt i % 3
    steps = 10
    alone = [eng.decode_codec(p[None], [p.shape[0]], steps, sampling=False, return_logp=True) for p in P]
    for i in range(S):
        p = P[i % 3]
        s.start(i, p, p.shape[0], steps, sampling=False)
    got = run_to_end(s, range(S))
    s.free()
    worst = 0.0
    for i in range(S):
        t1, o1, l1 = alone[i % 3]
        assert got[i][1] == o1[0] and torch.equal(got[i][0], t1[0, : o1[0]]), (S, i)
        worst = max(worst, float((got[i][2] - l1[0]).abs().max()))
    print("S", S, "greedy, max |logp - alone|", worst)
    assert worst < 2e-5, (S, worst)


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_the_session_calls_on_high_slots():
    from funcodec_amd.laura import SamplingRules
    eng, P, spec = prompts(B3)
    keep = 3

    def run(a, b, c, d, e):
        """start_many into {a, b, c}, start_from(d, a), fork(e, c, keep), rewind(c, keep), rules on a: two sessions of ONE width (one key-
        range split), the slots in high or low column blocks"""
        s = eng.open_decode(20, max_positions=64, score=True, wide=True)
        s.start_many({a: dict(text_outs=P[0], text_len=P[0].shape[0], max_length=12, sampling=True, seed=41),
                      b: dict(text_outs=P[1], text_len=P[1].shape[0], max_length=12, sampling=5, seed=42),
                      c: dict(text_outs=P[2], text_len=P[2].shape[0], max_length=12, sampling=True, seed=43)})
        s.step(3)
        s.start_from(d, a, 11, sampling=0.8, seed=44)
        s.step(2)
        assert s.n_gen(c) == 6
        s.fork(e, c, keep, sampling=True, seed=45)
        s.rewind(c, keep, sampling=True, seed=46)
        s.rewind(a, 2, sampling=5, seed=47, rules=SamplingRules(temperature=0.8, min_length=12, top_p=0.9))
        order = (a, b, c, d, e)
        for _ in range(32):
            st = s.step(1)
            if all(st.get(i) != "running" for i in order):
                break
        out = [s.take(i, return_logp=True, return_score=True) for i in order]
        s.free()
        return out

    high, low = run(17, 2, 19, 18, 16), run(1, 2, 3, 4, 0)
    for k, (h, l) in enumerate(zip(high, low)):
        assert same(h, l), k
        assert h[3] == l[3] and h[3][1] > 0, (k, h[3], l[3])


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_slot_and_change_nothing():
    from funcodec_amd.engine import EngineError
    eng, P, spec = prompts(B3)
    with pytest.raises(EngineError, match=r"1 \.\. 64 slots"):
        eng.open_decode(65, wide=True)
    with pytest.raises(EngineError, match=r"1 \.\. 16 slots"):
        eng.open_decode(17)
    # the library's own refusals, past the binding's check
    import ctypes
    from funcodec_amd import _lib
    h = ctypes.c_void_p()
    for bad in (65, 0):
        assert eng.lib.fc_laura_slots_state_bytes_wide(eng._h, bad, 64, 0, 0) == 0
        assert eng.lib.fc_laura_slots_create_wide(eng._h, bad, 64, 0, 0, None, 0, ctypes.byref(h)) != 0
        assert "1 .. 64 slots" in _lib.last_error() and f"got {bad}" in _lib.last_error()
        assert not h.value
    assert eng.lib.fc_laura_slots_state_bytes_wide(eng._h, 64, 64, 0, 0) > eng.lib.fc_laura_slots_state_bytes_wide(eng._h, 17, 64, 0, 0) > 0
    assert eng.lib.fc_laura_slots_state_bytes_scored(eng._h, 17, 64, 0, 0) == 0
    assert eng.lib.fc_laura_slots_create_scored(eng._h, 17, 64, 0, 0, None, 0, ctypes.byref(h)) != 0
    assert "1 .. 16 slots" in _lib.last_error()

    def session(with_refusals):
        s = eng.open_decode(33, max_positions=32, wide=True)
        s.start(32, P[0], P[0].shape[0], 10, sampling=True, seed=21)
        s.step(3)
        if with_refusals:
            with pytest.raises(EngineError, match="slot 33"):
                s.start(33, P[1], P[1].shape[0], 5)
            with pytest.raises(EngineError, match=r"slot 32.*max_positions 32"):
                s.start(32, P[1], P[1].shape[0], 40, sampling=False)                   # the RUNNING high slot: it must go on
            with pytest.raises(EngineError, match=r"slot 20.*max_positions 32"):
                s.start_from(20, 32, 40)
            with pytest.raises(EngineError, match=r"slot 32.*keep 9"):
                s.rewind(32, 9)
            with pytest.raises(EngineError, match="source slot 33"):
                s.fork(20, 33)
            with pytest.raises(EngineError, match="slot 32 has not ended"):
                s.take(32)
            with pytest.raises(EngineError, match="slot 17"):
                s.start_many({i: dict(text_outs=P[1], text_len=P[1].shape[0], max_length=5) for i in range(1, 18)})     # 17 prompts
        r = run_to_end(s, [32])[32]
        s.free()
        return r

    assert same(session(True), session(False))


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_generate_many_through_a_wide_session(tmp_path):
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
    from funcodec_amd.synth import make_laura_state_dict, make_state_dict, write_checkpoint
    c = MAN["e2e"]["laura_e2e_tinyphn_ds320"]
    lcfg = laura_recipe_config(c["laura_config"])
    spec = laura_spec_from_config(lcfg)
    lsd = make_laura_state_dict(lcfg, c["laura_seed"])
    ccfg = recipe_config(c["codec_config"])
    csd = make_state_dict(arch_from_config(ccfg), c["codec_seed"])
    lsd["quantizer_codebook.embed"] = csd["quantizer.rq.model.embed"][: spec.num_quantizers].copy()
    lc, lp = write_checkpoint(str(tmp_path / "laura"), lcfg, lsd)
    cc, cp = write_checkpoint(str(tmp_path / "codec"), ccfg, csd)
    t2a = Text2Audio(config_file=lc, model_file=lp, device="cuda", text_emb_model=None, beam_size=1, sampling=True, continual=True,
                     codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False, exclude_prompt=True, max_length=14,
                     max_positions=256)
    words = c["text"].split(" ")
    texts = [" ".join(words[i % 3: 4 + i % 5]) for i in range(24)]          # more prompts than slots: some slots are refilled
    seeds = [100 + i for i in range(24)]
    _, wide = t2a.generate_many(texts, slots=20, seeds=seeds)
    _, narrow = t2a.generate_many(texts, slots=4, seeds=seeds)
    assert len(wide) == len(narrow) == 24
    for i in range(24):
        assert wide[i].shape == narrow[i].shape and torch.equal(wide[i], narrow[i]), i
