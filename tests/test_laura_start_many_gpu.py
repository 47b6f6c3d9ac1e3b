"""Several DIFFERENT prompts per prefix pass, held for free slots, on the GPU: DecodeSlots.start_many, start_from(source=another
session), Text2Audio.generate_many(prefill=P).  The contract pinned here is equality of BITS: a slot started as one row of a B-row prefix
pass padded to the longest prompt, or by a copy from a row of a holding session, is the slot ``start`` gives for the same prompt and
parameters -- tokens, per-step log-probabilities and score terms by torch.equal, never a tolerance.  The ``start`` it is compared with
runs in a twin session of the same slot count (the key ranges per head depend on S).

Prompts are seeded random text_outs (``start`` takes them as given) on the laura_tiny_b3 checkpoint with max_positions 1024.  Prefix
lengths P = text_len + 2 + cont_len in one call: 7, 16, 17, 33, 128, 129, 257, 300 -- both pad4 classes, a 16-key tile edge of the
attention, the 128- and 256-column tile edges of the Linear kernel, several blocks of every kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_laura import case_inputs, laura_engine
from test_laura_slots_gpu import B3

pytestmark = pytest.mark.gpu

PS = [7, 16, 17, 33, 128, 129, 257, 300]
TEXT = [3, 5, 4, 6, 3, 7, 5, 4]                   # text tokens of prompt i when the rest of its prefix is a continual prompt
STEPS, CAP = 12, 320                              # 12 steps behind the start's sample: max_length 13;  CAP >= 300 + 13
MODES = [(False, 0), (True, 1234), (5, 7), (0.7, 9)]
_eng = {}


def engine():
    """The laura_tiny_b3 checkpoint in an engine of 1024 positions (the fixture's own has 256)."""
    if "e" not in _eng:
        from funcodec_amd.laura import LauraGenMI355X
        _, _, spec, sd, _, _ = case_inputs(B3)
        m = LauraGenMI355X(spec, "cuda:0", max_positions=1024)
        m.load_state_dict(sd)
        _eng["e"], _eng["spec"] = m.engine, spec
    return _eng["e"], _eng["spec"]


def prompt(i, P, cont=True, seed=0):
    """Prompt i of prefix length P: (text_outs [tl, D], continual [P - 2 - tl, nq] or None), a function of (i, P, cont, seed)."""
    _, spec = engine()
    rng = np.random.Generator(np.random.PCG64(1000 * seed + 10 * P + i))
    tl = TEXT[i % len(TEXT)] if cont and P - 2 - TEXT[i % len(TEXT)] >= 0 else P - 2
    text = torch.from_numpy(rng.standard_normal((tl, spec.codebook_dim)).astype(np.float32))
    cl = P - 2 - tl
    c = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(cl, spec.predict_nq)).astype(np.int64)) if cl else None
    return text, c


def request(p, max_length, sampling, seed, rules=None):
    return dict(text_outs=p[0], text_len=p[0].shape[0], max_length=max_length, sampling=sampling, seed=seed, continual=p[1], rules=rules)


def finish(sess, slots, steps=STEPS):
    """`steps` steps, then for every slot (length, tokens, log-probability rows, score row, score count): all must have ended."""
    for _ in range(steps):
        st = sess.step(1)
    assert all(st.get(s) == "done" for s in slots), st
    out = {}
    for s in slots:
        row, count, end = sess.score_row(s)
        tokens, n, logp = sess.take(s, return_logp=True)
        out[s] = (n, tokens.cpu(), logp.cpu(), row, count)
    return out


def assert_same(got, ref, what=""):
    assert got[0] == ref[0] and got[4] == ref[4], (what, got[0], ref[0])
    assert torch.equal(got[1], ref[1]), (what, "tokens")
    assert torch.equal(got[2], ref[2]), (what, "log-probabilities", float((got[2] - ref[2]).abs().max()))
    assert torch.equal(got[3], ref[3]), (what, "score terms", float((got[3] - ref[3]).abs().max()))


def one_by_one(eng, S, reqs, cap=CAP, steps=STEPS):
    """The twin: the same requests, slot by slot through ``start``."""
    s = eng.open_decode(S, max_positions=cap, logp=True, score=True)
    for slot, r in reqs.items():
        s.start(slot, r["text_outs"], r["text_len"], r["max_length"], sampling=r["sampling"], seed=r["seed"], continual=r["continual"],
                rules=r["rules"])
    assert s.prefix_passes == len(reqs)
    out = finish(s, list(reqs), steps)
    s.free()
    return out


def many(eng, S, reqs, cap=CAP, steps=STEPS):
    s = eng.open_decode(S, max_positions=cap, logp=True, score=True)
    s.start_many(reqs)
    assert s.prefix_passes == 1
    out = finish(s, list(reqs), steps)
    s.free()
    return out


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cont", [True, False])
@pytest.mark.parametrize("sampling,seed", MODES)
def test_start_many_is_start_bit_for_bit(sampling, seed, cont):
    eng, _ = engine()
    reqs = {i: request(prompt(i, P, cont), STEPS + 1, sampling, seed + i) for i, P in enumerate(PS)}
    assert sorted(r["text_len"] + 2 + (0 if r["continual"] is None else r["continual"].shape[0]) for r in reqs.values()) == PS
    got, ref = many(eng, 8, reqs), one_by_one(eng, 8, reqs)
    for slot in reqs:
        assert_same(got[slot], ref[slot], (slot, PS[slot], sampling))


def test_rules_on_one_slot_and_every_mode_in_one_call():
    from funcodec_amd.laura import SamplingRules
    eng, _ = engine()
    rules = SamplingRules(temperature=0.8, min_length=4, top_p=0.9, repeat_window=4, repeat_count=2)
    reqs = {i: request(prompt(i, P), STEPS + 1, MODES[i % 4][0], 40 + i) for i, P in enumerate(PS)}
    reqs[2] = request(prompt(2, PS[2]), STEPS + 1, 5, 42, rules)             # top_p goes with an integer `sampling`
    got, ref = many(eng, 8, reqs), one_by_one(eng, 8, reqs)
    for slot in reqs:
        assert_same(got[slot], ref[slot], slot)
    neutral = one_by_one(eng, 8, {2: request(prompt(2, PS[2]), STEPS + 1, 5, 42)})[2]
    assert not torch.equal(neutral[3], ref[2][3]), "the rules reach the slot (temperature changes every score term)"


@pytest.mark.parametrize("S,slots", [(1, [0]), (4, [2]), (16, list(range(16))), (6, [5, 0, 3])])
def test_one_prompt_a_full_session_and_slots_in_any_order(S, slots):
    eng, _ = engine()
    reqs = {slot: request(prompt(j, PS[(3 * j + 1) % len(PS)]), STEPS + 1, MODES[j % 4][0], 7 + j) for j, slot in enumerate(slots)}
    got, ref = many(eng, S, reqs), one_by_one(eng, S, reqs)
    for slot in slots:
        assert_same(got[slot], ref[slot], (S, slot))


# 2 ---------------------------------------------------------------------------------------------------------------------------
def raw_start_many(sess, slots, text, tls, cont, cls, max_length, sampling, seeds):
    """fc_laura_slots_start_many on buffers of the test's own making (the wrapper cuts every prompt to its length and pads with zeros,
    so what lies behind a row's length never reaches the library through it)."""
    from funcodec_amd.laura import _i32, sampling_args
    eng, n = sess.engine, len(slots)
    mode, k, p = sampling_args(sampling)
    text, cont = text.cuda().contiguous(), cont.cuda().contiguous()
    L, Cmax = text.shape[1], cont.shape[1]
    need = int(sess.lib.fc_laura_slots_start_many_workspace_bytes(sess._handle(), n, L, Cmax))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    cur, run = sess._run_stream()
    eng._check(sess.lib.fc_laura_slots_start_many(
        sess._handle(), n, _i32(slots), C.c_void_p(text.data_ptr()), _i32(tls), L, C.c_void_p(cont.data_ptr()), _i32(cls), Cmax,
        _i32([max_length] * n), _i32([mode] * n), _i32([k] * n), (C.c_float * n)(*[p] * n), (C.c_uint64 * n)(*seeds),
        C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(run.cuda_stream)))
    if run is not cur:
        cur.wait_stream(run)
    torch.cuda.synchronize()
    for s in slots:
        sess._max_length[s] = max_length


def test_nothing_outside_a_row_reaches_it():
    eng, spec = engine()
    Ps = [7, 17, 128, 33, 300, 16]
    P = [prompt(i, p) for i, p in enumerate(Ps)]
    reqs = {i: request(P[i], STEPS + 1, True, 70 + i) for i in range(6)}
    ref = one_by_one(eng, 6, reqs)
    # NaN behind every row's text_len, other valid ids behind every row's cont_len
    L, Cmax = max(p[0].shape[0] for p in P) + 3, max(p[1].shape[0] for p in P) + 5
    text = torch.full((6, L, spec.codebook_dim), float("nan"))
    rng = np.random.Generator(np.random.PCG64(5))
    cont = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(6, Cmax, spec.predict_nq)).astype(np.int64))
    for i, (t, c) in enumerate(P):
        text[i, : t.shape[0]] = t
        cont[i, : c.shape[0]] = c
    s = eng.open_decode(6, max_positions=CAP, logp=True, score=True)
    raw_start_many(s, list(range(6)), text, [p[0].shape[0] for p in P], cont, [p[1].shape[0] for p in P], STEPS + 1, True,
                   [70 + i for i in range(6)])
    got = finish(s, list(range(6)))
    s.free()
    for i in range(6):
        assert_same(got[i], ref[i], ("padding", i))
    # every prompt alone, and in another batch with another longest prompt (in the same slot of a session of the same S)
    for i in range(6):
        alone = many(eng, 6, {i: reqs[i]})[i]
        assert_same(alone, ref[i], ("alone", i))
    other = {5: request(prompt(7, 257, seed=3), STEPS + 1, 5, 1)}
    for group in ([0, 1, 3], [2, 4]):
        got = many(eng, 6, {**{i: reqs[i] for i in group}, **other})
        for i in group:
            assert_same(got[i], ref[i], ("another batch", i))


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_neighbours_in_the_middle_of_their_utterances_are_not_disturbed():
    eng, _ = engine()
    A, B = prompt(0, 17), prompt(1, 33)
    late = {5: request(prompt(2, 129), 6, True, 3), 0: request(prompt(3, 7), 6, 5, 4), 3: request(prompt(4, 300), 6, 0.7, 5)}

    def run(disturb):
        s = eng.open_decode(6, max_positions=CAP, logp=True, score=True)
        s.start(1, A[0], A[0].shape[0], STEPS + 1, sampling=True, seed=11, continual=A[1])
        s.start(4, B[0], B[0].shape[0], STEPS + 1, sampling=5, seed=12, continual=B[1])
        s.step(3)
        if disturb:
            s.start_many(late)
        out = finish(s, [1, 4], STEPS - 3)
        s.free()
        return out

    def check(form):
        quiet, busy = run(False), run(True)
        for slot in (1, 4):
            assert_same(busy[slot], quiet[slot], (form, slot))

    assert eng.set_persistent_step(True)
    check("persistent step")
    try:
        assert not eng.set_persistent_step(False)
        check("kernel chain")
    finally:
        assert eng.set_persistent_step(True)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_names_the_slot_and_changes_nothing():
    from funcodec_amd.engine import EngineError
    from funcodec_amd.laura import SamplingRules
    eng, _ = engine()
    A, B, X = prompt(0, 17), prompt(1, 16), prompt(2, 33)
    ok = request(X, 5, True, 1)

    def session(with_refusals):
        s = eng.open_decode(4, max_positions=64, logp=True, score=True)
        s.start(1, A[0], A[0].shape[0], STEPS + 1, sampling=True, seed=21, continual=A[1])
        s.start(3, B[0], B[0].shape[0], STEPS + 1, sampling=0.7, seed=2, continual=B[1])
        s.step(3)
        if with_refusals:
            with pytest.raises(EngineError, match="slot 2 is named twice"):
                s.start_many([(2, ok), (1, ok), (2, ok)])
            with pytest.raises(EngineError, match="slot 4 outside"):
                s.start_many({1: ok, 4: ok})
            with pytest.raises(EngineError, match=r"slot \d+"):
                s.start_many({i: ok for i in range(17)})                     # n = 17
            with pytest.raises(EngineError, match=r"slot \d+"):
                s.start_many({i: ok for i in range(5)})                      # n > S
            with pytest.raises(EngineError, match=r"slot 3.*max_positions 64"):
                s.start_many({0: ok, 1: ok, 3: request(X, 64 - 33 + 1, True, 1)})        # one row one position too long
            # the library's own checks, behind the wrapper's: the same refusals from the C entry point
            raw = dict(text=torch.zeros(3, 4, 128), tls=[4, 4, 4], cont=torch.zeros(3, 1, 2, dtype=torch.int64), cls=[0, 0, 0])
            with pytest.raises(EngineError, match="slot 2 is named twice"):
                raw_start_many(s, [2, 3, 2], max_length=5, sampling=True, seeds=[1, 2, 3], **raw)
            with pytest.raises(EngineError, match="slot 7 outside"):
                raw_start_many(s, [0, 7, 2], max_length=5, sampling=True, seeds=[1, 2, 3], **raw)
            with pytest.raises(EngineError, match=r"slot 3.*max_positions 64"):
                raw_start_many(s, [3, 2, 0], max_length=64 - 6 + 1, sampling=True, seeds=[1, 2, 3], **raw)
            with pytest.raises(EngineError, match=r"slot 0.*sampling_k"):
                raw_start_many(s, [0, 2, 3], max_length=5, sampling=0, seeds=[1, 2, 3], **raw)
            # last: the wrapper hands a row's rules to the library ahead of the call, where they wait for the slot's next start
            with pytest.raises(EngineError, match=r"slot 1.*top-k"):
                s.start_many({0: request(X, 5, 5, 1, SamplingRules(top_p=0.9)), 1: request(X, 5, 0.7, 1, SamplingRules(top_p=0.9))})
            assert s.prefix_passes == 2
        out = finish(s, [1, 3], STEPS - 3)
        s.free()
        return out

    a, b = session(True), session(False)
    for slot in (1, 3):
        assert_same(a[slot], b[slot], slot)
    s = eng.open_decode(4, max_positions=64)
    s.start_many({3: request(X, 64 - 33, False, 0)})                         # exactly max_positions: accepted
    s.free()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_a_slot_imported_from_a_holding_session_is_a_start():
    from funcodec_amd.engine import EngineError
    eng, _ = engine()
    held = eng.open_decode(3, max_positions=512, logp=False)                 # K pitch 512; never stepped
    main = eng.open_decode(4, max_positions=1024, logp=True, score=True)     # K pitch 1024
    twin = eng.open_decode(4, max_positions=1024, logp=True, score=True)

    def round_(prompts, seed0):
        held.start_many({row: request(p, 1, False, 0) for row, p in enumerate(prompts)})
        plan = {0: (1, True, seed0), 2: (1, 5, seed0 + 1), 3: (0, 0.7, seed0 + 2), 1: (2, False, 0)}    # slot: (held row, sampling, seed)
        for slot, (row, sampling, seed) in plan.items():
            main.start_from(slot, row, STEPS + 1, sampling=sampling, seed=seed, source=held)
            p = prompts[row]
            twin.start(slot, p[0], p[0].shape[0], STEPS + 1, sampling=sampling, seed=seed, continual=p[1])
        got, ref = finish(main, list(plan)), finish(twin, list(plan))
        for slot in plan:
            assert_same(got[slot], ref[slot], (seed0, slot))
        assert not torch.equal(got[0][1], got[2][1]), "one held row, two seeds: two utterances"

    round_([prompt(0, 9), prompt(1, 129), prompt(2, 300)], 50)
    round_([prompt(3, 257), prompt(4, 16, cont=False), prompt(5, 33)], 60)    # the holding session refilled through start_many
    assert held.prefix_passes == 2 and main.prefix_passes == 0 and twin.prefix_passes == 8

    # refusals: nothing changes for the destination (slot 0 of `main` is free; it stays free)
    other = laura_engine(B3).engine.open_decode(2, max_positions=64)         # the same weights in ANOTHER engine
    p = prompt(0, 9)
    other.start(0, p[0], p[0].shape[0], 4, continual=p[1])
    with pytest.raises(EngineError, match=r"slot 0.*another engine"):
        main.start_from(0, 0, 5, source=other)
    other.free()
    fresh = eng.open_decode(3, max_positions=512, logp=False)
    fresh.start_many({0: request(p, 1, False, 0)})
    with pytest.raises(EngineError, match=r"source slot 2.*free or never started"):
        main.start_from(0, 2, 5, source=fresh)
    with pytest.raises(EngineError, match=r"source slot 3 outside"):
        main.start_from(0, 3, 5, source=fresh)
    with pytest.raises(EngineError, match=r"slot 0.*max_positions 1024"):
        main.start_from(0, 0, 1024 - 9 + 1, source=fresh)
    small = eng.open_decode(2, max_positions=16)
    with pytest.raises(EngineError, match=r"slot 1.*max_positions 16"):
        small.start_from(1, 0, 8, source=fresh)                               # 9 + 8 > 16: the DESTINATION's bound
    small.start_from(1, 0, 7, source=fresh)                                   # exactly 16: accepted
    assert main.step(1) == {}, "a refused import started nothing"
    for s in (held, main, twin, fresh, small):
        s.free()


# 6 ---------------------------------------------------------------------------------------------------------------------------
_t2a = {}


@pytest.mark.parametrize("kw", [dict(), dict(samples=2), dict(samples=2, keep="best", retries=1)], ids=["plain", "samples", "best"])
def test_generate_many_with_prefill_is_generate_many(kw, tmp_path_factory):
    from test_laura_score_gpu import tiny_t2a
    if "t" not in _t2a:
        _t2a["t"] = tiny_t2a(tmp_path_factory.mktemp("laura_prefill"), 12)
    t2a, words = _t2a["t"]
    texts = [" ".join(words[a:b]) for a, b in ((0, 4), (1, 6), (2, 9), (0, 7), (3, 8), (4, 9))]      # six prompts, different lengths
    N = kw.get("samples", 1)
    seeds = [100 + i for i in range(6)] if N == 1 else [[100 + 10 * i + k for k in range(N)] for i in range(6)]
    ref = t2a.generate_many(texts, slots=2, seeds=seeds, **kw)
    assert t2a.last_prefix_passes["held"] == 0 and t2a.last_prefix_passes["main"] >= 6
    got = t2a.generate_many(texts, slots=2, seeds=seeds, prefill=4, **kw)
    assert t2a.last_prefix_passes == {"main": 0, "held": 2}, t2a.last_prefix_passes      # ceil(6 / 4) passes, all in the holding session

    def flat(x):
        return [x] if isinstance(x, (dict, torch.Tensor)) else [v for y in x for v in flat(y)]

    rets, codecs = flat(got[0]), flat(got[1])
    rrets, rcodecs = flat(ref[0]), flat(ref[1])
    assert len(rets) == len(rrets) == len(codecs) == len(rcodecs) == (6 if kw.get("keep") == "best" else 6 * N)
    for i, (a, b) in enumerate(zip(codecs, rcodecs)):
        assert torch.equal(a, b), ("tokens", i)
    for i, (a, b) in enumerate(zip(rets, rrets)):
        for part in ("gen", "gen_only_lm"):
            assert torch.equal(a[part], b[part]), (part, i)
    if kw.get("keep") == "best":
        assert got[2] == ref[2], "the same candidate kept, with the same mean"
