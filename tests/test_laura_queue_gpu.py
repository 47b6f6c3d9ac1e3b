"""Queued decoding sessions on the GPU: open_decode(queue=, source=), DecodeSlots.submit / claimed / collect,
Text2Audio.generate_many(queue=True).  Tickets wait on the device; inside every captured step ended slots retire into a result ring and
free slots claim the oldest tickets.  The contract pinned here is equality of BITS: a claimed slot is the slot
``start_from(slot, row, source=held, ...)`` gives, so a ticket's tokens, score row, count and end flag are torch.equal / == to those
of a twin session of the same slot count WITHOUT a queue (the key ranges per head depend on S), whatever slot the ticket landed in,
the step it was claimed at, its neighbours and the n of step(n).

laura_tiny_b3 checkpoint, max_positions 320, the prompts of test_laura_start_many_gpu.py: prefix lengths 7, 16, 17, 33, 128, 129, 257,
300 -- both pad4 classes, a 16-key tile edge, one and several 1024-vector chunks of the copy kernel per layer."""
import pytest
import torch

from test_laura_start_many_gpu import CAP, MODES, PS, engine, prompt, request

pytestmark = pytest.mark.gpu

LENGTHS = [5, 5, 13, 1, 2, 13, 2, 5]              # max_length of ticket i: see test_a_ticket_is_start_from_bit_for_bit


def hold(eng, prompts, rows=None, cap=CAP):
    """a holding session with prompts[i] in row i; a row whose prompt is None is never started and holds NaN keys and values"""
    held = eng.open_decode(rows or len(prompts), max_positions=cap, logp=False)
    held.start_many({row: request(p, 1, False, 0) for row, p in enumerate(prompts) if p is not None})
    empty = [row for row in range(held.slots) if row >= len(prompts) or prompts[row] is None]
    if empty:
        poison(held, empty, {row: p[0].shape[0] + 2 + (0 if p[1] is None else p[1].shape[0]) for row, p in enumerate(prompts) if p is not None})
    return held


def poison(held, rows, started):
    """NaN into every key and value the holding session keeps for `rows`, which no ticket may name.  The session's state begins with
    its positions [S] and counters [3 S + 4] (ints), then keys [layers][S][d][R] and values [layers][S][R][d] (floats), every part on a
    256-byte boundary.  The views are checked before anything is written: they are zero except the started rows' first P positions,
    which hold a prompt."""
    _, spec = engine()
    S, R, d, NL = held.slots, held.max_positions, spec.codec_lm.d_model, spec.codec_lm.layers
    a256 = lambda n: (n + 255) & ~255
    n = NL * S * d * R
    k0 = a256(a256(4 * S) + 4 * (3 * S + 4))
    v0 = a256(k0 + 4 * n)
    assert held.state.data_ptr() % 256 == 0
    K = held.state[k0: k0 + 4 * n].view(torch.float32).view(NL, S, d, R)
    V = held.state[v0: v0 + 4 * n].view(torch.float32).view(NL, S, R, d)
    torch.cuda.synchronize()
    for row in range(S):
        P = started.get(row, 0)
        P4 = (P + 3) & ~3
        assert not K[:, row, :, P4:].any() and not V[:, row, P4:, :].any(), ("the state's layout is not the one assumed", row)
        if P:
            assert bool((K[:, row, :, :P] != 0).any(dim=1).all()) and bool((V[:, row, :P, :] != 0).any(dim=2).all()), row
    for row in rows:
        assert row not in started
        K[:, row] = float("nan")
        V[:, row] = float("nan")
    torch.cuda.synchronize()


def run_queue(qs, step_n=1, limit=400):
    """step(step_n) until nothing waits or runs; {ticket: (tokens, len, score row, count, end)}, and per step call (claimed, finished)"""
    out, trace = {}, []
    for _ in range(limit):
        if not qs.pending:
            break
        st = qs.step(step_n)
        assert set(st.values()) <= {"running"}, st        # a queued session retires what ended before it reads back
        assert set(st) == set(qs.slot_tickets()), (st, qs.slot_tickets())
        trace.append((qs.claimed, qs.finished))
        for t, tokens, n, score in qs.collect(score_rows=True):
            assert t not in out and tokens is not None
            out[t] = (tokens.cpu(), n) + (score if score is not None else (None, None, None))
    assert not qs.pending
    return out, trace


def twin(eng, held, S, tickets, cap=CAP, **more):
    """the tickets [(row, max_length, sampling, seed, rules)] through start_from(source=held) in a session of S slots without a queue,
    S at a time, each stepped to its end: [(tokens, len, score row, count, end)]"""
    s = eng.open_decode(S, max_positions=cap, logp=False, score=True, **more)
    out = []
    for i0 in range(0, len(tickets), S):
        group = tickets[i0: i0 + S]
        for slot, (row, ml, sampling, seed, rules) in enumerate(group):
            s.start_from(slot, row, ml, sampling=sampling, seed=seed, rules=rules, source=held)
        for _ in range(max(t[1] for t in group)):
            st = s.step(1)
        assert all(st.get(slot) == "done" for slot in range(len(group))), st
        for slot in range(len(group)):
            row, count, end = s.score_row(slot)
            tokens, n = s.take(slot)
            out.append((tokens.cpu(), n, row, count, end))
    s.free()
    return out


def assert_same(got, ref, what):
    assert got[1] == ref[1] and got[3] == ref[3] and got[4] == ref[4], (what, got[1:2] + got[3:], ref[1:2] + ref[3:])
    assert torch.equal(got[0], ref[0]), (what, "tokens")
    assert torch.equal(got[2], ref[2]), (what, "score terms", float((got[2] - ref[2]).abs().max()))


def submit_all(qs, tickets):
    for i, (row, ml, sampling, seed, rules) in enumerate(tickets):
        assert qs.submit(row, ml, sampling, seed, rules) == i


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling,seed", MODES)
def test_a_ticket_is_start_from_bit_for_bit(sampling, seed):
    """S = 3, eight tickets.  Tickets 0, 1 (max_length 5) and 2 (13) are claimed in step 1; 0 and 1 end in the same step, both slots
    retire and claim tickets 3 (max_length 1: it ends at its first sample) and 4 (2) in one step, and so on."""
    eng, _ = engine()
    held = hold(eng, [prompt(i, P) for i, P in enumerate(PS)])
    tickets = [(row, LENGTHS[row], sampling, seed + row, None) for row in range(8)]
    qs = eng.open_decode(3, max_positions=CAP, logp=False, score=True, queue=8, source=held)
    submit_all(qs, tickets)
    assert qs.claimed == 0 and qs.pending == 8
    got, trace = run_queue(qs)
    ref = twin(eng, held, 3, tickets)
    for i in range(8):
        assert_same(got[i], ref[i], (i, PS[i], sampling))
    assert trace[0][0] == 3, "a fresh session fills all its slots in its first step"
    claims = [b[0] - a[0] for a, b in zip(trace, trace[1:])]
    ends = [b[1] - a[1] for a, b in zip(trace, trace[1:])]
    assert max(claims) >= 2 and max(ends) >= 2, (trace, "two slots ended in one step and were refilled in one step")
    assert ref[3][3] == 1, "ticket 3 (max_length 1) ended at its first sample: one scored step"
    assert qs.prefix_passes == 0 and held.prefix_passes == 1
    qs.free()
    held.free()


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_a_ticket_depends_on_its_row_and_parameters_only():
    eng, _ = engine()
    X = prompt(2, 17)
    mine = (None, 13, True, 77, None)                 # the ticket under test: (row, max_length, sampling, seed, rules)
    others = [prompt(i, P) for i, P in enumerate(PS) if P != 17]
    held1 = hold(eng, [None, None, X, None])          # the rows no ticket names hold NaN
    ref = twin(eng, held1, 3, [(2,) + mine[1:]])[0]

    def alone(step_n):
        qs = eng.open_decode(3, max_positions=CAP, logp=False, score=True, queue=4, source=held1)
        submit_all(qs, [(2,) + mine[1:]])
        got, _ = run_queue(qs, step_n)
        qs.free()
        return got[0]

    for step_n in (1, 5, 16):
        assert_same(alone(step_n), ref, ("alone", step_n))
    held1.free()
    held8 = hold(eng, others + [X])
    seven = [(row, LENGTHS[row], MODES[row % 4][0], 5 + row, None) for row in range(7)]
    # last behind seven others
    qs = eng.open_decode(3, max_positions=CAP, logp=False, score=True, queue=8, source=held8)
    submit_all(qs, seven + [(7,) + mine[1:]])
    got, _ = run_queue(qs, 5)
    assert_same(got[7], ref, "last behind seven others")
    qs.free()
    # submitted between two step calls of a running session
    qs = eng.open_decode(3, max_positions=CAP, logp=False, score=True, queue=8, source=held8)
    submit_all(qs, seven[:4])
    qs.step(3)
    assert qs.submit(7, *mine[1:]) == 4
    got, _ = run_queue(qs, 16)
    assert_same(got[4], ref, "submitted into a running session")
    qs.free()
    held8.free()


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_samples_of_one_row_and_the_row_overwritten_once_claimed():
    eng, _ = engine()
    A, B = prompt(4, 128), prompt(5, 33)
    held = hold(eng, [None, A], rows=2)
    tickets = [(1, 13, MODES[k][0], 200 + k, None) for k in range(4)]
    ref = twin(eng, held, 2, tickets)
    qs = eng.open_decode(2, max_positions=CAP, logp=False, score=True, queue=4, source=held)
    submit_all(qs, tickets)
    got = {}
    while qs.claimed < 4:
        qs.step(1)
        got.update({t: (tok.cpu(), n) + sc for t, tok, n, sc in qs.collect(score_rows=True)})
    assert len(qs.slot_tickets()) == 2 and len(got) == 2, "tickets 2 and 3 are running from copies of the row"
    held.start_many({1: request(B, 1, False, 0)})      # every ticket of row 1 is claimed: the row may go
    rest, _ = run_queue(qs, 5)
    got.update(rest)
    for k in range(4):
        assert_same(got[k], ref[k], ("sample", k))
    assert not torch.equal(got[1][0], got[2][0]), "one held row, four seeds: different utterances"
    qs.free()
    held.free()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_an_utterance_that_ends_on_eos():
    from test_laura import MAN
    from test_laura_slots_gpu import EOS, prompts
    eng, Q, spec = prompts(EOS)
    assert MAN["cases"][EOS]["tokens"] == [6, 8]
    held = eng.open_decode(2, max_positions=64, logp=False)
    held.start_many({b: dict(text_outs=Q[b], text_len=Q[b].shape[0], max_length=1, sampling=False) for b in (0, 1)})
    tickets = [(0, 16, False, 0, None), (1, 16, False, 0, None)]
    ref = twin(eng, held, 3, tickets, cap=64)
    qs = eng.open_decode(3, max_positions=64, logp=False, score=True, queue=2, source=held)
    submit_all(qs, tickets)
    got, _ = run_queue(qs, 16)
    for b in (0, 1):
        assert_same(got[b], ref[b], ("eos", b))
        n = (6, 8)[b]
        assert got[b][1] == n and got[b][3] == n + 1 and got[b][4] == 2, got[b][1:]
        assert float(got[b][2][n]) < 0 and not got[b][2][n + 1:].any(), "the ending step has its term, nothing behind it"
    qs.free()
    held.free()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_back_pressure_and_refusals():
    from funcodec_amd.engine import EngineError
    from funcodec_amd.laura import SamplingRules
    eng, _ = engine()
    X = prompt(1, 33)
    held = hold(eng, [prompt(0, 17), X], rows=3)      # row 2 is never started
    ok = (1, 5, True, 9, None)
    ref = twin(eng, held, 2, [ok], cap=64)[0]
    with pytest.raises(EngineError, match="queue= needs logp=False"):
        eng.open_decode(2, max_positions=CAP, logp=True, queue=4, source=held)
    with pytest.raises(EngineError, match="queue= needs source="):
        eng.open_decode(2, max_positions=CAP, logp=False, queue=4)
    qs = eng.open_decode(2, max_positions=64, logp=False, score=True, queue=3, source=held)

    def runs_a_ticket():
        t = qs.submit(*ok)
        got, _ = run_queue(qs, 4)
        assert_same(got[t], ref, ("after the refusals", t))

    runs_a_ticket()
    n = qs.submitted
    with pytest.raises(EngineError, match=rf"ticket {n} \(row 1\).*max_positions 64"):
        qs.submit(1, 64 - 33 + 1, True, 1)
    qs.submit(1, 64 - 33, True, 1)                    # exactly max_positions: accepted (ticket n)
    with pytest.raises(EngineError, match=rf"ticket {n + 1} \(row 2\).*holds no prompt"):
        qs.submit(2, 5, True, 1)
    with pytest.raises(EngineError, match=rf"ticket {n + 1} \(row 3\).*outside"):
        qs.submit(3, 5, True, 1)
    with pytest.raises(EngineError, match=rf"ticket {n + 1} \(row 0\).*top-k"):
        qs.submit(0, 5, 0.7, 1, SamplingRules(top_p=0.9))
    with pytest.raises(EngineError, match=rf"ticket {n + 1} \(row 0\).*greedy"):
        qs.submit(0, 5, False, 1, SamplingRules(repeat_window=4, repeat_count=2))
    # back-pressure: queue = 3 results waiting, running or uncollected
    assert qs.submit(0, 2, True, 2) == n + 1 and qs.submit(0, 2, True, 3) == n + 2
    with pytest.raises(EngineError, match=rf"ticket {n + 3} \(row 0\).*result entries"):
        qs.submit(0, 2, True, 4)
    while qs.pending:
        qs.step(16)
    with pytest.raises(EngineError, match=rf"ticket {n + 3} \(row 0\).*result entries"):
        qs.submit(0, 2, True, 4)                       # finished, but uncollected
    assert sorted(t for t, *_ in qs.collect()) == [n, n + 1, n + 2]
    assert qs.submit(0, 2, True, 4) == n + 3           # collect made room
    run_queue(qs, 4)
    # a queued session is fed by its queue only
    P0 = prompt(0, 17)
    calls = [("start", lambda: qs.start(0, P0[0], P0[0].shape[0], 5, continual=P0[1])),
             ("start_many", lambda: qs.start_many({0: request(P0, 5, True, 1)})),
             ("start_from", lambda: qs.start_from(0, 1, 5)),
             ("start_from", lambda: qs.start_from(0, 1, 5, source=held)),
             ("fork", lambda: qs.fork(0, 1)),
             ("rewind", lambda: qs.rewind(0, 1)),
             ("take", lambda: qs.take(0))]
    for name, call in calls:
        with pytest.raises(EngineError, match=name + ": a queued session is fed by its queue only"):
            call()
    with pytest.raises(EngineError, match="opened without a queue"):
        held.submit(0, 5)
    runs_a_ticket()
    qs.free()
    held.free()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_a_wide_queued_session():
    eng, _ = engine()
    held = hold(eng, [prompt(i, P) for i, P in enumerate(PS)])
    tickets = [(i % 8, [1, 2, 5, 13][(i // 3) % 4], MODES[i % 4][0], 300 + i, None) for i in range(20)]
    qs = eng.open_decode(17, max_positions=CAP, logp=False, score=True, wide=True, queue=20, source=held)
    submit_all(qs, tickets)
    qs.step(1)
    assert qs.claimed == 17, "a fresh session fills all its slots in its first step"
    got, _ = run_queue(qs, 4)
    ref = twin(eng, held, 17, tickets, wide=True)
    for i in range(20):
        assert_same(got[i], ref[i], ("wide", i))
    qs.free()
    held.free()


# 7 ---------------------------------------------------------------------------------------------------------------------------
_t2a = {}


@pytest.mark.parametrize("kw", [dict(samples=2), dict(samples=2, keep="best")], ids=["samples", "best"])
def test_generate_many_with_a_queue_is_generate_many(kw, tmp_path_factory):
    from test_laura_score_gpu import tiny_t2a
    if "t" not in _t2a:
        _t2a["t"] = tiny_t2a(tmp_path_factory.mktemp("laura_queue"), 12)
    t2a, words = _t2a["t"]
    texts = [" ".join(words[a:b]) for a, b in ((0, 4), (1, 6), (2, 9), (0, 7), (3, 8), (4, 9))]
    seeds = [[100 + 10 * i + k for k in range(2)] for i in range(6)]
    ref = t2a.generate_many(texts, slots=2, seeds=seeds, prefill=4, **kw)
    got = t2a.generate_many(texts, slots=2, seeds=seeds, prefill=4, queue=True, **kw)
    assert t2a.last_prefix_passes["main"] == 0 and 2 <= t2a.last_prefix_passes["held"] <= 6, t2a.last_prefix_passes

    def flat(x):
        return [x] if isinstance(x, (dict, torch.Tensor)) else [v for y in x for v in flat(y)]

    rets, codecs, rrets, rcodecs = flat(got[0]), flat(got[1]), flat(ref[0]), flat(ref[1])
    assert len(rets) == len(rrets) == len(codecs) == len(rcodecs) == (6 if kw.get("keep") == "best" else 12)
    for i, (a, b) in enumerate(zip(codecs, rcodecs)):
        assert torch.equal(a, b), ("tokens", i)
    for i, (a, b) in enumerate(zip(rets, rrets)):
        for part in ("gen", "gen_only_lm"):
            assert torch.equal(a[part], b[part]), (part, i)
    if kw.get("keep") == "best":
        assert got[2] == ref[2], "the same candidate kept, with the same mean"
    with pytest.raises(ValueError, match="retries = 0"):
        t2a.generate_many(texts, slots=2, seeds=seeds, prefill=4, queue=True, retries=1, **kw)
    with pytest.raises(ValueError, match="prefill >= 1"):
        t2a.generate_many(texts, slots=2, seeds=seeds, queue=True, **kw)


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_a_timed_out_persistent_step_fails_the_running_tickets_and_the_queue_goes_on(monkeypatch):
    eng, _ = engine()
    held = hold(eng, [prompt(0, 17), prompt(1, 33)])
    tickets = [(i % 2, 6, True, 40 + i, None) for i in range(5)]
    assert eng.set_persistent_step(True)
    qs = eng.open_decode(2, max_positions=CAP, logp=False, score=True, queue=8, source=held)
    try:
        submit_all(qs, tickets)
        qs.step(2)
        before = eng.persistent_step_fallbacks
        monkeypatch.setenv("FC_LAURA_PERSIST_TEST", "timeout")
        with pytest.warns(RuntimeWarning, match="timed out at a hand-off"):
            st = qs.step(2)
        monkeypatch.delenv("FC_LAURA_PERSIST_TEST")
        assert st == {} and eng.persistent_step_fallbacks == before + 1
        assert sorted(qs.collect()) == [(0, None, 0, None), (1, None, 0, None)], "failed, never with tokens"
        got, _ = run_queue(qs, 3)                      # the waiting tickets, over the kernel chain
        assert sorted(got) == [2, 3, 4]
        assert not eng.set_persistent_step(False)
        chain = twin(eng, held, 2, tickets)            # the twin on the kernel chain: the form the session fell back to
        for i in (2, 3, 4):
            assert_same(got[i], chain[i], ("after the time-out", i))
    finally:
        assert eng.set_persistent_step(True)
        qs.free()
        held.free()
