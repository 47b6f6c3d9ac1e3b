"""Per-slot sampling rules of a decoding session on the GPU (DecodeSlots.start / start_from / fork / rewind(rules=SamplingRules(...)),
fc_laura_slots_set_rules): temperature, minimum length, top-k with top-p, the repeat rule.  Tiny synthetic checkpoints and the existing
goldens, sessions of S = 4 slots with max_positions 256 opened with logp=True, score=True.  What is pinned:

1. neutral rules are the session without rules, bit for bit;
2. temperature: greedy tokens unchanged, the score terms against float64 from the slot's own log-probability rows (the group softmax
   is shift-invariant, so the rows suffice), bar 2e-5 (nq x 1e-5 as test_laura_score_gpu.py) x max(1, 1 / T); T = 1/64 draws the
   arg-max.  Largest |term - float64| found on the MI355X (2026-10-19): T = 0.5 greedy 9.1e-7, top-k 25 1.6e-6 (bar
   4e-5); T = 2 greedy 1.8e-6, top-k 25 1.5e-6 (bar 2e-5);
3. minimum length on the <eos> golden;  4. top-k with top-p;  5. / 6. the repeat rule: its exact window boundary, the redraw's
   distribution;  7. rules travel with fork / rewind and a fork without rules has none;  8. refusals.
No tolerance anywhere but the float64 bars of 2 and 3 and the chi-square of 6 (the existing sampler test's: 8 ids + rest, 27.9)."""
import math

import numpy as np
import pytest
import torch

from helpers import golden

from test_laura import MAN
from test_laura_slots_gpu import B3, EOS, prompts

pytestmark = pytest.mark.gpu

S, CAP, STEPS = 4, 256, 12
BAR = 2e-5


def rules(**kw):
    from funcodec_amd.laura import SamplingRules
    return SamplingRules(**kw)


def all_on():
    return rules(temperature=0.75, min_length=5, top_p=0.9, repeat_window=8, repeat_count=2)


def open_session(eng):
    return eng.open_decode(S, max_positions=CAP, logp=True, score=True)


def until_done(s, slots, limit=64):
    for _ in range(limit):
        st = s.step(1)
        if all(st.get(i) != "running" for i in slots):
            break
    assert all(st.get(i) == "done" for i in slots), st


def finish(s, slot):
    """an ended slot's (generated tokens [n, nq] on the host, n, log-probability rows [max_length, V], score row [CAP], count, end)"""
    row, count, end = s.score_row(slot)
    tok, n, lp = s.take(slot, return_logp=True)
    return tok.cpu(), n, lp.cpu(), row, count, end


def run(eng, text, steps, sampling, seed, r="none", slot=1, session=None):
    """one prompt alone in `slot` to its end.  r: a SamplingRules, None, or "none": a session whose library never hears of rules"""
    s = session or open_session(eng)
    if isinstance(r, str):
        s._set_rules = lambda slot, rules: None
        s.start(slot, text, text.shape[0], steps, sampling=sampling, seed=seed)
    else:
        s.start(slot, text, text.shape[0], steps, sampling=sampling, seed=seed, rules=r)
    until_done(s, [slot])
    out = finish(s, slot)
    if session is None:
        s.free()
    return out


def equal(a, b):
    return a[1] == b[1] and a[4:] == b[4:] and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def terms64(logp, picks, spec, T=1.0, no_eos_below=0):
    """float64 score terms from log-probability rows [n, V] and picks [n, nq]: sum over the groups of log softmax(row_k / T)[pick_k],
    <eos> left out of the groups of rows < no_eos_below"""
    nq, G = spec.predict_nq, spec.codebook_size + 1
    lp = logp[: picks.shape[0]].double().reshape(-1, nq, G) / T
    lp[:no_eos_below, :, G - 1] = -math.inf
    ls = lp - torch.logsumexp(lp, dim=2, keepdim=True)
    return ls.gather(2, picks.long()[:, :, None])[:, :, 0].sum(1)


def many(eng, text, seeds, steps, sampling, r):
    """one generation per seed: a source slot holds the prompt, three slots at a time are started from it.  [(tokens, n)]"""
    s = open_session(eng)
    s.start(0, text, text.shape[0], 1, sampling=False)
    out = []
    for i in range(0, len(seeds), 3):
        part = list(enumerate(seeds[i: i + 3], 1))
        for slot, seed in part:
            s.start_from(slot, 0, steps, sampling=sampling, seed=seed, rules=r)
        until_done(s, [slot for slot, _ in part])
        for slot, _ in part:
            tok, n = s.take(slot)
            out.append((tok.cpu(), n))
    s.free()
    return out


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling,seed", [(False, 0), (True, 1234), (25, 7), (0.8, 9)])
def test_neutral_rules_are_no_rules(sampling, seed):
    eng, P, spec = prompts(B3)
    A = P[0]
    ref = run(eng, A, STEPS, sampling, seed, "none")
    assert ref[1] >= 1 and bool((ref[3][: ref[4]] != 0).all())
    assert equal(run(eng, A, STEPS, sampling, seed, rules()), ref), "rules=SamplingRules()"
    assert equal(run(eng, A, STEPS, sampling, seed, None), ref), "rules=None"
    # among slots that run under all rules, one of them started after the neutral slot
    s = open_session(eng)
    s.start(0, P[1], P[1].shape[0], 30, sampling=25, seed=5, rules=all_on())
    s.step(2)
    s.start(1, A, A.shape[0], STEPS, sampling=sampling, seed=seed, rules=rules())
    s.start(3, P[2], P[2].shape[0], 30, sampling=7, seed=11, rules=all_on())
    s.step(3)
    s.start(2, P[1], P[1].shape[0], 30, sampling=True, seed=3, rules=rules(temperature=2.0, min_length=20, repeat_window=256, repeat_count=1))
    until_done(s, [1])
    got = finish(s, 1)
    s.free()
    assert equal(got, ref), "a neutral slot among slots with all rules on"


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0.5, 2.0])
def test_temperature_scales_the_distribution_and_the_score(T):
    eng, P, spec = prompts(B3)
    A = P[0]
    ref = run(eng, A, STEPS, False, 0, None)
    for sampling, seed in ((False, 0), (25, 7)):
        got = run(eng, A, STEPS, sampling, seed, rules(temperature=T))
        n = got[1]
        if sampling is False:
            assert n == ref[1] and torch.equal(got[0], ref[0]), "a power of two scales exactly: the greedy tokens are those of T = 1"
            assert torch.equal(got[2], ref[2]), "the log-probability rows stay those of the raw logits"
        err = float((got[3][:n].double() - terms64(got[2], got[0], spec, T)).abs().max())
        print("T", T, "sampling", sampling, "steps", n, "max |term - float64|", err, "bar", BAR * max(1.0, 1.0 / T))
        assert err < BAR * max(1.0, 1.0 / T), (T, sampling, err)
        if T != 1.0:
            plain = float((got[3][:n].double() - terms64(got[2], got[0], spec)).abs().max())
            assert plain > 100 * BAR, "the terms are not those of T = 1"


def test_a_small_temperature_draws_the_arg_max():
    eng, P, spec = prompts(B3)
    G = spec.codebook_size + 1
    # the condition on the inputs: the golden's first step, group 0, has its top-1 0.38 above its top-2, so at T = 1/64 everything
    # but the arg-max has at most 1024 exp(-64 x 0.38) < 1e-7 of the mass
    row = torch.from_numpy(golden(B3)["logp_0"])[0].reshape(spec.predict_nq, G)[0].double()
    top = row.topk(2)[0]
    assert (G - 1) * math.exp(-64.0 * float(top[0] - top[1])) < 1e-7
    got = many(eng, P[0], list(range(500, 532)), 1, True, rules(temperature=1.0 / 64))
    first = [int(t[0, 0]) for t, n in got]
    assert len(first) == 32 and sum(1 for v in first if v == int(row.argmax())) >= 31, first
    plain = [int(t[0, 0]) for t, n in many(eng, P[0], list(range(500, 532)), 1, True, None)]
    assert len(set(plain)) > 16, "the same seeds at T = 1 spread over the group"


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_min_length_masks_eos_until_then():
    eng, Q, spec = prompts(EOS)
    nq, G, K = spec.predict_nq, spec.codebook_size + 1, spec.codebook_size
    g = golden(EOS)
    assert MAN["cases"][EOS]["tokens"] == [6, 8]
    want = {0: (6, [76, 444]), 1: (8, [176, 568])}
    for b in (0, 1):
        gold, (end_at, nxt) = torch.from_numpy(g[f"tokens_{b}"].astype(np.int64)), want[b]
        grow = torch.from_numpy(g[f"logp_{b}"])[end_at].reshape(nq, G)
        assert grow.argmax(1)[0] == K and grow[:, :K].argmax(1).tolist() == nxt, "the golden ends on <eos> in group 0"
        tok, n, lp, row, count, end = run(eng, Q[b], 16, False, 0, rules(min_length=12), slot=b)
        assert 12 <= n <= 16 and torch.equal(tok[:end_at], gold) and tok[end_at].tolist() == nxt, (b, n, tok)
        assert int(tok.max()) < K, "no <eos> among the tokens"
        rows = lp.reshape(-1, nq, G)
        for j in range(n):
            pick = rows[j, :, :K].argmax(1) if j < 12 else rows[j].argmax(1)
            assert torch.equal(tok[j], pick), (b, j)
        if end == 2:                                                            # ended on <eos> at step n >= 12: that row's arg-max
            assert n >= 12 and bool((rows[n].argmax(1) == K).any())
        else:
            assert n == 16
        m = min(n, 12)
        err = float((row[:m].double() - terms64(lp, tok[:m], spec, 1.0, 12)).abs().max())
        print("prompt", b, "tokens", n, "end", end, "max |term - float64| below step 12", err)
        assert err < BAR, (b, err)
        assert float((row[end_at].double() - terms64(lp, tok[: end_at + 1], spec)[end_at]).abs()) > 100 * BAR, "not the term with <eos> in the group"


def test_min_length_holds_when_sampling():
    eng, Q, spec = prompts(EOS)
    got = many(eng, Q[0], list(range(32)), 16, True, rules(min_length=12))
    assert len(got) == 32 and all(12 <= n <= 16 for t, n in got), [n for t, n in got]
    assert all(int(t.max()) < spec.codebook_size for t, n in got)
    # nearly greedy (T = 1/64): without the rule the golden's <eos> at step 6 ends the utterance, with it nothing ends before 12
    sharp = many(eng, Q[0], list(range(6)), 16, True, rules(temperature=1.0 / 64))
    assert any(n < 12 for t, n in sharp), [n for t, n in sharp]
    held = many(eng, Q[0], list(range(6)), 16, True, rules(temperature=1.0 / 64, min_length=12))
    assert all(12 <= n <= 16 for t, n in held), [n for t, n in held]


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_top_k_with_top_p():
    eng, P, spec = prompts(B3)
    G = spec.codebook_size + 1
    p0 = torch.from_numpy(golden(B3)["logp_0"])[0].reshape(spec.predict_nq, G)[0].softmax(0)
    sv, si = p0.sort(descending=True, stable=True)
    nucleus = set(si[: int((torch.cumsum(sv, 0) < 0.8).sum()) + 2].tolist())     # + one entry for a cumulative sum rounding across p
    for k in (25, 100):                                                          # the radix select and the sort path
        allowed = set(p0.topk(k)[1].tolist()) & nucleus
        assert len(allowed) > 1
        first = [int(t[0, 0]) for t, n in many(eng, P[0], list(range(60)), 1, k, rules(top_p=0.8))]
        assert all(v in allowed for v in first), (k, first)
        assert len(set(first)) > 1, (k, first)
    # a case where the nucleus cuts inside the top-k: at T = 1/4 the top 25 hold 0.69 of the mass and 0.5 of it lies in 5 entries
    p4 = (torch.from_numpy(golden(B3)["logp_0"])[0].reshape(spec.predict_nq, G)[0].double() * 4).softmax(0)
    sv, si = p4.sort(descending=True, stable=True)
    cut = int((torch.cumsum(sv, 0) < 0.5).sum()) + 2
    assert 2 < cut < 25, cut
    first = [int(t[0, 0]) for t, n in many(eng, P[0], list(range(60)), 1, 25, rules(temperature=0.25, top_p=0.5))]
    assert all(v in set(si[:cut].tolist()) for v in first) and len(set(first)) > 1, (cut, first)
    # the smallest nucleus is the arg-max, at every step
    greedy = run(eng, P[0], STEPS, False, 0, None)
    tiny = run(eng, P[0], STEPS, 25, 77, rules(top_p=1e-6))
    assert tiny[1] == greedy[1] and torch.equal(tiny[0], greedy[0])


# 5 ---------------------------------------------------------------------------------------------------------------------------
def repeats_of(tokens):
    return {k: {v: [j for j, x in enumerate(tokens[:, k].tolist()) if x == v] for v in set(tokens[:, k].tolist())
                if tokens[:, k].tolist().count(v) > 1} for k in range(tokens.shape[1])}


def check_pick_or_window(tok, lp, spec, W):
    """every pick is the arg-max of its row, or the arg-max stands in the last W generated tokens of the group"""
    nq, G = spec.predict_nq, spec.codebook_size + 1
    rows = lp.reshape(-1, nq, G)
    fired = []
    for j in range(tok.shape[0]):
        for k in range(nq):
            top = int(rows[j, k].argmax())
            if int(tok[j, k]) != top:
                assert top in tok[max(0, j - W): j, k].tolist(), (j, k, top)
                fired.append((j, k))
    return fired


def test_the_repeat_rule_at_its_window_boundary():
    eng, P, spec = prompts(B3)
    gold = torch.from_numpy(golden(B3)["tokens_1"].astype(np.int64))
    assert repeats_of(gold) == {0: {372: [4, 10]}, 1: {}}, "the golden's greedy path repeats id 372 of group 0 at steps 4 and 10, nothing else"
    B = P[1]
    five = run(eng, B, STEPS, 1, 3, rules(repeat_window=5))
    assert five[1] == 12 and torch.equal(five[0], gold), "step 4 is outside the window of step 10"
    assert check_pick_or_window(five[0], five[2], spec, 5) == []
    seen = set()
    for seed in (3, 4, 5):
        six = run(eng, B, STEPS, 1, seed, rules(repeat_window=6))
        assert six[1] == 12 and torch.equal(six[0][:10], gold[:10]) and int(six[0][10, 1]) == int(gold[10, 1]), seed
        fired = check_pick_or_window(six[0], six[2], spec, 6)
        assert all(j >= 10 for j, k in fired) and (10, 1) not in fired, fired
        seen.add(int(six[0][10, 0]))
        assert equal(run(eng, B, STEPS, 1, seed, rules(repeat_window=6)), six), "a second run"
        assert equal(run(eng, B, STEPS, 1, seed, rules(repeat_window=6), slot=3), six), "in another slot"
    # the rule fired at step 10 of group 0: the draw from the whole group depends on the seed (372 itself has 0.5 % of the mass)
    assert len(seen) > 1 and seen != {372}, seen


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_the_redraw_follows_the_whole_distribution():
    eng, P, spec = prompts(B3)
    nq, G = spec.predict_nq, spec.codebook_size + 1
    gold = torch.from_numpy(golden(B3)["tokens_1"].astype(np.int64))
    B, N = P[1], 400
    s = open_session(eng)
    s.start(0, B, B.shape[0], STEPS, sampling=False)
    until_done(s, [0])
    picks, other = [], []
    w6 = rules(repeat_window=6)
    for i in range(0, N, 3):
        part = list(enumerate(range(2000 + i, 2000 + min(i + 3, N)), 1))
        for slot, seed in part:
            s.fork(slot, 0, 10, 11, sampling=1, seed=seed, rules=w6)
        st = s.step(1)
        for slot, _ in part:
            assert st[slot] == "done"
            tok, n, lp = s.take(slot, return_logp=True)
            assert n == 11 and torch.equal(tok[:10].cpu(), gold[:10])
            picks.append(int(tok[10, 0])); other.append(int(tok[10, 1]))
    src = finish(s, 0)
    s.free()
    assert torch.equal(src[0], gold)
    assert set(other) == {int(gold[10, 1])}, "group 1 has no repeat: its top-1 draw stands"
    p = src[2][10].reshape(nq, G)[0].double().softmax(0)
    top8 = p.topk(8)[1]
    counts = np.zeros(9)
    for v in picks:
        hit = (top8 == v).nonzero()
        counts[int(hit[0]) if len(hit) else 8] += 1
    expect = np.concatenate([p[top8].numpy(), [1.0 - float(p[top8].sum())]]) * N
    chi2 = float(((counts - expect) ** 2 / np.maximum(expect, 1e-9)).sum())
    print("chi2", chi2, "distinct", len(set(picks)))
    assert chi2 < 27.9, (chi2, counts, expect)                # chi-square, 8 degrees of freedom, p = 0.0005
    assert len(set(picks)) > 16


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_rules_travel_with_branches():
    eng, P, spec = prompts(B3)
    A = P[0]
    on = rules(temperature=1.0 / 64, min_length=5, top_p=0.9, repeat_window=8, repeat_count=2)
    ref = run(eng, A, STEPS, 25, 21, on)
    n = ref[1]
    assert n == STEPS, "the tiny model does not end on <eos> at this temperature"
    s = open_session(eng)
    s.start(1, A, A.shape[0], STEPS, sampling=25, seed=21, rules=on)
    assert s.step(5)[1] == "running" and s.n_gen(1) == 6
    s.fork(0, 1, 6, sampling=25, seed=21, rules=on)
    s.fork(3, 1, 6, sampling=25, seed=21)                                       # rules=None: neutral from here on
    until_done(s, [0, 1, 3])
    a, b = finish(s, 0), finish(s, 1)
    assert equal(b, ref) and equal(a, ref), "the fork with the source's sampling, seed and rules ends as the source does"
    s.start(1, A, A.shape[0], STEPS, sampling=25, seed=21, rules=on)
    until_done(s, [1])
    s.rewind(1, 6, sampling=25, seed=21, rules=on)
    until_done(s, [1])
    assert equal(finish(s, 1), ref), "a rewind with the rules"
    free = finish(s, 3)
    s.free()
    assert free[1] == STEPS and torch.equal(free[0][:6], ref[0][:6]) and torch.equal(free[3][:6], ref[3][:6])
    # the source's temperature pins group 0 to its arg-max (test_a_small_temperature_draws_the_arg_max); the fork without rules draws
    # from the top 25 of a flat distribution, and its terms from the fork point on are those of T = 1, not of T = 1/64
    G = spec.codebook_size + 1
    rows = free[2].reshape(-1, spec.predict_nq, G)
    assert any(int(free[0][j, 0]) != int(rows[j, 0].argmax()) for j in range(6, STEPS)), free[0][6:]
    err = float((free[3][6:STEPS].double() - terms64(free[2], free[0], spec)[6:]).abs().max())
    assert err < BAR, err
    hot = float((ref[3][6:STEPS].double() - terms64(ref[2], ref[0], spec)[6:]).abs().max())
    assert hot > 100 * BAR, "while the source's terms are those of its temperature"


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from funcodec_amd import _lib
    from funcodec_amd.engine import EngineError
    eng, P, spec = prompts(B3)
    A = P[0]
    on = all_on()

    def session(disturb):
        s = open_session(eng)
        s.start(2, A, A.shape[0], STEPS, sampling=25, seed=8, rules=on)
        s.step(3)
        if disturb:
            h, call = s._handle(), s.lib.fc_laura_slots_set_rules
            bad = [(4, 1.0, 0, 0.0, 0, 1, "slot 4 outside"), (-1, 1.0, 0, 0.0, 0, 1, "slot -1 outside"),
                   (2, 0.0, 0, 0.0, 0, 1, "slot 2.*temperature"), (2, -1.0, 0, 0.0, 0, 1, "slot 2.*temperature"),
                   (2, math.inf, 0, 0.0, 0, 1, "slot 2.*temperature"), (2, math.nan, 0, 0.0, 0, 1, "slot 2.*temperature"),
                   (2, 1.0, -1, 0.0, 0, 1, "slot 2.*min_length"), (2, 1.0, 0, -0.1, 0, 1, "slot 2.*top_p"),
                   (2, 1.0, 0, 1.5, 0, 1, "slot 2.*top_p"), (2, 1.0, 0, math.nan, 0, 1, "slot 2.*top_p"),
                   (2, 1.0, 0, 0.0, -1, 1, "slot 2.*repeat_window"), (2, 1.0, 0, 0.0, 257, 1, "slot 2.*repeat_window"),
                   (2, 1.0, 0, 0.0, 4, 0, "slot 2.*repeat_count"), (2, 1.0, 0, 0.0, 4, 5, "slot 2.*repeat_count")]
            import re
            for slot, t, n, p, w, r, msg in bad:
                assert call(h, slot, t, n, p, w, r) != 0, (slot, t, n, p, w, r)
                assert re.search(msg, _lib.last_error()), (msg, _lib.last_error())
            with pytest.raises(EngineError, match=r"slot 2.*top_p"):
                s.start(2, A, A.shape[0], STEPS, sampling=0.8, seed=1, rules=rules(top_p=0.5))
            with pytest.raises(EngineError, match=r"slot 2.*top_p"):
                s.start(2, A, A.shape[0], STEPS, sampling=True, seed=1, rules=rules(top_p=0.5))
            with pytest.raises(EngineError, match=r"slot 2.*repeat"):
                s.start(2, A, A.shape[0], STEPS, sampling=False, seed=1, rules=rules(repeat_window=4))
            with pytest.raises(EngineError, match=r"slot 2.*repeat"):
                s.rewind(2, 2, sampling=False, rules=rules(repeat_window=4))
            with pytest.raises(EngineError, match=r"slot 1.*top_p"):
                s.start_from(1, 2, STEPS, sampling=0.8, rules=rules(top_p=0.5))
            with pytest.raises(ValueError, match="SamplingRules"):
                s.start(2, A, A.shape[0], STEPS, rules=(0.5, 0))
        until_done(s, [2])
        out = finish(s, 2)
        s.free()
        return out

    assert equal(session(True), session(False)), "a refused call leaves the running slot as it was"
