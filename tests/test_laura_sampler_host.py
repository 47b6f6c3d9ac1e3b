"""The LauraTTS device sampler (sample_kernel, csrc/laura_kernels.hip) per draw: a host Philox that reproduces the kernel's uniform number
bit for bit, a float64 restatement of one sampled row (`sample_ref`), the input recipes tests/test_laura_sampler_gpu.py runs through
LauraEngine.sample, and -- here, without a GPU or the library -- the proof that the recipes decide their draws and can tell a wrong
sampler from a right one.

The draw is deterministic: u = (x0 >> 8) * 2^-24 with x0 the first word of Philox4x32-10 of counter (step, rng_row, word, 0x5eed) keyed by
the seed.  So a draw has ONE right id, except where u * total lies within rounding of a boundary of the candidates' cumulative sums; the
reference returns the SET of ids a correctly rounded fp32 sampler can return there, and the recipes keep such draws rare (caps below).

DELTA, the relative width of that band, is counted from draw_inverse_cdf, not measured on the kernel.  Every fp32 addition of positive
terms errs by at most 2^-24 of its result <= total.  Longest path from the candidates' probabilities to a prefix sum that `target` is
compared with: 4 additions inside a chunk (CH <= 5), 2 levels of the four-chunk combine, 6 steps of the shuffle scan, 1 for
below = incl - mine, 3 for the walk over the lane's chunks, 4 for the walk inside a chunk: 20.  The total itself takes 12 of these again
(chunk, combine, scan) before target = u * total rounds once: 13.  Each probability is expf(x - m): 1 ulp = 2 x 2^-24 for expf (the HIP
math API's stated bound), and x - m, exact on the 2^-6 grid at T = 1, rounds by half an ulp of a number below 16 once a temperature took
x off the grid: 2^-21 absolute in the exponent = 8 x 2^-24 relative; both enter the prefix and the total: 20.  Sum 53, taken linearly.
DELTA = 64 x 2^-24 = 3.8e-6.  The thread-0 walks of the nucleus / top-p cut add one term per entry: n roundings, the same 10 per
probability, 24 for the group total they are compared with (4 in-thread additions, 6 wave-sum steps, 3 for the four waves, 10 per
probability, 1 for p x total): n + 35; DELTA_N(n) = (n + 48) x 2^-24.  The bands hold for logits within 16 of the group's maximum; the
recipes put every other logit at least 40 below it (mass below DELTA / 100 of the total, asserted) or 120 below it (probability exactly 0
in fp32).  An id whose fp32 probability is 0 is never accepted.

Caps (conditions on the recipes, checked from the reference alone): at most 2 % of each mode's random draws have more than one accepted
id; every planted case has exactly one.

Power: ten deliberately wrong samplers (WRONG) each leave the accepted set on at least 5 % of the random decided draws of the mode they
touch and on the planted case aimed at them.  One exception, by arithmetic and not by choice: a strict `<` in the walk differs from `<=`
only where u * total EQUALS a prefix sum, which a random draw never does; it is held to its planted cases alone (u = 0 in front of
zero-probability ids), and its share on random draws is printed, not asserted.  One variant is restated: "a temperature applied after
the arg-max" changes nothing for T > 0 taken literally (the arg-max and the order of the candidates do not depend on T), so
`temperature_after_cut` takes the candidate cut (the nucleus / top-p count) from the untempered distribution and draws from the tempered
one, the observable form of the same mistake.  `row_word_batch` (the table form's Philox row word taken from the batch row) has its
planted row too, "row word 23 softmax"; on the GPU the rows are packed at batch rows that differ from their rng_row.
"""
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from laura_oracle import LauraOracle

K = 1024
G = K + 1
EOS = K
DELTA = 64.0 * 2.0 ** -24
NEAR, FAR, ZERO = 16.0, 40.0, 120.0     # mass-carrying logits lie within NEAR of the maximum, the others FAR (or ZERO: fp32 probability 0) below
GRID = 64.0                              # logits are multiples of 2^-6
SHARPNESS = (0.5, 2.0, 5.0)
R_ROWS = 272                             # token rows of a packed launch: a 256-token window and room behind it
WRONG = ("strict_walk", "index_order_topk", "k_off_by_one", "nucleus_drops_crossing", "top_p_whole_group", "redraw_word_k",
         "redraw_truncated", "row_word_batch", "eos_last_candidate", "temperature_after_cut")


def delta_n(n):
    return (n + 48.0) * 2.0 ** -24


# ---- Philox4x32-10 ----------------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(ctr, key):
    """Philox4x32-10 (Random123): ctr 4 and key 2 arrays (or scalars) of 32-bit words, broadcast against each other -> 4 uint64 arrays"""
    x = [np.asarray(c, dtype=np.uint64) & _M32 for c in ctr]
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x[0], np.uint64(0xCD9E8D57) * x[2]
        x = [(p1 >> np.uint64(32)) ^ x[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ x[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return x


def philox_uniform(seed, step, rng_row, word):
    """the kernel's philox_uniform: float32 u in [0, 1), a multiple of 2^-24; arguments broadcast"""
    seed = np.asarray(seed, dtype=np.uint64)
    x0 = philox4x32((step, rng_row, word, 0x5EED), (seed & _M32, seed >> np.uint64(32)))[0]
    return (x0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


# found once by a search over the seeds 0 .. 2^26 at counter (0, 0, 0); test_extreme_seeds re-derives u from them
SEED_U_ZERO = 31370842
SEED_U_TOP = 2974210


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def neutral(**kw):
    """the parameters of one sampled row; the defaults are a call without rules"""
    p = dict(mode=0, k=0, p=0.0, temperature=1.0, min_length=0, top_p=0.0, repeat_window=0, repeat_count=1)
    p.update(kw)
    return p


def tempered(x32, prm, gen):
    """what every statement behind the rules sees: x / T in fp32, <eos> = -inf while gen < min_length"""
    y = np.asarray(x32, dtype=np.float32).copy()
    if np.float32(prm["temperature"]) != np.float32(1.0):
        y = (y / np.float32(prm["temperature"])).astype(np.float32)
    masked = gen < prm["min_length"]
    if masked:
        y[G - 1] = -np.inf
    return y, masked


def draw_set(e, order, n, u, exact=False):
    """ids a correctly rounded inverse-CDF draw over candidates order[:n] with probabilities e can return: those whose interval of the
    cumulative sums, widened by DELTA x total, holds u x total; never an id without fp32 mass"""
    pr = e[order[:n]]
    cum = np.cumsum(pr)
    tot = cum[-1]
    t = float(u) * tot
    d = DELTA * tot
    lo = np.concatenate(([0.0], cum[:-1]))
    live = pr > 0.0
    if exact:                            # the exact draw, no band: the first entry whose sum exceeds t, walked back to one with mass
        j = min(int(np.searchsorted(cum, t, side="right")), n - 1)
        while j > 0 and not live[j]:
            j -= 1
        return {int(order[j])}
    ok = live & (lo - d <= t) & (t <= cum + d)
    if not ok.any():                     # above the last sum by rounding alone
        ok[np.nonzero(live)[0][-1]] = True
    return {int(i) for i in order[:n][ok]}


def nucleus_counts(e, order, limit, thr_p, total):
    """candidate counts the thread-0 walk `while (n < limit && cum < p x total)` can end with, n >= 1"""
    cum, out = 0.0, set()
    for n in range(limit + 1):
        if n == limit:
            out.add(max(n, 1))
            break
        band = delta_n(n) * total
        if cum >= thr_p * total + band:
            out.add(max(n, 1))
            break
        if cum >= thr_p * total - band:
            out.add(max(n, 1))
        cum += e[order[n]]
    return out


def group_ref(x32, prm, gen, u, u2, window, wrong=None, exact=False):
    """One group of one row: x32 the group's G raw fp32 logits, u / u2 the first draw's and the redraw's uniform numbers, window the
    group's ids the repeat rule looks at.  -> (the set of ids the sampler may pick, y, m, total) with y the logits behind the rules, m
    their maximum, total = sum exp(y - m) in float64.  exact: no rounding bands (one id: what an exact sampler picks).  wrong: one of
    WRONG."""
    y, masked = tempered(x32, prm, gen)
    m = float(y.max())
    first = int(np.argmax(y))            # numpy returns the first index of the maximum
    y64 = y.astype(np.float64)
    e = np.exp(y64 - m)
    e[np.exp(y64 - m) < 2.0 ** -150] = 0.0
    total = float(e.sum())
    mode = prm["mode"]
    if mode == 0:
        return {first}, y, m, total
    index_order = np.arange(G)
    desc = np.argsort(-y64, kind="stable")           # logit descending, index ascending
    e_cut = e
    if wrong == "temperature_after_cut":              # the candidate cut from the untempered distribution
        y0, _ = tempered(x32, dict(prm, temperature=1.0), gen)
        e_cut = np.exp(y0.astype(np.float64) - float(y0.max()))
        desc = np.argsort(-y0.astype(np.float64), kind="stable")
    tot_cut = float(e_cut.sum())
    order, counts = index_order, {G}
    if mode == 2:
        k = min(max(prm["k"], 1), G)
        if wrong == "k_off_by_one":
            k = max(k - 1, 1) if k > 1 else 2
        order, counts = desc, {k}
        if prm["top_p"] > 0.0:
            limit = G if wrong == "top_p_whole_group" else k
            counts = nucleus_counts(e_cut, desc, limit, float(np.float32(prm["top_p"])), tot_cut) if not exact else \
                {exact_count(e_cut, desc, limit, float(np.float32(prm["top_p"])), tot_cut)}
        if wrong == "index_order_topk":
            kk = max(counts)
            order = np.concatenate((np.sort(desc[:kk]), desc[kk:]))
    elif mode == 3:
        order = desc
        pf = float(np.float32(prm["p"]))
        counts = {exact_count(e_cut, desc, G, pf, tot_cut)} if exact else nucleus_counts(e_cut, desc, G, pf, tot_cut)
        if wrong == "nucleus_drops_crossing":
            counts = {max(n - 1, 1) for n in counts}
    if masked:
        if wrong == "eos_last_candidate":             # <eos> moved behind the candidates with the mass it had before the mask
            y_un, _ = tempered(x32, dict(prm, min_length=0), gen)
            e = e.copy()
            e[G - 1] = math.exp(float(y_un[G - 1]) - m)
            order = np.concatenate((order[order != G - 1], [G - 1]))
            counts = {n + 1 if mode != 1 else G for n in counts}
        else:
            counts = {min(n, G - 1) for n in counts}
    counts = {min(n, G) for n in counts}
    picks = set()
    for n in counts:
        picks |= draw_set(e, order, n, u, exact)
    if wrong == "strict_walk":
        picks = {strict_pick(e, order, max(counts), u)}
    W, cnt = prm["repeat_window"], prm["repeat_count"]
    if W > 0:
        final = set()
        for t in picks:
            if sum(1 for v in window if v == t) >= cnt:
                if wrong == "redraw_truncated":
                    for n in counts:
                        final |= draw_set(e, order, n, u2, exact)
                else:
                    final |= draw_set(e, index_order, G - 1 if masked else G, u if wrong == "redraw_word_k" else u2, exact)
            else:
                final.add(t)
        picks = final
    return picks, y, m, total


def exact_count(e, order, limit, thr_p, total):
    cum, n = 0.0, 0
    while n < limit and cum < thr_p * total:
        cum += e[order[n]]
        n += 1
    return max(n, 1)


def strict_pick(e, order, n, u):
    """the walk with `<` for `<=`: an entry is passed only while the sum stays BELOW the target"""
    pr = e[order[:n]]
    cum = np.cumsum(pr)
    j = min(int(np.searchsorted(cum, float(u) * cum[-1], side="left")), n - 1)
    return int(order[j])


def window_of(history, gen, W, k):
    """the group-k ids of generated tokens [max(0, gen - W), gen)"""
    return [int(history[j][k]) for j in range(max(0, gen - W), gen)] if W > 0 else []


def sample_ref(logits, prm, state, history, forced=None, wrong=None, exact=False, batch_row=None):
    """One row of a sampler launch.  logits [nq, G] fp32 as the device sees them; prm = neutral(...) plus seed, rng_row, max_steps,
    forced_on; state = dict(step, gen, done, pos); history [gen, nq] generated ids; forced [nq] or None.  batch_row: the call form,
    whose Philox row word is the batch row.  -> dict(accepted: per group the set of ids the sampler may pick BEFORE forcing,
    final: per group the set after forcing, y / m / total per group)"""
    nq = logits.shape[0]
    row_word = prm.get("rng_row", 0) if batch_row is None else batch_row
    if wrong == "row_word_batch":
        row_word = prm["_batch_row"]
    out = dict(accepted=[], final=[], y=[], m=[], total=[])
    for k in range(nq):
        u = philox_uniform(prm.get("seed", 0), state["step"], row_word, k)
        u2 = philox_uniform(prm.get("seed", 0), state["step"], row_word, 8 + k)
        picks, y, m, total = group_ref(logits[k], prm, state["gen"], u, u2, window_of(history, state["gen"], prm["repeat_window"], k),
                                       wrong, exact)
        out["accepted"].append(picks)
        use_forced = forced is not None and prm.get("forced_on", 1) and state["gen"] < prm["max_steps"]
        out["final"].append({int(forced[k])} if use_forced else picks)
        out["y"].append(y); out["m"].append(m); out["total"].append(total)
    return out


def score_ref(ref, picks):
    """the step's score term in float64 for the final picks: sum over the groups of (y[t] - m) - log(total)"""
    return sum((float(ref["y"][k][t]) - ref["m"][k]) - math.log(ref["total"][k]) for k, t in enumerate(picks))


def log_softmax_ref(logits):
    """float64 log-softmax of the raw logits over the whole vocabulary"""
    x = np.asarray(logits, dtype=np.float64).reshape(-1)
    s = x - x.max()
    return s - math.log(np.exp(s).sum())


def bookkeeping_ref(picks, prm, state, tok_off):
    """decode_codec's bookkeeping for the final picks: dict(step, gen, done, pos, ended (1 if the row ends in this launch), write: the
    token row written or None)"""
    active = not state["done"] and state["gen"] < prm["max_steps"]
    out = dict(step=state["step"] + 1, gen=state["gen"], done=int(bool(state["done"])), pos=state["pos"], ended=0, write=None)
    if not active:
        return out
    if EOS in picks:
        out.update(done=1, ended=1)
        return out
    out.update(gen=state["gen"] + 1, write=tok_off + state["gen"])
    if state["step"] > 0:
        out["pos"] = state["pos"] + 1
    if state["gen"] + 1 >= prm["max_steps"]:
        out.update(done=1, ended=1)
    return out


# ---- input recipes ------------------------------------------------------------------------------------------------------------------------
def grid(x):
    return (np.round(np.asarray(x, dtype=np.float64) * GRID) / GRID).astype(np.float32)


def random_group(rng, sd, eos="zero"):
    """G logits on the 2^-6 grid, normal with standard deviation sd, clipped to NEAR below their maximum; <eos> ZERO below it (never
    drawn: a drawn <eos> would hide the other group's pick) or, "high", 4 above it"""
    x = grid(rng.normal(0.0, sd, G))
    top = float(x[:K].max())
    x = np.maximum(x, np.float32(top - NEAR))
    x[EOS] = top - ZERO if eos == "zero" else top + 4.0
    return x.astype(np.float32)


def flat_group(rng, lo=0.0, eos="zero"):
    """every id carries mass: the draw-position cases search a seed for one chosen candidate"""
    x = grid(lo + rng.uniform(0.0, 1.0, G))
    x[EOS] = float(x[:K].max()) - ZERO if eos == "zero" else x[EOS]
    return x


def distinct_group(rng, eos="zero"):
    """all K token logits different (a permutation of a 2^-6 ladder 16 wide): no tie decides a cut"""
    x = np.empty(G, dtype=np.float32)
    x[:K] = (rng.permutation(K) / GRID).astype(np.float32)
    x[EOS] = 16.0 - ZERO if eos == "zero" else 17.0
    return x


def case(name, logits, prm, *, step=1, gen=0, done=0, pos=7, tok_off=0, history=None, forced=None, seed=0, rng_row=0, max_steps=None,
         forced_on=1, planted=True, aimed=None):
    """one row of a launch.  history [gen, nq] (default: ids 1 .. that the logits make improbable); max_steps default gen + 4"""
    logits = np.asarray(logits, dtype=np.float32).reshape(-1, G)
    nq = logits.shape[0]
    if history is None:
        history = np.full((gen, nq), 3, dtype=np.int64)
    history = np.asarray(history, dtype=np.int64).reshape(gen, nq)
    prm = dict(prm, seed=seed, rng_row=rng_row, max_steps=gen + 4 if max_steps is None else max_steps, forced_on=forced_on)
    return dict(name=name, logits=logits, nq=nq, prm=prm, state=dict(step=step, gen=gen, done=done, pos=pos), tok_off=tok_off,
                history=history, forced=None if forced is None else [int(v) for v in forced], planted=planted, aimed=aimed)


def ref_of(c, **kw):
    if kw:
        return sample_ref(c["logits"], c["prm"], c["state"], c["history"], c["forced"], **kw)
    if "_ref" not in c:
        c["_ref"] = sample_ref(c["logits"], c["prm"], c["state"], c["history"], c["forced"])
    return c["_ref"]


def decided(c):
    return all(len(s) == 1 for s in ref_of(c)["final"])


def off_the_set(c, w):
    """does the wrong sampler w pick, in group 0, an id the reference does not accept?"""
    c2 = dict(c, prm=dict(c["prm"], _batch_row=c["prm"]["rng_row"] + 17))
    c2.pop("_ref", None)
    return not (ref_of(c2, wrong=w, exact=(w != "strict_walk"))["final"][0] <= ref_of(c)["final"][0])


def seed_where(c, pred, tries=400):
    """the case with the first seed at which it is decided and pred holds"""
    for seed in range(tries):
        c2 = dict(c, prm=dict(c["prm"], seed=seed))
        c2.pop("_ref", None)
        if decided(c2) and pred(c2):
            return c2
    raise AssertionError("no seed found for " + c["name"])


def aimed_at(c, w):
    return dict(seed_where(c, lambda c2: off_the_set(c2, w)), aimed=w)


def exact_first(c):
    """every group's exact pick with the repeat rule off"""
    off = {k: v for k, v in c.items() if k != "_ref"}
    off["prm"] = dict(c["prm"], repeat_window=0)
    return [next(iter(p)) for p in ref_of(off, exact=True)["accepted"]]


def first_pick_is(t):
    return lambda c: exact_first(c)[0] == t


def find_seed(logits_k, prm, gen, want, *, step=1, rng_row=0, word=0, tries=1 << 15):
    """the first seed whose exact draw in this group is candidate position `want` of the candidate order, away from both boundaries by
    10 x DELTA.  -> (seed, the id)"""
    y, masked = tempered(logits_k, prm, gen)
    y64 = y.astype(np.float64)
    e = np.exp(y64 - y64.max())
    order = np.arange(G) if prm["mode"] == 1 else np.argsort(-y64, kind="stable")
    n = G if prm["mode"] == 1 else min(max(prm["k"], 1), G)
    n = min(n, G - 1) if masked else n
    cum = np.cumsum(e[order[:n]])
    lo, hi = (cum[want - 1] if want else 0.0), cum[want]
    gap = 10.0 * DELTA * cum[-1]
    assert hi - lo > 4.0 * gap, "the wanted candidate is too thin to be aimed at"
    seeds = np.arange(tries, dtype=np.uint64)
    t = philox_uniform(seeds, step, rng_row, word).astype(np.float64) * cum[-1]
    hit = np.nonzero((t > lo + gap) & (t < hi - gap))[0]
    assert hit.size, "no seed found"
    return int(hit[0]), int(order[want])


def with_nq(rng, nq, group0, other=None):
    """[nq, G]: the planted group first, an ordinary one behind it"""
    return np.stack([group0] + [random_group(rng, 2.0) if other is None else other for _ in range(nq - 1)])


def snapped(c):
    """a random nucleus / top-p row with its threshold moved to the middle of the entry that crosses it, and the further groups a
    permutation of group 0's logits (<eos> in place): the candidate count, which the groups share p for, is then decided in all of
    them, at every sharpness (in a flat group the walk's band, DELTA_N of hundreds of entries, is a tenth of an entry otherwise)"""
    prm = c["prm"]
    key = "p" if prm["mode"] == 3 else "top_p"
    if prm["mode"] not in (2, 3) or prm[key] <= 0.0:
        return c
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(c["name"].encode())))
    for k in range(1, c["nq"]):
        c["logits"][k, :K] = c["logits"][0, rng.permutation(K)]
        c["logits"][k, EOS] = c["logits"][0, EOS]
    y, _ = tempered(c["logits"][0], prm, c["state"]["gen"])
    y64 = y.astype(np.float64)
    e = np.exp(y64 - y64.max())
    cum = np.cumsum(np.sort(e)[::-1])
    n = exact_count(e, np.argsort(-y64, kind="stable"), G, float(np.float32(prm[key])), float(e.sum()))
    mid = ((cum[n - 2] if n > 1 else 0.0) + cum[n - 1]) / 2.0 / cum[-1]
    c["prm"] = dict(prm, **{key: float(np.float32(mid))})
    return c


@functools.lru_cache(maxsize=None)
def random_cases(nq):
    """the random (non-planted) rows: per mode and sharpness, with temperatures, masks, top-p and repeat windows that fire"""
    rng = np.random.Generator(np.random.PCG64(20261021 + nq))
    out = []
    modes = [("greedy", neutral(mode=0)), ("softmax", neutral(mode=1)), ("top25", neutral(mode=2, k=25)), ("top5", neutral(mode=2, k=5)),
             ("top100", neutral(mode=2, k=100)), ("nucleus0.8", neutral(mode=3, p=0.8)), ("nucleus0.5", neutral(mode=3, p=0.5)),
             ("top25p0.9", neutral(mode=2, k=25, top_p=0.9)), ("top25p0.3", neutral(mode=2, k=25, top_p=0.3))]
    i = 0
    for label, base in modes:
        for sd in SHARPNESS:
            for T in (1.0, 0.25, 0.75, 2.0):
                for rep in range(2):
                    i += 1
                    prm = dict(base, temperature=T)
                    lg = np.stack([random_group(rng, sd) for _ in range(nq)])
                    out.append(case(f"random {label} sd{sd} T{T} #{rep}", lg, prm, step=1 + i % 5, gen=i % 4, seed=1000 + i, rng_row=(i * 7) % 61,
                                    planted=False))
    # <eos> masked with mass behind the mask
    for label, base in modes[1:]:
        for sd in SHARPNESS:
            for rep in range(3):
                i += 1
                lg = np.stack([random_group(rng, sd, eos="high") for _ in range(nq)])
                out.append(case(f"random masked {label} sd{sd} #{rep}", lg, dict(base, min_length=6), step=2, gen=rep, seed=3000 + i,
                                rng_row=i % 64, planted=False))
    # the repeat rule fires: the window holds the exact pick of the first draw
    for label, base in modes[1:]:
        for sd in SHARPNESS:
            for W, cnt in ((1, 1), (8, 2), (256, 1)):
                i += 1
                lg = np.stack([random_group(rng, sd) for _ in range(nq)])
                gen = 5 if W < 256 else 260
                c = case(f"random repeat {label} sd{sd} W{W}", lg, dict(base, repeat_window=W, repeat_count=cnt), step=3, gen=gen, seed=5000 + i,
                         rng_row=i % 64, planted=False)
                c = snapped(c)
                c["history"][-cnt:] = exact_first(c)
                out.append(c)
    return [snapped(c) for c in out]


@functools.lru_cache(maxsize=None)
def planted_cases(nq):
    """every planted row of the issue's list, for models of nq groups; each is a decided draw (asserted below)"""
    rng = np.random.Generator(np.random.PCG64(77 + nq))
    out = []

    def add(name, g0, prm, **kw):
        out.append(case(name, with_nq(rng, nq, g0), prm, **kw))
        return out[-1]

    # position of the maximum, and ties: greedy and a draw that the maximum dominates
    for at in (0, 255, 256, 767, 768, 1023, EOS):
        x = random_group(rng, 2.0)
        x[at] = float(x.max()) + 60.0
        for label, prm in (("greedy", neutral(mode=0)), ("softmax", neutral(mode=1)), ("top25", neutral(mode=2, k=25)), ("nucleus", neutral(mode=3, p=0.8))):
            add(f"max at {at} {label}", x, prm, seed=at)
    for a, b in ((5, 40), (40, 700), (255, 256), (63, 64)):          # one wave / two waves / a thread seam / a lane-to-wave seam
        x = random_group(rng, 2.0)
        x[a] = x[b] = float(x.max()) + 2.0
        add(f"max tied {a} {b}", x, neutral(mode=0))
        add(f"max tied {a} {b} top1", x, neutral(mode=2, k=1))
    # signs and zeros
    x = random_group(rng, 2.0) - np.float32(40.0)
    add("all negative softmax", x, neutral(mode=1), seed=1)
    # the Philox row word is the row's own (rng_row 23), not the batch row it is packed at
    out.append(aimed_at(add("row word 23 softmax", random_group(rng, 2.0), neutral(mode=1), rng_row=23), "row_word_batch"))
    del out[-2]
    add("all negative top25", x, neutral(mode=2, k=25), seed=2)
    add("mixed signs nucleus", random_group(rng, 5.0), neutral(mode=3, p=0.8), seed=3)
    for k_cut, ids, vals in ((1, (3, 7), (-0.0, 0.0)), (1, (3, 7), (0.0, -0.0)), (2, (700, 20, 300), (0.0, -0.0, 0.0)), (2, (10, 600, 900), (-0.0, -0.0, 0.0))):
        x = -np.abs(random_group(rng, 2.0)) - np.float32(1.0)       # everything else below zero
        x[EOS] = -ZERO
        for i_, v in zip(ids, vals):
            x[i_] = v
        sgn = "".join("-" if math.copysign(1.0, v) < 0 else "+" for v in vals)
        # the expected pick set is the k lowest indices among the zeros (probability descending, index ascending); the seed aims at the last of them
        seed, want = find_seed(x, neutral(mode=2, k=k_cut), 0, k_cut - 1)
        c = add(f"signed zeros k{k_cut} ids{ids} {sgn}", x, neutral(mode=2, k=k_cut), seed=seed, aimed="signed_zero")
        assert want == sorted(ids)[k_cut - 1]
        c["expect"] = want
    # ties around the k-th key: exactly k, k - 1, k + 2 entries at or above it, the seed aimed at the LAST candidate (the cut between tied entries)
    for k in (1, 2, 5, 25, 64):
        for n_at in (k, k - 1, k + 2):
            if n_at < 1:
                continue
            x = random_group(rng, 0.5)
            top = float(x[:K].max())
            ids = rng.choice(K, size=n_at + 3, replace=False)
            x[ids[:n_at]] = top + 1.0                                   # n_at entries at the k-th key ...
            x[ids[n_at:]] = top + 0.5                                   # ... and three tied just below it
            seed, want = find_seed(x, neutral(mode=2, k=k), 0, k - 1)
            add(f"ties k{k} with {n_at} at the key", x, neutral(mode=2, k=k), seed=seed, aimed="k_off_by_one" if n_at == k and k > 1 else None)
    # large top-k: the sort path, k >= G; more than 256 tied at the k-th key over a non-constant rest
    for k in (65, 100, 1025, 2000):
        x = flat_group(rng)
        seed, _ = find_seed(x, neutral(mode=2, k=k), 0, min(k, G) - 2)
        add(f"top{k} last-but-one candidate", x, neutral(mode=2, k=k), seed=seed)
    x = random_group(rng, 0.5)
    ids = rng.choice(K, size=300, replace=False)
    x[ids] = float(x[:K].max()) + 1.0
    for k in (25, 64, 100):
        seed, _ = find_seed(x, neutral(mode=2, k=k), 0, k - 1)
        add(f"300 tied at the key top{k}", x, neutral(mode=2, k=k), seed=seed)
    for k in (5, 25):                    # the candidates' order: descending, not by index
        out.append(aimed_at(add(f"top{k} of distinct logits", distinct_group(rng), neutral(mode=2, k=k)), "index_order_topk"))
        del out[-2]
    # nucleus
    for p in (0.05, 0.5, 0.8, 0.999, 1.0):
        for sd in (0.5, 5.0):
            add(f"nucleus {p} sd{sd}", random_group(rng, sd), neutral(mode=3, p=p), seed=int(p * 1000) + int(sd))
    x = random_group(rng, 0.5)
    x[321] = float(x[:K].max()) + 8.0
    add("nucleus of one entry", x, neutral(mode=3, p=0.5), seed=9)
    # the mass reaches p exactly at an entry in float64: 1, 1/2, 1/4, 1/4 of the total with every other id without mass, p = 0.75
    x = np.full(G, -ZERO, dtype=np.float32)
    x[[100, 200, 300, 400]] = [0.0, -1.0, -2.0, -2.0]
    # exp is not dyadic on logits; the probabilities are made so by the reference itself: p is taken from the float64 sums
    e = np.exp(x.astype(np.float64))
    p_exact = float(np.float32((e[100] + e[200]) / e.sum()))
    c = add("nucleus near an entry's sum", x, neutral(mode=3, p=p_exact))
    assert nucleus_counts_of(c) == {2, 3}
    out[-1] = seed_where(c, lambda c2: True)
    out.append(aimed_at(add("nucleus, the crossing entry drawn", x, neutral(mode=3, p=0.7)), "nucleus_drops_crossing"))
    del out[-2]
    # top-k with top-p
    for tp in (0.3, 0.9, 1.0):
        for sd in (0.5, 2.0):
            add(f"top25 top_p {tp} sd{sd}", random_group(rng, sd), neutral(mode=2, k=25, top_p=tp), seed=int(tp * 10))
            if (tp, sd) == (0.9, 0.5):
                out[-1] = aimed_at(out[-1], "top_p_whole_group")
    # draw position: first / last candidate, the seams of chunks and lanes
    x = flat_group(rng)
    for ncand in (1, 2, 5, 25, 64, 100, 255, 256, 257, 512, 513, 1024, 1025):
        CH = (ncand + 255) // 256
        spots = sorted({0, ncand - 1} | {s for s in (CH - 1, CH, 4 * CH - 1, 4 * CH, 255 * CH - 1, 255 * CH) if 0 <= s < ncand})
        prm = neutral(mode=1) if ncand == G else neutral(mode=2, k=ncand)
        xx = x.copy()
        if ncand == G:
            xx[EOS] = 0.5                                               # the 1025th candidate carries mass
        for spot in spots:
            seed, want = find_seed(xx, prm, 0, spot)
            if want == EOS and nq > 1:
                continue                                                 # a drawn <eos> is one case of its own below
            add(f"ncand {ncand} spot {spot}", xx, prm, seed=seed)
    # extreme u against ids without mass at both ends, and against a masked <eos>
    x = flat_group(rng)
    x[[0, 1, 2, 3, 1020, 1021, 1022, 1023, EOS]] = float(x.max()) - ZERO
    for label, seed in (("u zero", SEED_U_ZERO), ("u top", SEED_U_TOP)):
        add(f"{label} softmax, ids without mass at both ends", x, neutral(mode=1), seed=seed, step=0, rng_row=0, aimed="strict_walk" if label == "u zero" else "zero_top")
        add(f"{label} nucleus 1.0", x, neutral(mode=3, p=1.0), seed=seed, step=0, rng_row=0)
        xm = flat_group(rng)
        xm[EOS] = float(xm.max()) + 3.0
        add(f"{label} masked <eos>", xm, neutral(mode=1, min_length=2), seed=seed, step=0, rng_row=0)
        add(f"{label} masked <eos> top2000", xm, neutral(mode=2, k=2000, min_length=2), seed=seed, step=0, rng_row=0)
    # u at the top where the ids without mass share a chunk (a lane) with the last ids that have some: there the walk's own sums, rounded
    # in another order than the scan's, can pass the last entry with mass
    for i in range(16):
        xz = flat_group(rng)
        xz[1016 + i % 4:] = float(xz[:K].max()) - ZERO
        add(f"u top softmax, mass ends inside the last chunk #{i}", xz, neutral(mode=1), seed=SEED_U_TOP, step=0, rng_row=0, aimed="zero_top")
    for i in range(16):
        xz = flat_group(rng)
        keep = rng.choice(K, size=97 + i % 3, replace=False)
        zero = np.ones(G, dtype=bool)
        zero[keep] = False
        xz[zero] = float(xz[keep].max()) - ZERO
        add(f"u top top100, {keep.size} ids with mass #{i}", xz, neutral(mode=2, k=100), seed=SEED_U_TOP, step=0, rng_row=0, aimed="zero_top")
    # temperature with each mode
    for T in (0.25, 0.75, 1.0, 2.0):
        for label, prm in (("greedy", neutral(mode=0)), ("softmax", neutral(mode=1)), ("top25", neutral(mode=2, k=25)), ("nucleus", neutral(mode=3, p=0.8))):
            add(f"T {T} {label}", random_group(rng, 2.0), dict(prm, temperature=T), seed=int(T * 100))
            if (T, label) == (0.25, "nucleus"):
                out[-1] = aimed_at(out[-1], "temperature_after_cut")
    # masking: gen = min_length - 1 and = min_length, <eos> the arg-max
    xm = random_group(rng, 2.0)
    xm[EOS] = float(xm.max()) + 60.0
    for gen in (2, 3):
        for label, prm in (("greedy", neutral(mode=0)), ("softmax", neutral(mode=1)), ("top25", neutral(mode=2, k=25)), ("nucleus", neutral(mode=3, p=0.8))):
            add(f"min_length 3 gen {gen} {label}", xm, dict(prm, min_length=3), gen=gen, seed=gen)
            if (gen, label) == (2, "softmax"):
                out[-1] = aimed_at(out[-1], "eos_last_candidate")
    # the repeat rule
    xr = random_group(rng, 0.5)
    xr[500] = float(xr[:K].max()) + 8.0                                  # the first draw is 500 at the seeds chosen below
    for W in (1, 8, 256):
        for cnt in sorted({1, 2, W} & set(range(1, W + 1))):
            gen = W + 3
            for where, fires in (("inside", True), ("outside", False)):
                h = np.full((gen, nq), 3, dtype=np.int64)
                h[gen - W - (0 if fires else 1): gen - W - (0 if fires else 1) + cnt, 0] = 500      # cnt hits from the window's far edge / one token further
                c = add(f"repeat W{W} count{cnt} {where}", xr, neutral(mode=1, repeat_window=W, repeat_count=cnt), gen=gen, history=h)
                out[-1] = aimed_at(c, "redraw_word_k") if (W, cnt, fires) == (8, 2, True) else seed_where(c, first_pick_is(500))
    h = np.full((2, nq), 500, dtype=np.int64)
    out.append(aimed_at(add("repeat gen below the window", xr, neutral(mode=2, k=25, repeat_window=8, repeat_count=2), gen=2, history=h), "redraw_truncated"))
    del out[-2]
    c = add("repeat gen below the window, one short", xr, neutral(mode=1, repeat_window=8, repeat_count=3), gen=2, history=h)
    out[-1] = seed_where(c, first_pick_is(500))
    xs_ = np.full(G, -ZERO, dtype=np.float32) + np.float32(20.0)
    xs_[500] = 20.0                                                      # the redraw can only return 500 again: allowed
    add("repeat redraws the same id", xs_, neutral(mode=1, repeat_window=1, repeat_count=1), gen=1, history=np.full((1, nq), 500), seed=5)
    if nq == 2:                                                          # the rule fires in group 1 only
        lg = np.stack([xr, xr])
        h = np.full((4, 2), 3, dtype=np.int64)
        h[:, 1] = 500
        c = case("repeat fires in group 1 only", lg, neutral(mode=1, repeat_window=4, repeat_count=4), gen=4, history=h)
        out.append(seed_where(c, lambda c2: exact_first(c2) == [500, 500]))
    # forced tokens
    xf = random_group(rng, 2.0)
    for label, prm in (("greedy", neutral(mode=0)), ("top25", neutral(mode=2, k=25))):
        add(f"forced on {label}", xf, prm, forced=[11 + k for k in range(nq)], seed=7)
        add(f"forced off for the row {label}", xf, prm, forced=[11 + k for k in range(nq)], forced_on=0, seed=7)
        add(f"forced <eos> {label}", xf, prm, forced=[EOS] + [12] * (nq - 1), seed=7)
        add(f"forced at the last step {label}", xf, prm, forced=[21] * nq, gen=3, max_steps=4, seed=7)
        add(f"forced <eos> below the minimum length {label}", xf, dict(prm, min_length=5), forced=[EOS] * nq, gen=1, seed=7)
    # bookkeeping
    xb = random_group(rng, 2.0)
    xe = xb.copy()
    xe[EOS] = float(xe.max()) + 60.0
    for label, prm in (("greedy", neutral(mode=0)), ("softmax", neutral(mode=1))):
        add(f"done row {label}", xb, prm, done=1, gen=2, seed=8)
        add(f"gen at max_steps {label}", xb, prm, gen=4, max_steps=4, seed=8)
        add(f"step 0 {label}", xb, prm, step=0, gen=0, pos=9, seed=8)
        add(f"step 5 {label}", xb, prm, step=5, gen=2, pos=9, tok_off=6, seed=8)
        add(f"last step {label}", xb, prm, step=5, gen=3, max_steps=4, seed=8)
        add(f"<eos> ends the row {label}", xe, prm, step=2, gen=1, seed=8)
    return [settled(c, rng) for c in out]


def settled(c, rng):
    """a planted case is a decided draw: where the arbitrary part of it (the seed of a case that aims at no candidate, the ordinary
    groups behind the planted one) leaves a draw within the rounding band, that part is chosen again"""
    for _ in range(20):
        sets = ref_of(c)["final"]
        if all(len(s) == 1 for s in sets):
            return c
        c = {k: v for k, v in c.items() if k != "_ref"}
        if len(sets[0]) > 1:
            c["prm"] = dict(c["prm"], seed=c["prm"]["seed"] + 100000)
        else:
            c["logits"] = np.stack([c["logits"][0]] + [random_group(rng, 2.0) for _ in range(c["nq"] - 1)])
    raise AssertionError("undecided: " + c["name"])


def all_cases(nq):
    return random_cases(nq) + planted_cases(nq)


def mode_label(c):
    p = c["prm"]
    return {0: "greedy", 1: "softmax", 2: "top-k + top-p" if p["top_p"] > 0 else "top-k", 3: "nucleus"}[p["mode"]]


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's known answers for Philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in philox4x32(ctr, key)) == want


def test_uniform_mapping():
    seeds = np.arange(1 << 14, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    u = philox_uniform(seeds, 3, 5, 1)
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    scaled = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(scaled, np.round(scaled)), "multiples of 2^-24: exactly representable"
    x0 = philox4x32((3, 5, 1, 0x5EED), (seeds & _M32, seeds >> np.uint64(32)))[0]
    assert np.array_equal(scaled.astype(np.uint64), x0 >> np.uint64(8))
    assert 0.49 < float(u.mean()) < 0.51
    # the words of the counter are in their places: each changes u
    base = philox_uniform(7, 1, 2, 3)
    assert len({float(base), float(philox_uniform(8, 1, 2, 3)), float(philox_uniform(7, 2, 2, 3)), float(philox_uniform(7, 1, 3, 3)),
                float(philox_uniform(7, 1, 2, 4)), float(philox_uniform(7 + (1 << 32), 1, 2, 3))}) == 6


def test_extreme_seeds():
    assert float(philox_uniform(SEED_U_ZERO, 0, 0, 0)) == 0.0
    assert float(philox_uniform(SEED_U_TOP, 0, 0, 0)) == 1.0 - 2.0 ** -24


@pytest.mark.parametrize("nq", [1, 2])
def test_recipes_keep_their_promises(nq):
    """mass-carrying logits within NEAR of the maximum, on the grid; the rest FAR below with a total mass under DELTA / 100, or without
    fp32 mass at all"""
    for c in all_cases(nq):
        for k in range(nq):
            y, _ = tempered(c["logits"][k], c["prm"], c["state"]["gen"])
            assert np.array_equal(c["logits"][k] * GRID, np.round(c["logits"][k] * GRID)), c["name"]
            d = (float(y.max()) - y.astype(np.float64))[np.isfinite(y)]
            near, far = d <= NEAR / min(1.0, c["prm"]["temperature"]) * (1.0 + 1e-6), d >= FAR      # x / T rounds in fp32
            assert bool((near | far).all()), c["name"]
            mass = np.exp(-d[far & (d < 100.0)]).sum() / np.exp(-d).sum()
            assert mass < DELTA / 100.0, (c["name"], mass)
            assert not bool(((d > 87.0) & (d < 110.0)).any()), c["name"]      # no denormal probabilities: zero or normal


@pytest.mark.parametrize("nq", [1, 2])
def test_caps(nq):
    """every planted case is decided; at most 2 % of each mode's random draws are not"""
    for c in planted_cases(nq):
        r = ref_of(c)
        assert all(len(s) == 1 for s in r["final"]), (c["name"], r["final"])
        if "expect" in c:
            assert r["final"][0] == {c["expect"]}, c["name"]
    tally = {}
    for c in random_cases(nq):
        t = tally.setdefault(mode_label(c), [0, 0])
        for s in ref_of(c)["accepted"]:
            t[0] += 1
            t[1] += len(s) > 1
    for label, (n, open_) in sorted(tally.items()):
        print(f"nq {nq} {label}: {open_} of {n} random draws undecided ({100.0 * open_ / n:.2f} %)")
        assert open_ <= 0.02 * n, label


def test_zero_probability_ids_are_never_accepted():
    for nq in (1, 2):
        for c in all_cases(nq):
            r = ref_of(c)
            for k in range(nq):
                for t in r["accepted"][k]:
                    assert r["y"][k][t] > r["m"][k] - 100.0, (c["name"], t)


MODES_OF_THE_ORACLE = {0: lambda p: False, 1: lambda p: True, 2: lambda p: int(p["k"]), 3: lambda p: float(np.float32(p["p"]))}


def test_reference_follows_the_reference_model():
    """on decided draws with the neutral rules, sample_ref is LauraOracle.sample_from (proven against LauraGenModel.sampling_ids'
    candidate construction in test_laura.py) for all four modes"""
    n = {0: 0, 1: 0, 2: 0, 3: 0}
    rng = np.random.Generator(np.random.PCG64(5))
    free_of_ties = [case(f"top{k} of distinct logits #{i}", distinct_group(rng), neutral(mode=2, k=k), seed=i, planted=False)
                    for i in range(4) for k in (1, 2, 5, 25, 64, 65, 100, 1025)]
    for c in all_cases(1) + free_of_ties:
        p = c["prm"]
        if (p["temperature"], p["min_length"], p["top_p"], p["repeat_window"]) != (1.0, 0, 0.0, 0) or (p["mode"] == 2 and p["k"] > G):
            continue
        ys = np.sort(c["logits"][0])[::-1]
        if p["mode"] == 2 and bool((ys[: min(p["k"], G - 1)] == ys[1: min(p["k"], G - 1) + 1]).any()):
            continue                     # torch.topk promises no order among tied entries; the documented one is pinned by the planted cases
        r = ref_of(c)
        if len(r["accepted"][0]) != 1:
            continue
        u = float(philox_uniform(p["seed"], c["state"]["step"], p["rng_row"], 0))
        got = LauraOracle.sample_from(torch.from_numpy(c["logits"][0]), MODES_OF_THE_ORACLE[p["mode"]](p), u)
        if p["mode"] == 3 and len(nucleus_counts_of(c)) > 1:
            continue
        assert {got} == r["accepted"][0], (c["name"], got, r["accepted"][0])
        n[p["mode"]] += 1
    print("draws compared with LauraOracle.sample_from per mode:", n)
    assert min(n.values()) >= 10


def nucleus_counts_of(c):
    y, _ = tempered(c["logits"][0], c["prm"], c["state"]["gen"])
    y64 = y.astype(np.float64)
    e = np.exp(y64 - y64.max())
    return nucleus_counts(e, np.argsort(-y64, kind="stable"), G, float(np.float32(c["prm"]["p"])), float(e.sum()))


def touches(w, c):
    """does the wrong variant change a statement this row runs?"""
    p = c["prm"]
    drawing = p["mode"] != 0
    return {"strict_walk": drawing, "index_order_topk": p["mode"] == 2 and p["k"] <= 100 and p["top_p"] == 0.0,
            "k_off_by_one": p["mode"] == 2 and p["k"] <= 25 and p["top_p"] == 0.0,
            "nucleus_drops_crossing": p["mode"] == 3, "top_p_whole_group": p["mode"] == 2 and p["top_p"] > 0.0,
            "redraw_word_k": drawing and p["repeat_window"] > 0, "redraw_truncated": p["mode"] in (2, 3) and p["repeat_window"] > 0,
            "row_word_batch": drawing, "eos_last_candidate": drawing and c["state"]["gen"] < p["min_length"],
            "temperature_after_cut": p["temperature"] != 1.0 and (p["mode"] == 3 or (p["mode"] == 2 and p["top_p"] > 0.0))}[w]


@pytest.mark.parametrize("w", WRONG)
def test_wrong_samplers_are_told_apart(w):
    """each wrong restatement leaves the accepted set on >= 5 % of the random decided draws of the mode it touches, and on its planted case"""
    n = off = 0
    for b, c in enumerate(random_cases(2)):
        if not touches(w, c):
            continue
        right = ref_of(c)
        c = {k_: v_ for k_, v_ in c.items() if k_ != "_ref"}
        c["prm"] = dict(c["prm"], _batch_row=(b % 64) if (b % 64) != c["prm"]["rng_row"] else (b + 1) % 64)
        wrong = ref_of(c, wrong=w, exact=(w != "strict_walk"))
        for k in range(2):
            if len(right["final"][k]) == 1:
                n += 1
                off += not (wrong["final"][k] <= right["final"][k])
    share = off / max(n, 1)
    print(f"{w}: off the accepted set on {off} of {n} random decided draws ({100.0 * share:.1f} %)")
    aimed = [c for nq in (1, 2) for c in planted_cases(nq) if c["aimed"] == w]
    for c in aimed:
        assert off_the_set(c, w), c["name"]
    if w == "strict_walk":
        assert aimed, "the strict walk is held to its planted cases (see the module docstring)"
        return
    assert n >= 30 and share >= 0.05, (w, n, share)
    assert aimed, w
