"""Time ``DecodeSlots.start_many`` (n different prompts per prefix pass), ``start_from(source=held)`` (a slot started by a copy from a
row of a holding session) and ``prefill`` (prefix passes run ahead of need into a holding session) on the synthetic checkpoints of the
``laura`` and ``lauramusic`` recipes.  The method of ``tools/laura_start_from.py``: 15 of 16 slots of the main session running, warm-up,
then 24 synchronised repetitions with the forms alternating; median and min .. max.  No pass / fail bar: what is found is reported.

(a) ``start_many`` of n = 1 / 2 / 4 / 8 / 16 prompts into a holding session of 16 rows against n x ``start`` into the same rows
    (texts of 16 .. 26 tokens, the prompts of ``tools/laura_slots_step.py``).
(b) ``start_from(source=held)`` against ``start_from`` inside the session and against ``start``, into the 16th slot.
(c) The 64-request workload of ``tools/laura_slots_step.py`` (lengths 50 .. 750 shuffled, forced tokens, then a forced <eos>) through 16
    slots kept full with prefill 0 / 4 / 16: the same lengths first, then steps, prefix passes and milliseconds (best of 2 each).

    python tools/laura_start_many.py [--out profiles/laura_start_many.txt]
"""
import argparse
import datetime
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from funcodec_amd.laura import HeldPrompts, LauraGenMI355X, drive_slots             # noqa: E402
from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config   # noqa: E402
from funcodec_amd.synth import make_laura_state_dict, synthetic_text                # noqa: E402

REPS, S = 24, 16


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(v):
    v = sorted(v)
    return f"median {statistics.median(v) * 1e6:9.1f} us (min {v[0] * 1e6:.1f}, max {v[-1] * 1e6:.1f})"


def crowd(m, cfg, spec):
    """A session of 16 slots with 15 running (forced tokens: nobody ends), 32 steps in; 16 prompts, their lengths, the forced tokens."""
    lens = [16 + (5 * i) % 11 for i in range(S)]
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, S, lens, 11)), torch.tensor(lens))
    rng = np.random.Generator(np.random.PCG64(9))
    forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(S, 750, spec.predict_nq)).astype(np.int64)).cuda()
    sess = m.engine.open_decode(S, max_positions=1024, logp=False)
    for b in range(S - 1):
        sess.start(b, outs[b], lens[b], 750, sampling=False, forced=forced[b])
    sess.step(32)
    return sess, outs, lens, forced


def part_a(m, cfg, spec, say):
    sess, outs, lens, _ = crowd(m, cfg, spec)
    held = m.engine.open_decode(S, max_positions=1024, logp=False)
    say(f"  (a) n prompts (text of {min(lens)} .. {max(lens)} tokens) into a holding session of 16 rows, 15 slots of the main session "
        f"running, {REPS} repetitions, forms alternating")
    for n in (1, 2, 4, 8, 16):
        reqs = {b: dict(text_outs=outs[b], text_len=lens[b], max_length=1, sampling=False) for b in range(n)}

        def one_by_one():
            for b in range(n):
                held.start(b, outs[b], lens[b], 1, sampling=False)
        a, b_ = [], []
        for r in range(REPS + 2):                              # the first two rounds are warm-up
            ta = timed(one_by_one)
            sess.step(4)
            tb = timed(lambda: held.start_many(reqs))
            sess.step(4)
            if r >= 2:
                a.append(ta)
                b_.append(tb)
        say(f"      n = {n:2d}   {n:2d} x start {spread(a)}   start_many {spread(b_)}   ratio {statistics.median(b_) / statistics.median(a):.3f}")
    held.free()
    sess.free()


def part_b(m, cfg, spec, say):
    sess, outs, lens, forced = crowd(m, cfg, spec)
    held = m.engine.open_decode(S, max_positions=1024, logp=False)
    held.start_many({b: dict(text_outs=outs[b], text_len=lens[b], max_length=1, sampling=False) for b in range(S)})
    a, b_, c = [], [], []
    for r in range(REPS + 2):
        j = r % (S - 1)                                        # the prompt of running slot j = held row j
        ta = timed(lambda: sess.start(S - 1, outs[j], lens[j], 750, sampling=False, forced=forced[j]))
        sess.step(4)
        tb = timed(lambda: sess.start_from(S - 1, j, 750, sampling=False, forced=forced[j]))
        sess.step(4)
        tc = timed(lambda: sess.start_from(S - 1, j, 750, sampling=False, forced=forced[j], source=held))
        sess.step(4)
        if r >= 2:
            a.append(ta)
            b_.append(tb)
            c.append(tc)
    held.free()
    sess.free()
    say(f"  (b) the 16th slot while 15 run, {REPS} repetitions, forms alternating")
    say(f"      start                        {spread(a)}")
    say(f"      start_from, same session     {spread(b_)}")
    say(f"      start_from, source = held    {spread(c)}")


def part_c(m, cfg, spec, say):
    N = 64
    K, nq = spec.codebook_size, spec.predict_nq
    lengths = [50 + (700 * i) // (N - 1) for i in range(N)]
    np.random.Generator(np.random.PCG64(0)).shuffle(lengths)
    lens = [16 + (5 * i) % 11 for i in range(N)]
    rng = np.random.Generator(np.random.PCG64(9))
    forced = rng.integers(0, K, size=(N, 750, nq)).astype(np.int64)
    for i, n in enumerate(lengths):
        if n < 750:
            forced[i, n:] = K                              # a forced <eos>: the row ends after n tokens
    forced = torch.from_numpy(forced).cuda()
    outs = []
    with torch.no_grad():
        for g in range(0, N, S):
            o, _ = m.encode(torch.from_numpy(synthetic_text(cfg, S, lens[g: g + S], 11 + g)), torch.tensor(lens[g: g + S]))
            outs += [o[b, : lens[g + b]] for b in range(S)]
    info = {}

    def session(P):
        sess = m.engine.open_decode(S, max_positions=1024, logp=False)
        held = m.engine.open_decode(P, max_positions=1024, logp=False) if P else None
        plan = HeldPrompts(P, N, 1) if P else None
        real_step, steps = sess.step, [0]

        def counting(n=1):
            steps[0] += n
            return real_step(n)
        sess.step = counting

        def start(slot, i):
            if not P:
                return sess.start(slot, outs[i], lens[i], 750, sampling=False, forced=forced[i])
            todo = plan.need(i)
            if todo:
                held.start_many({row: dict(text_outs=outs[q], text_len=lens[q], max_length=1, sampling=False) for row, q in todo})
            sess.start_from(slot, plan.start(i), 750, sampling=False, forced=forced[i], source=held)
        res = drive_slots(sess, S, N, start)
        info[P] = (steps[0], sess.prefix_passes + (held.prefix_passes if held else 0))
        sess.free()
        if held:
            held.free()
        return [r[1] for r in res]

    want = [min(n, 750) for n in lengths]
    for P in (0, 4, 16):                                       # warm-up, and the same lengths every way
        assert session(P) == want, P
    best = {P: [] for P in (0, 4, 16)}
    for _ in range(2):
        for P in (0, 4, 16):
            best[P].append(timed(lambda: session(P)))
    say("  (c) 64 requests, lengths 50 .. 750 shuffled, 16 slots kept full, a look after every step (best of 2, alternating)")
    for P in (0, 4, 16):
        say(f"      prefill {P:2d}   {min(best[P]) * 1e3:8.1f} ms   {info[P][0]} steps   {info[P][1]} prefix passes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laura_start_many.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/laura_start_many.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    for name in ("laura", "lauramusic"):
        cfg = laura_recipe_config(name)
        spec = laura_spec_from_config(cfg)
        m = LauraGenMI355X(spec, "cuda:0", max_positions=1024)
        m.load_state_dict(make_laura_state_dict(cfg, 0))
        s = spec.codec_lm
        say(f"{name}: codec LM {s.layers} layers, d {s.d_model}, {s.heads} heads, ff {s.ff}; persistent step "
            f"{'available' if m.engine.set_persistent_step(True) else 'not available'} (per S: where its LDS fits)")
        part_a(m, cfg, spec, say)
        part_b(m, cfg, spec, say)
        part_c(m, cfg, spec, say)
        assert m.engine.persistent_step_fallbacks == 0
        del m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
