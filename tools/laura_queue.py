"""Time a QUEUED decoding session (``open_decode(queue=, source=)``: ended slots retire and free slots claim waiting tickets on the
device, inside the captured step) against the session without a queue, on the synthetic checkpoints of the ``laura`` and ``lauramusic``
recipes.  The method of ``tools/laura_slots_step.py`` and ``tools/laura_start_many.py``: warm-up, then 24 synchronised repetitions with
the forms alternating in one process; median and min .. max.  No pass / fail bar: what is found is reported.

A ticket takes no forced tokens, so lengths are set by ``max_length`` with ``SamplingRules(min_length=max_length)`` (greedy, <eos>
masked): every utterance runs exactly its length, in both forms.

(a) The price of the idle phase: ``step(n) / n`` and ``step(1)`` with every slot running and nothing waiting, queued against not, at
    S = 1 / 8 / 16 / 64.
(b) One refill: a ``step(1)`` in which k = 1 / 4 / 16 of 16 slots claim a waiting ticket, against k x ``start_from(source=held)`` by the
    host followed by the same ``step(1)``; the k ``submit`` calls on their own.
(c) 64 requests, lengths 50 .. 750 shuffled, 16 held rows, through 16 and 64 slots: the host's refill loop with a look after every step
    and after every 16th, and the queue with ``step(16)``: steps, milliseconds (best of 2, alternating), tokens equal.

    python tools/laura_queue.py [--out profiles/laura_queue.txt]
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

from funcodec_amd.laura import HeldPrompts, LauraGenMI355X, SamplingRules, drive_queue, drive_slots   # noqa: E402
from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config                     # noqa: E402
from funcodec_amd.synth import make_laura_state_dict, synthetic_text                                  # noqa: E402

REPS, ROWS, CAP = 24, 16, 1024


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(v):
    v = sorted(v)
    return f"median {statistics.median(v) * 1e6:8.1f} us (min {v[0] * 1e6:.1f}, max {v[-1] * 1e6:.1f})"


def exactly(n):
    return SamplingRules(min_length=n)


def holding(m, cfg, n, seed=11):
    """a holding session of 16 rows with 16 prompts (texts of 16 .. 26 tokens)"""
    lens = [16 + (5 * i) % 11 for i in range(ROWS)]
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, ROWS, lens, seed)), torch.tensor(lens))
    held = m.engine.open_decode(ROWS, max_positions=CAP, logp=False)
    held.start_many({b: dict(text_outs=outs[b], text_len=lens[b], max_length=1, sampling=False) for b in range(ROWS)})
    return held


def wide(S):
    return dict(wide=True) if S > 16 else {}


def part_a(m, cfg, say):
    held = holding(m, cfg, ROWS)
    L, n = 900, 16
    say(f"  (a) every slot running, nothing waiting: one step (median of {REPS}, forms alternating)")
    for S in (1, 8, 16, 64):
        plain = m.engine.open_decode(S, max_positions=CAP, logp=False, **wide(S))
        qs = m.engine.open_decode(S, max_positions=CAP, logp=False, queue=S, source=held, **wide(S))
        for b in range(S):
            plain.start_from(b, b % ROWS, L, sampling=False, rules=exactly(L), source=held)
            qs.submit(b % ROWS, L, False, rules=exactly(L))
        plain.step(4), qs.step(4)                              # warm-up: the eager step, the capture
        assert qs.claimed == S and qs.pending == S
        a, b_, c, d = [], [], [], []
        for _ in range(REPS):
            a.append(timed(lambda: plain.step(n)) / n)
            b_.append(timed(lambda: qs.step(n)) / n)
            c.append(timed(lambda: plain.step(1)))
            d.append(timed(lambda: qs.step(1)))
        say(f"      S = {S:2d}   step(16) / 16: no queue {spread(a)}   queued {spread(b_)}   + {(statistics.median(b_) - statistics.median(a)) * 1e6:5.1f} us")
        say(f"               step(1):       no queue {spread(c)}   queued {spread(d)}   + {(statistics.median(d) - statistics.median(c)) * 1e6:5.1f} us")
        plain.free()
        qs.free()
    held.free()


def part_b(m, cfg, say):
    held = holding(m, cfg, ROWS)
    S, L = 16, 900
    say(f"  (b) one refill of k of 16 slots while the others run (median of {REPS}, forms alternating)")
    for k in (1, 4, 16):
        plain = m.engine.open_decode(S, max_positions=CAP, logp=False)
        qs = m.engine.open_decode(S, max_positions=CAP, logp=False, queue=2 * S, source=held)
        for b in range(S - k):                                 # the slots that keep running: the first S - k
            plain.start_from(b, b, L, sampling=False, rules=exactly(L), source=held)
            qs.submit(b, L, False, rules=exactly(L))
        if S - k:
            plain.step(4), qs.step(4)
        a, b_, c = [], [], []
        for r in range(REPS + 2):                              # the first two rounds are warm-up
            def host():
                for j in range(S - k, S):
                    plain.start_from(j, j, 2, sampling=False, rules=exactly(2), source=held)
                plain.step(1)
            ta = timed(host)
            for j in range(S - k, S):                          # max_length 2: ended in that step
                plain.take(j)
            tc = timed(lambda: [qs.submit(j, 2, False, rules=exactly(2)) for j in range(S - k, S)])
            before = qs.claimed
            tb = timed(lambda: qs.step(1))
            assert qs.claimed == before + k and len(qs.collect()) == k
            if r >= 2:
                a.append(ta), b_.append(tb), c.append(tc)
        say(f"      k = {k:2d}   k x start_from(source=held) + step(1) {spread(a)}   queued step(1) {spread(b_)}   "
            f"ratio {statistics.median(b_) / statistics.median(a):.3f}   k x submit {spread(c)}")
        plain.free()
        qs.free()
    held.free()


def part_c(m, cfg, say):
    N = 64
    lengths = [50 + (700 * i) // (N - 1) for i in range(N)]
    np.random.Generator(np.random.PCG64(0)).shuffle(lengths)
    lens = [16 + (5 * i) % 11 for i in range(N)]
    outs = []
    with torch.no_grad():
        for g in range(0, N, ROWS):
            o, _ = m.encode(torch.from_numpy(synthetic_text(cfg, ROWS, lens[g: g + ROWS], 11 + g)), torch.tensor(lens[g: g + ROWS]))
            outs += [o[b, : lens[g + b]] for b in range(ROWS)]
    info = {}

    def fill_rows(held, batch):
        held.start_many({row: dict(text_outs=outs[q], text_len=lens[q], max_length=1, sampling=False) for row, q in batch})

    def counted(sess):
        real, steps = sess.step, [0]

        def step(n=1):
            steps[0] += n
            return real(n)
        sess.step = step
        return steps

    def host_loop(S, step_n):
        held = m.engine.open_decode(ROWS, max_positions=CAP, logp=False)
        sess = m.engine.open_decode(S, max_positions=CAP, logp=False, **wide(S))
        plan, steps = HeldPrompts(ROWS, N, 1), counted(sess)

        def start(slot, i):
            todo = plan.need(i)
            if todo:
                fill_rows(held, todo)
            sess.start_from(slot, plan.start(i), lengths[i], sampling=False, rules=exactly(lengths[i]), source=held)
        res = drive_slots(sess, S, N, start, step_n)
        info[(S, "host", step_n)] = (steps[0], held.prefix_passes)
        sess.free(), held.free()
        return [r[0] for r in res]

    def queued(S, step_n=16):
        held = m.engine.open_decode(ROWS, max_positions=CAP, logp=False)
        sess = m.engine.open_decode(S, max_positions=CAP, logp=False, queue=S + ROWS, source=held, **wide(S))
        steps = counted(sess)
        res = drive_queue(sess, ROWS, N, 1, lambda batch: fill_rows(held, batch),
                          lambda row, i: sess.submit(row, lengths[i], False, rules=exactly(lengths[i])), step_n)
        info[(S, "queue", step_n)] = (steps[0], held.prefix_passes)
        sess.free(), held.free()
        return [r[0] for r in res]

    say("  (c) 64 requests, lengths 50 .. 750 shuffled, 16 held rows (best of 2, alternating)")
    for S in (16, 64):
        forms = [("host loop, step_n  1", lambda: host_loop(S, 1), (S, "host", 1)), ("host loop, step_n 16", lambda: host_loop(S, 16), (S, "host", 16)),
                 ("queue,     step_n 16", lambda: queued(S), (S, "queue", 16))]
        ref = None
        for _, fn, _k in forms:                                # warm-up, and the same tokens every way
            toks = fn()
            assert [t.shape[0] for t in toks] == lengths
            same = ref is None or all(torch.equal(a, b) for a, b in zip(toks, ref))
            ref = ref or toks
            assert same, "tokens differ between the forms"
        best = {name: [] for name, _, _ in forms}
        for _ in range(2):
            for name, fn, _k in forms:
                best[name].append(timed(fn))
        for name, _, key in forms:
            say(f"      S = {S:2d}   {name}   {min(best[name]) * 1e3:8.1f} ms   {info[key][0]:5d} steps   {info[key][1]} prefix passes   tokens equal")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laura_queue.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/laura_queue.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    for name in ("laura", "lauramusic"):
        cfg = laura_recipe_config(name)
        spec = laura_spec_from_config(cfg)
        m = LauraGenMI355X(spec, "cuda:0", max_positions=CAP)
        m.load_state_dict(make_laura_state_dict(cfg, 0))
        s = spec.codec_lm
        say(f"{name}: codec LM {s.layers} layers, d {s.d_model}, {s.heads} heads, ff {s.ff}; persistent step "
            f"{'available' if m.engine.set_persistent_step(True) else 'not available'} (per S: where its LDS fits)")
        part_a(m, cfg, say)
        part_b(m, cfg, say)
        part_c(m, cfg, say)
        assert m.engine.persistent_step_fallbacks == 0
        del m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
