#!/usr/bin/env python3
"""Timing of the length-aware (ragged) call on a mixed-length batch: 16 utterances with seeded lengths uniform in 1 - 10 s,
encode + all quantiser stages + decode, for ds640 and ds320wn with seeded weights.

  (a) one ragged call (lengths given);
  (b) the same results without it: 16 offline calls at B = 1 in a loop, same process, same workspace;
  (c) the offline call on the batch padded to Tmax (different results: the floor the fused kernels set).

Warm-up, then the median of synchronised repetitions, clocks as found.  `--once RECIPE` runs one ragged call after a warm-up
(for a kernel trace of that call)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.model import EncodecMI355X
from funcodec_amd.synth import make_state_dict, synthetic_audio


def load(name):
    arch = arch_from_config(recipe_config(name))
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0).items()})
    return m


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", default=None)
    args = ap.parse_args()
    sr = 16000
    lens = [int(x) for x in np.random.RandomState(2024).randint(sr, 10 * sr + 1, size=16)]
    print("lengths (samples):", lens)
    Tmax = max(lens)
    wav = torch.from_numpy(synthetic_audio(16, Tmax, 7, "noise")).cuda()
    L = torch.tensor(lens, dtype=torch.int32, device="cuda")
    rows = [wav[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
    for name in ([args.once] if args.once else ["ds640", "ds320wn"]):
        m = load(name)
        e, n_q = m.engine, m.arch.num_quantizers
        e._workspace(16, Tmax, True), e._workspace(16, Tmax)       # one workspace for all three
        ragged = lambda: e.encode_decode(wav, n_q, lengths=L)      # noqa: E731
        if args.once:
            ragged(); torch.cuda.synchronize(); ragged(); torch.cuda.synchronize()
            return
        loop = lambda: [e.encode_decode(r, n_q) for r in rows]     # noqa: E731
        padded = lambda: e.encode_decode(wav, n_q)                 # noqa: E731
        a = median_ms(ragged, args.reps, args.warmup)
        b = median_ms(loop, args.reps, args.warmup)
        c = median_ms(padded, args.reps, args.warmup)
        e.check_status(sync=True)
        print(f"{name}: n_q {n_q}, 16 utterances, {sum(lens) / sr:.1f} s of audio, Tmax {Tmax}, median of {args.reps} (min .. max), ms")
        print(f"  (a) ragged call               {a[0]:8.2f}  ({a[1]:.2f} .. {a[2]:.2f})")
        print(f"  (b) 16 offline calls at B = 1 {b[0]:8.2f}  ({b[1]:.2f} .. {b[2]:.2f})")
        print(f"  (c) offline call padded       {c[0]:8.2f}  ({c[1]:.2f} .. {c[2]:.2f})")
        print(f"  (a) / (b) = {a[0] / b[0]:.3f}   (a) / (c) = {a[0] / c[0]:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
