#!/usr/bin/env python3
"""Timing of a batch whose rows have bit rates of their own: ds640 with seeded weights, 16 utterances of 10 s, encode + quantiser +
decode, stage counts spread over 1 .. 32 (2 k + 1 and 2 k + 2 alternating: mean 16.5).

  (a) one call with the per-row stage counts (fc_engine_set_row_nq);
  (b) the same call with all 32 stages for every row (no table: the plain kernels);
  (c) the same results as (a) without the table: 16 one-utterance calls, each at its own count.

Also the quantiser alone on the same rows (8 000 frames, fc_rvq_encode), where the early end of a workgroup shows undiluted.
Warm-up, then the median of synchronised repetitions with the three forms alternating, clocks as found."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.model import EncodecMI355X
from funcodec_amd.synth import make_state_dict, synthetic_audio


def alternating_ms(fns, reps, warmup):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    B, T = 16, 160000
    arch = arch_from_config(recipe_config("ds640"))
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0).items()})
    e, cap = m.engine, arch.num_quantizers
    counts = [2 * b + 1 + (b & 1) for b in range(B)]
    assert min(counts) == 1 and max(counts) == cap
    wav = torch.from_numpy(synthetic_audio(B, T, 7, "noise")).cuda()
    rows = [wav[b:b + 1].contiguous() for b in range(B)]
    mixed = lambda: e.encode_decode(wav, cap, n_q_rows=counts)                   # noqa: E731
    full = lambda: e.encode_decode(wav, cap)                                     # noqa: E731
    loop = lambda: [e.encode_decode(r, k) for r, k in zip(rows, counts)]         # noqa: E731
    got, want = mixed(), loop()
    for b, k in enumerate(counts):                                               # faster and different is not faster
        assert torch.equal(got["codes"][:k, b], want[b]["codes"][:, 0]) and torch.equal(got["recon"][b], want[b]["recon"][0]), b
    a, f, c = alternating_ms([mixed, full, loop], args.reps, args.warmup)
    e.check_status(sync=True)
    print(f"ds640: {B} x {T / 16000:.0f} s, stage counts {counts}, median of {args.reps} alternating repetitions (min .. max), ms")
    print(f"  (a) one call, a count per row      {a[0]:8.2f}  ({a[1]:.2f} .. {a[2]:.2f})")
    print(f"  (b) one call, all {cap} stages        {f[0]:8.2f}  ({f[1]:.2f} .. {f[2]:.2f})")
    print(f"  (c) {B} one-utterance calls         {c[0]:8.2f}  ({c[1]:.2f} .. {c[2]:.2f})")
    print(f"  (a) / (b) = {a[0] / f[0]:.3f}   (a) / (c) = {a[0] / c[0]:.3f}")
    Tf = e.frames(T)
    x = (torch.randn(B * Tf, arch.codebook_dim, generator=torch.Generator().manual_seed(3)) * 1.5).cuda()
    qa, qf = alternating_ms([lambda: e.rvq_encode(x, cap, n_q_rows=counts), lambda: e.rvq_encode(x, cap)], args.reps, args.warmup)
    print(f"quantiser alone, {B * Tf} rows: a count per row {qa[0]:.3f} ms ({qa[1]:.3f} .. {qa[2]:.3f}), all {cap} stages {qf[0]:.3f} ms "
          f"({qf[1]:.3f} .. {qf[2]:.3f}), ratio {qa[0] / qf[0]:.3f} (stages run / stages of the full call: {sum(counts) / (B * cap):.3f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
