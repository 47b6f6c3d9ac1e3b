"""Timing of the transformer bottleneck (seq_model: transformer) on one MI355X; writes the table committed as profiles/seqtf_step.txt.

    python tools/seqtf_step.py [--reps 10] [--warmup 3] [--out profiles/seqtf_step.txt]

  1. whole step, ds640tf vs ds640 at the headline shape (16 x 10 s, encode + 32-stage RVQ + decode), wall time per step between
     CUDA events (median, min, max of --reps steps after --warmup);
  2. the attention kernel alone (seq_attn_kernel<DK>, HIP events around each launch through the engine's profiling spans) inside one
     2-block TransformerEncoder (CodecEngine.seq_forward) at B = 16, T in {250, 1000, 3000}, d_k in {64, 128, 256}, causal off / on:
     microseconds per launch (median, min, max over the reps) and the fraction of the 157.3 TF fp32 MFMA peak that
     4 * B * pairs * C flops make; and the attention's share of the whole block stack's time.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from funcodec_amd.config import arch_from_config, recipe_config  # noqa: E402
from funcodec_amd.model import EncodecMI355X  # noqa: E402
from funcodec_amd.plan import encoder_plan  # noqa: E402
from funcodec_amd.synth import make_state_dict, synthetic_audio  # noqa: E402

PEAK_TF = 157.3


def engine(cfg):
    arch = arch_from_config(cfg)
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0).items()})
    return m, arch


def spread(xs):
    return f"{statistics.median(xs):9.3f} [{min(xs):.3f} .. {max(xs):.3f}]"


def whole_step(name, reps, warmup):
    m, _ = engine(recipe_config(name))
    wav = torch.from_numpy(synthetic_audio(16, 160000, 1234, "noise")).cuda()
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m.engine.encode_decode(wav, 32, use_scale=True)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def attention(C, causal, T, reps, warmup, B=16):
    cfg = recipe_config("tinytf")
    for k in ("encoder_conf", "decoder_conf"):
        cfg[k]["n_filters"] = C // 4
        if causal:
            cfg[k].update(norm="weight_norm", causal=True)
            cfg[k].pop("norm_params", None)
    m, arch = engine(cfg)
    prefix = [op.key for op in encoder_plan(arch) if op.kind == "transformer"][0]
    x = torch.randn(B, C, T, device="cuda")
    us, stack_ms = [], []
    for i in range(warmup + reps):
        m.engine.set_profiling(True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m.engine.seq_forward(prefix, x)
        b.record()
        torch.cuda.synchronize()
        prof = m.engine.read_profile()
        m.engine.set_profiling(False)
        att = [p for p in prof if p["kernel"].startswith("seq_attn_kernel")]
        if i >= warmup:
            us.append(1e3 * att[0]["total_ms"] / att[0]["launches"])
            stack_ms.append(a.elapsed_time(b))
    pairs = T * (T + 1) / 2 if causal else T * T
    flops = 4.0 * B * pairs * C
    frac = flops / (statistics.median(us) * 1e-6) / (PEAK_TF * 1e12)
    share = 2 * statistics.median(us) * 1e-3 / statistics.median(stack_ms)     # 2 blocks: 2 attention launches per stack
    return us, frac, share, stack_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqtf_step.txt"))
    args = ap.parse_args()
    lines = [f"# tools/seqtf_step.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); "
             f"{args.warmup} warm-up + {args.reps} timed repetitions, median [min .. max]", ""]
    lines.append("## whole step: 16 x 10 s, encode + 32-stage RVQ + decode (ms per step)")
    for name in ("ds640", "ds640tf"):
        lines.append(f"{name:8s} {spread(whole_step(name, args.reps, args.warmup))}")
        print(lines[-1], flush=True)
    lines += ["", "## attention kernel alone, B = 16, 4 heads (us per launch; fraction of the 157.3 TF fp32 MFMA peak; share of the 2-block stack)"]
    for dk in (64, 128, 256):
        for causal in (False, True):
            for T in (250, 1000, 3000):
                us, frac, share, stack = attention(4 * dk, causal, T, args.reps, args.warmup)
                lines.append(f"d_k {dk:3d} causal {int(causal)} T {T:4d}: {spread(us)} us  peak {frac:.3f}  "
                             f"stack {statistics.median(stack):8.3f} ms  attention share {share:.3f}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
