"""Measurements of the codec's bit stream (csrc/code_pack_kernels.h; fc_codes_pack / fc_codes_unpack), written to profiles/code_pack.txt:

  1. the pack and the unpack launch at three shapes: the headline call's codes (16 x 250 frames x 32 stages x 10 bits), a slot push
     (32 x 1 x 32) and a long row (1 x 7500 x 32);
  2. codes to the host both ways at the headline shape: ``codes.cpu()`` (int64) against pack plus one copy of the packets;
  3. cost of the mode: the headline call (16 x 10 s, ds640, encode + 32 stages + decode) with ``packed=True`` against the same call
     without, in the same tree;
  4. (--bench LABEL=FILE ...) nothing moved: the result lines of bench.py --gpus 1 --steps 40 --warmup 8 runs, in the order they were run.

The forms of a comparison alternate in one process, median of 24, every call bracketed by HIP events and synchronised (host copies:
wall clock around the synchronised call).

    python tools/code_pack.py [--out profiles/code_pack.txt] [--bench parent=a.json tree=b.json parent=c.json tree=d.json]
"""
import argparse
import datetime
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from rvq_rate import REPS, alternate, bench_ms, model  # noqa: E402
from funcodec_amd.synth import synthetic_audio  # noqa: E402

SHAPES = (("headline", 16, 250, 32), ("slot push", 32, 1, 32), ("long row", 1, 7500, 32))


def wall(fn):
    """ms of a call that ends on the host (a copy), the device idle before it"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate_wall(forms, reps=REPS, warm=3):
    for _ in range(warm):
        for fn in forms.values():
            fn()
    t = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            t[k].append(wall(fn))
    return {k: statistics.median(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "code_pack.txt"))
    ap.add_argument("--bench", nargs="*", default=[], metavar="LABEL=FILE")
    args = ap.parse_args()
    lines = [f"code pack (packets) measurements, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    m = model("ds640")
    eng = m.engine
    bits = eng.code_bits
    say(f"1. the two launches alone; median of {REPS}, pack and unpack alternating, HIP events around each synchronised call (us)")
    for name, B, Tf, n_q in SHAPES:
        codes = torch.randint(0, 1 << bits, (n_q, B, Tf), dtype=torch.int64, device="cuda")
        packets = eng.pack_codes(codes)
        assert torch.equal(eng.unpack_codes(packets, Tf, n_q), codes.permute(1, 2, 0))
        t = alternate({"pack": lambda: eng.pack_codes(codes), "unpack": lambda: eng.unpack_codes(packets, Tf, n_q)})
        say(f"   {name:9s} {B:2d} x {Tf:4d} frames x {n_q} stages x {bits} bits: codes {codes.numel() * 8 / 1e6:.3f} MB, packets "
            f"{packets.numel() / 1e6:.3f} MB; pack {1e3 * t['pack']:.1f}   unpack {1e3 * t['unpack']:.1f}")
    say()
    _, B, Tf, n_q = SHAPES[0]
    codes = torch.randint(0, 1 << bits, (n_q, B, Tf), dtype=torch.int64, device="cuda")
    t = alternate_wall({"cpu": lambda: codes.cpu(), "packed": lambda: eng.packets_to_host(eng.pack_codes(codes)),
                        "packed_raw": lambda: eng.pack_codes(codes).cpu()})
    say(f"2. codes to the host at the headline shape; median of {REPS}, forms alternating, wall clock around each synchronised call (us)")
    say(f"   codes.cpu() (int64, {codes.numel() * 8 / 1e6:.3f} MB) {1e3 * t['cpu']:.1f}   pack + one copy of the packets "
        f"({eng.pack_codes(codes).numel() / 1e6:.3f} MB) {1e3 * t['packed_raw']:.1f}   the same cut into {B} bytes objects {1e3 * t['packed']:.1f}")
    say()
    wav = torch.from_numpy(synthetic_audio(16, 160000, 0, "noise")).cuda()
    t = alternate({"plain": lambda: m.inference(wav, need_recon=True), "packed": lambda: m.inference(wav, need_recon=True, packed=True)})
    a, b = t["plain"], t["packed"]
    say(f"3. cost of the mode: headline call (16 x 10 s, ds640, encode + 32-stage quantiser + decode), same tree; median of {REPS}, forms")
    say("   alternating, HIP events around each synchronised call (ms)")
    say(f"   plain {a:.3f}   packed=True {b:.3f}   ({b - a:+.3f} ms, {100 * (b - a) / a:+.2f} %)")
    say()
    if args.bench:
        say("4. nothing moved: bench.py --gpus 1 --steps 40 --warmup 8, one process per entry, in the order run (ms per step)")
        runs = [(lab, bench_ms(path)) for lab, path in (x.split("=", 1) for x in args.bench)]
        say("   " + "   ".join(f"{lab} {ms:.3f}" for lab, ms in runs))
        par = [ms for lab, ms in runs if lab == "parent"]
        tree = [ms for lab, ms in runs if lab != "parent"]
        if par and tree:
            lo, hi, spread = min(par), max(par), max(par) - min(par)
            inside = all(lo - spread <= ms <= hi + spread for ms in tree)
            say(f"   parent min .. max {lo:.3f} .. {hi:.3f} (its processes differ by {spread:.3f}); this tree {'inside' if inside else 'OUTSIDE'} "
                "that range widened by the same amount")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "wt") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
