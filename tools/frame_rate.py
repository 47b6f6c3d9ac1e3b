"""Measurements of the stage count per frame chosen by a target SNR (per_frame=True; csrc/rvq_rate_kernels.h) and of the bit
stream's mode 1 (csrc/code_pack_kernels.h), written to profiles/frame_rate.txt:

  1. cost of the mode: the headline call (16 x 10 s, ds640, encode + 32 stages + decode) in frame mode against the row-mode target call
     and the plain call of the same tree, at rvq_beam 1 and 4;
  2. the launches: mode-1 pack and unpack (two launches each) at the three shapes of profiles/code_pack.txt beside mode 0, same run;
  3. what it buys: over the three shipped recordings (tests/golden/wav) with the synthetic ds640 / ds320 checkpoints (UNTRAINED: seeded
     random weights, Gaussian codebooks, sigma x 0.8 per stage), targets = every recording's own greedy 32-stage SNR and 6 dB; the row
     rule against the frame rule (floor 0) at rvq_beam 1 and 4: mean stages per frame, achieved row_snr_db, and packet bytes (mode 0 /
     mode 1, the count bits included).  Reported as found;
  4. (--bench LABEL=FILE ...) nothing moved: the result lines of bench.py --gpus 1 --steps 40 --warmup 8 runs, in the order they were run.

The forms of a comparison alternate in one process, median of 24, every call bracketed by HIP events and synchronised.

    python tools/frame_rate.py [--out profiles/frame_rate.txt] [--bench parent=a.json tree=b.json parent=c.json tree=d.json]
"""
import argparse
import datetime
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from code_pack import SHAPES  # noqa: E402
from rvq_rate import INF, REPS, alternate, bench_ms, model  # noqa: E402
from funcodec_amd.io import read_wav  # noqa: E402
from funcodec_amd.synth import synthetic_audio  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_rate.txt"))
    ap.add_argument("--bench", nargs="*", default=[], metavar="LABEL=FILE")
    args = ap.parse_args()
    lines = [f"frame rate (target_snr_db, per_frame=True) and mode-1 packet measurements, {datetime.date.today().isoformat()}, "
             f"{torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    m = model("ds640", 0.8)
    eng = m.engine
    wav = torch.from_numpy(synthetic_audio(16, 160000, 0, "noise")).cuda()
    target = 1.0                         # dB; the cost does not depend on it: all 32 stages are coded before the pick
    forms = {}
    for w in (1, 4):
        forms[(w, "plain")] = lambda w=w: m.inference(wav, need_recon=True, rvq_beam=w)
        forms[(w, "row")] = lambda w=w: m.inference(wav, need_recon=True, rvq_beam=w, target_snr_db=target)
        forms[(w, "frame")] = lambda w=w: m.inference(wav, need_recon=True, rvq_beam=w, target_snr_db=target, per_frame=True, min_n_q=0)
    t = alternate(forms)
    say(f"1. cost of the mode: headline call (16 x 10 s, ds640, encode + 32-stage quantiser + decode), same tree; median of {REPS}, forms")
    say("   alternating, HIP events around each synchronised call (ms)")
    for w in (1, 4):
        a, b, c = t[(w, "plain")], t[(w, "row")], t[(w, "frame")]
        say(f"   rvq_beam {w}: plain {a:.3f}   target per row {b:.3f}   target per frame {c:.3f}   (frame - row {c - b:+.3f} ms, frame - plain "
            f"{c - a:+.3f} ms, {100 * (c - a) / a:+.2f} %)")
    say()
    bits = eng.code_bits
    say(f"2. the launches alone; median of {REPS}, the four forms alternating, HIP events around each synchronised call (us); mode 1 is two")
    say("   launches each way (the scan of the counts, then the words / tokens) and allocates its scan workspace per call")
    for name, B, Tf, n_q in SHAPES:
        codes = torch.randint(0, 1 << bits, (n_q, B, Tf), dtype=torch.int64, device="cuda")
        kf = torch.randint(0, n_q + 1, (B, Tf), dtype=torch.int32, device="cuda")
        p0, p1 = eng.pack_codes(codes), eng.pack_codes(codes, n_q_frames=kf)
        tok, back = eng.unpack_frame_codes(p1, Tf, n_q)
        keep = torch.arange(n_q, device="cuda")[None, None, :] < kf[:, :, None]
        assert torch.equal(back, kf) and torch.equal(tok, torch.where(keep, codes.permute(1, 2, 0), torch.zeros_like(tok)))
        t = alternate({"pack0": lambda: eng.pack_codes(codes), "unpack0": lambda: eng.unpack_codes(p0, Tf, n_q),
                       "pack1": lambda: eng.pack_codes(codes, n_q_frames=kf), "unpack1": lambda: eng.unpack_frame_codes(p1, Tf, n_q)})
        say(f"   {name:9s} {B:2d} x {Tf:4d} frames x {n_q} stages x {bits} bits: mode 0 pack {1e3 * t['pack0']:.1f} unpack {1e3 * t['unpack0']:.1f}   "
            f"mode 1 pack {1e3 * t['pack1']:.1f} unpack {1e3 * t['unpack1']:.1f}   (pitch {p0.shape[1]} / {p1.shape[1]} bytes)")
    say()
    say("3. what it buys: row rule against frame rule (floor 0).  UNTRAINED synthetic checkpoints (seeded random weights, Gaussian codebooks,")
    say("   sigma x 0.8 per stage): what the rules do on random codebooks, nothing about trained ones.  Per recording and target: mean")
    say("   stages per frame, achieved row_snr_db, packet bytes (row: mode 0; frame: mode 1 with its count bits)")
    wavdir = os.path.join(ROOT, "tests", "golden", "wav")
    for name in ("ds640", "ds320"):
        mm = m if name == "ds640" else model(name, 0.8)
        nq = mm.arch.num_quantizers
        for f in sorted(os.listdir(wavdir)):
            w, _ = read_wav(os.path.join(wavdir, f))
            w = torch.from_numpy(w[None].copy())
            E = mm.engine.encode(w, nq, target_snr_db=INF)["row_errors"][0]
            own = 10.0 * float(torch.log10(E[0] / E[nq]))
            for label, tgt in ((f"own greedy {nq}-stage SNR {own:.3f} dB", own - 1e-9), ("6 dB", 6.0)):
                say(f"   {name} {f}, target {label}:")
                for bw in (1, 4):
                    r = mm.inference_encoding(w, target_snr_db=tgt, rvq_beam=bw, packed=True)
                    fr = mm.inference_encoding(w, target_snr_db=tgt, rvq_beam=bw, packed=True, per_frame=True, min_n_q=0)
                    rb, fb = (len(mm.engine.packets_to_host(x["packets"])[0]) for x in (r, fr))
                    Tf = fr["n_q_frames"].shape[1]
                    say(f"      rvq_beam {bw}: row k {int(r['n_q_rows'][0])}, {float(r['row_snr_db'][0]):.3f} dB, {rb} bytes   |   frame mean k "
                        f"{int(fr['n_codes_rows'][0]) / Tf:.2f} (max {int(fr['n_q_rows'][0])}), {float(fr['row_snr_db'][0]):.3f} dB, {fb} bytes "
                        f"({100.0 * (fb - rb) / rb:+.1f} %)")
    say()
    if args.bench:
        say("4. nothing moved: bench.py --gpus 1 --steps 40 --warmup 8, one process per entry, in the order run (ms per step)")
        runs = [(lab, bench_ms(path)) for lab, path in (x.split("=", 1) for x in args.bench)]
        say("   " + "   ".join(f"{lab} {ms:.3f}" for lab, ms in runs))
        par = [ms for lab, ms in runs if lab == "parent"]
        tree = [ms for lab, ms in runs if lab != "parent"]
        if par and tree:
            lo, hi, spread = min(par), max(par), max(par) - min(par)
            slower = [ms for ms in tree if ms > hi + spread]
            faster = [ms for ms in tree if ms < lo - spread]
            say(f"   parent min .. max {lo:.3f} .. {hi:.3f} (its processes differ by {spread:.3f}); of this tree's {len(tree)} figures {len(slower)} lie above "
                f"that range widened by the same amount (slower) and {len(faster)} below it (faster)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "wt") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
