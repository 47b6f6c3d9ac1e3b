"""Measurements of the stage count per row chosen by a target SNR (target_snr_db; csrc/rvq_rate_kernels.h), written to
profiles/rvq_rate.txt:

  1. cost of the mode: the headline call (16 x 10 s, ds640, encode + 32 stages + decode) with a target against the plain call of the same
     tree, at rvq_beam 1 and 4.  The forms alternate in one process, median of 24, each call bracketed by HIP events and synchronised.
     The mode adds four launches to the call (stage errors, row sums + pick, the sum of the chosen codes' vectors, the zeros behind the
     counts) and a 16-entry host-to-device copy of the ratios;
  2. what it buys: over the three shipped recordings (tests/golden/wav) with the synthetic ds640 / ds320 checkpoints whose codebook sigma
     falls by 0.8 per stage, the target of every recording is its OWN greedy 32-stage SNR; reported is the mean chosen count at
     rvq_beam 1, 2, 4.  THE CHECKPOINTS ARE UNTRAINED (seeded random weights and codebooks): the counts say what the rule does on
     random codebooks, nothing about trained ones;
  3. (--bench FILE ...) nothing moved: the result lines of bench.py --gpus 1 --steps 40 --warmup 8 runs, given as label=file pairs in
     the order they were run, are copied into the report.

    python tools/rvq_rate.py [--out profiles/rvq_rate.txt] [--bench parent=a.json tree=b.json parent=c.json tree=d.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from funcodec_amd.config import arch_from_config, recipe_config  # noqa: E402
from funcodec_amd.io import read_wav  # noqa: E402
from funcodec_amd.model import EncodecMI355X  # noqa: E402
from funcodec_amd.synth import make_state_dict, synthetic_audio  # noqa: E402

REPS = 24
INF = float("inf")


def model(name, decay=1.0):
    arch = arch_from_config(recipe_config(name))
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0, decay).items()})
    return m


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)          # ms


def alternate(forms, reps=REPS, warm=3):
    """median time (ms) of every form, the forms taking turns"""
    for _ in range(warm):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            t[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in t.items()}


def bench_ms(path):
    """ms per step of a bench.py result file (its last JSON line)"""
    with open(path) as f:
        rows = [json.loads(ln) for ln in f if ln.strip().startswith("{")]
    return float(rows[-1]["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rvq_rate.txt"))
    ap.add_argument("--bench", nargs="*", default=[], metavar="LABEL=FILE")
    args = ap.parse_args()
    lines = [f"rvq rate (target_snr_db) measurements, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    m = model("ds640", 0.8)
    wav = torch.from_numpy(synthetic_audio(16, 160000, 0, "noise")).cuda()
    target = 1.0                         # dB; the cost does not depend on it: all 32 stages are coded before the pick
    forms = {}
    for w in (1, 4):
        forms[(w, False)] = lambda w=w: m.inference(wav, need_recon=True, rvq_beam=w)
        forms[(w, True)] = lambda w=w: m.inference(wav, need_recon=True, rvq_beam=w, target_snr_db=target)
    t = alternate(forms)
    ks = m.inference(wav, need_recon=True, target_snr_db=target)["n_q_rows"].tolist()
    say(f"1. cost of the mode: headline call (16 x 10 s, ds640, encode + 32-stage quantiser + decode), same tree; median of {REPS}, forms")
    say("   alternating, HIP events around each synchronised call (ms)")
    for w in (1, 4):
        a, b = t[(w, False)], t[(w, True)]
        say(f"   rvq_beam {w}: plain {a:.3f}   with target_snr_db {b:.3f}   (+{b - a:.3f} ms, {100 * (b - a) / a:+.2f} %)")
    say(f"   (target {target} dB on noise input; chosen counts {ks})")
    say()
    say("2. what it buys: target = every recording's own greedy 32-stage quantiser-domain SNR (less 1e-9 dB); chosen counts per recording")
    say("   and their mean.  UNTRAINED synthetic checkpoints (seeded random weights, Gaussian codebooks, sigma x 0.8 per stage): what the")
    say("   rule does on random codebooks, nothing about trained ones")
    wavdir = os.path.join(ROOT, "tests", "golden", "wav")
    for name in ("ds640", "ds320"):
        mm = m if name == "ds640" else model(name, 0.8)
        nq = mm.arch.num_quantizers
        rows = []
        for f in sorted(os.listdir(wavdir)):
            w, _ = read_wav(os.path.join(wavdir, f))
            w = torch.from_numpy(w[None].copy())
            E = mm.engine.encode(w, nq, target_snr_db=INF)["row_errors"][0]
            snr = 10.0 * float(torch.log10(E[0] / E[nq]))
            k = {bw: int(mm.inference_encoding(w, target_snr_db=snr - 1e-9, rvq_beam=bw)["n_q_rows"][0]) for bw in (1, 2, 4)}
            rows.append((f, snr, k))
        for f, snr, k in rows:
            say(f"   {name} {f}: greedy {nq}-stage SNR {snr:.3f} dB; k at rvq_beam 1 / 2 / 4 = {k[1]} / {k[2]} / {k[4]}")
        say(f"   {name} mean k: " + " / ".join(f"{statistics.mean(k[bw] for _, _, k in rows):.2f}" for bw in (1, 2, 4)) + "  (rvq_beam 1 / 2 / 4)")
    say()
    if args.bench:
        say("3. nothing moved: bench.py --gpus 1 --steps 40 --warmup 8, one process per entry, in the order run (ms per step)")
        runs = [(lab, bench_ms(path)) for lab, path in (b.split("=", 1) for b in args.bench)]
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
