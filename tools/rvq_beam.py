"""Measurements of the quantiser's search over the stages (rvq_beam; csrc/rvq_beam_kernels.h), written to profiles/rvq_beam.txt:

  1. quantiser time at 4 000 and 8 000 rows x 32 stages, D = 128, K = 1024, widths 1 / 2 / 4 / 8.  The greedy launch and each width in the
     same process, the forms alternating, median of 24 (HIP events around one call each).  A width's call holds the greedy launch, the
     search and the sum of the final codes' vectors, so "search" = call - greedy is what the width adds;
  2. the headline encode + decode (16 x 10 s, ds640) with width 4 against width 1, same alternation;
  3. quantiser-domain SNR 10 log10(|enc_out|^2 / |enc_out - quantized|^2) over the three shipped recordings (tests/golden/wav) with the
     synthetic ds640 / ds320 checkpoints, per width, and the number of stages at which width 4 reaches greedy's 32-stage SNR.  THE
     CHECKPOINTS ARE UNTRAINED (seeded random weights and codebooks): the SNR says what the search does on random codebooks, nothing
     about trained ones.

    python tools/rvq_beam.py [--out profiles/rvq_beam.txt] [--skip-headline]
"""
import argparse
import datetime
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

WIDTHS = (1, 2, 4, 8)
REPS = 24


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
    return a.elapsed_time(b) * 1e3          # us


def alternate(forms, reps=REPS, warm=3):
    """median time (us) of every form, the forms taking turns"""
    for _ in range(warm):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            t[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in t.items()}


def snr_db(x, q):
    return 10.0 * float(torch.log10((x.double() ** 2).sum() / ((x.double() - q.double()) ** 2).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rvq_beam.txt"))
    ap.add_argument("--skip-headline", action="store_true")
    args = ap.parse_args()
    lines = [f"rvq_beam measurements, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    m = model("ds640")
    eng = m.engine
    say(f"1. quantiser time, 32 stages, D = 128, K = 1024; median of {REPS}, forms alternating (us)")
    say("   rows   greedy   " + "   ".join(f"W={w} call / search / x greedy" for w in WIDTHS[1:]))
    g = torch.Generator().manual_seed(1)
    for n in (4000, 8000):
        x = torch.randn(n, 128, generator=g).cuda()
        forms = {1: lambda: eng.rvq_encode(x, 32)}
        for w in WIDTHS[1:]:
            forms[w] = lambda w=w: eng.rvq_encode(x, 32, beam=w)
        t = alternate(forms)
        say(f"   {n:5d}  {t[1]:7.1f}   " + "   ".join(f"{t[w]:8.1f} / {t[w] - t[1]:8.1f} / {(t[w] - t[1]) / t[1]:5.2f}" for w in WIDTHS[1:]))
    say()
    if not args.skip_headline:
        wav = torch.from_numpy(synthetic_audio(16, 160000, 0, "noise")).cuda()
        forms = {w: (lambda w=w: m.inference(wav, need_recon=True, rvq_beam=w)) for w in (1, 4)}
        t = alternate(forms, reps=12, warm=2)
        say("2. headline step (16 x 10 s, ds640, encode + 32-stage quantiser + decode); median of 12, forms alternating")
        say(f"   W=1 {t[1] / 1e3:.3f} ms   W=4 {t[4] / 1e3:.3f} ms   (+{(t[4] - t[1]) / 1e3:.3f} ms, {100 * (t[4] - t[1]) / t[1]:.1f} %)")
        say()
    say("3. quantiser-domain SNR (dB), 10 log10(|enc_out|^2 / |enc_out - quantized|^2), over tests/golden/wav; UNTRAINED synthetic")
    say("   checkpoints (seeded random weights, Gaussian codebooks): what the search does on random codebooks, nothing about trained ones")
    wavdir = os.path.join(ROOT, "tests", "golden", "wav")
    for name, decay in (("ds640", 1.0), ("ds640", 0.8), ("ds320", 1.0), ("ds320", 0.8)):
        mm = m if (name, decay) == ("ds640", 1.0) else model(name, decay)
        nq = mm.arch.num_quantizers
        encs = []
        for f in sorted(os.listdir(wavdir)):
            w, sr = read_wav(os.path.join(wavdir, f))
            encs.append(mm.engine.encode(torch.from_numpy(w[None].copy()), nq, want_enc_out=True)["enc_out"][0])
        x = torch.cat(encs, 0)
        if mm.arch.codebook_dim != mm.arch.dimension:
            continue
        snr = {w: snr_db(x, mm.engine.rvq_encode(x, nq, beam=w)[1]) for w in WIDTHS}
        by_stage = [snr_db(x, mm.engine.rvq_encode(x, k, beam=4)[1]) for k in range(1, nq + 1)]
        match = next((k for k, s in enumerate(by_stage, 1) if s >= snr[1]), None)
        say(f"   {name} (codebook sigma x {decay} per stage), {x.shape[0]} frames, {nq} stages: " +
            "  ".join(f"W={w} {snr[w]:.3f}" for w in WIDTHS) + f";  W=4 reaches greedy's {nq}-stage SNR at {match} stages")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "wt") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
