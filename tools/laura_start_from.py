"""Time ``DecodeSlots.start_from`` (a slot started from the prompt another slot holds: a device copy of the prefix instead of a prefix
pass) on the synthetic checkpoints of the ``laura`` and ``lauramusic`` recipes.

(a) ``start`` against ``start_from`` with 15 of 16 slots running, prompts of the size ``tools/laura_slots_step.py`` times its start
    with (texts of 16 .. 26 tokens).  Warm-up, then synchronised repetitions, the two forms alternating; median and min .. max.
    Condition: start_from costs less than 0.25 of start in the same run (reported, and the exit status says so).
(b) 16 requests x 4 samples through 16 slots with ``Text2Audio.generate_many(samples=4)`` against the same 64 candidates listed as
    64 requests with the same seeds: equal tokens first, then total time (fine predictor and codec decoder included, the same work
    in both) and the number of prefix passes.
(c) The copy kernel's time from a ``rocprofv3 --kernel-trace --stats`` run of its own (a child process that does nothing but starts
    and copies), and its bytes from shapes: 2 * layers * d * P * 4 * (1 + n).  No bar.

    python tools/laura_start_from.py [--out profiles/laura_start_from.txt]
"""
import argparse
import csv
import datetime
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from funcodec_amd.laura import DecodeSlots, LauraGenMI355X                          # noqa: E402
from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config   # noqa: E402
from funcodec_amd.synth import make_laura_state_dict, synthetic_text                # noqa: E402

REPS, S = 24, 16
CODEC = {"laura": "ds640", "lauramusic": "freqmp640"}          # the codecs the end-to-end fixtures pair the recipes with
COPY_TEXT, COPY_CONT, COPY_CALLS = 26, (0, 272), 32            # (c): P = 28 (text alone) and 300 (with prompt tokens); copies per run


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(v):
    v = sorted(v)
    return f"median {statistics.median(v) * 1e6:8.1f} us (min {v[0] * 1e6:.1f}, max {v[-1] * 1e6:.1f})"


def model_of(name):
    cfg = laura_recipe_config(name)
    spec = laura_spec_from_config(cfg)
    m = LauraGenMI355X(spec, "cuda:0", max_positions=1024)
    m.load_state_dict(make_laura_state_dict(cfg, 0))
    return cfg, spec, m


def crowd(m, cfg, spec, n_run):
    """A session of 16 slots with the first n_run running (forced tokens: nobody ends), 32 steps in; the prompts, their lengths."""
    lens = [16 + (5 * i) % 11 for i in range(S)]
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, S, lens, 11)), torch.tensor(lens))
    rng = np.random.Generator(np.random.PCG64(9))
    forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(S, 750, spec.predict_nq)).astype(np.int64)).cuda()
    sess = m.engine.open_decode(S, max_positions=1024, logp=False)
    for b in range(n_run):
        sess.start(b, outs[b], lens[b], 750, sampling=False, forced=forced[b])
    sess.step(32)
    return sess, outs, lens, forced


def part_a(m, cfg, spec, say):
    sess, outs, lens, forced = crowd(m, cfg, spec, S - 1)
    a, b = [], []
    for r in range(REPS + 2):                                  # the first two rounds are warm-up
        j = r % (S - 1)                                        # the prompt of running slot j: by a prefix pass, then by a copy from j
        ta = timed(lambda: sess.start(S - 1, outs[j], lens[j], 750, sampling=False, forced=forced[j]))
        sess.step(4)
        tb = timed(lambda: sess.start_from(S - 1, j, 750, sampling=False, forced=forced[j]))
        sess.step(4)
        if r >= 2:
            a.append(ta)
            b.append(tb)
    sess.free()
    ratio = statistics.median(b) / statistics.median(a)
    say(f"  (a) 15 slots running, text of {min(lens)} .. {max(lens)} tokens, {REPS} repetitions, forms alternating")
    say(f"      start      {spread(a)}")
    say(f"      start_from {spread(b)}")
    say(f"      start_from / start = {ratio:.4f}   (condition: < 0.25: {'met' if ratio < 0.25 else 'MISSED'})")
    return ratio < 0.25


def part_b(name, cfg, spec, say):
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.synth import make_freq_state_dict, make_state_dict, synthetic_text_embedder, write_checkpoint
    ccfg = recipe_config(CODEC[name])
    csd = make_freq_state_dict(ccfg, 0) if CODEC[name].startswith("freq") else make_state_dict(arch_from_config(ccfg), 0)
    lsd = make_laura_state_dict(cfg, 0)
    lsd["quantizer_codebook.embed"] = csd["quantizer.rq.model.embed"][: spec.num_quantizers].copy()
    tmp = tempfile.mkdtemp(prefix="laura_start_from_")
    try:
        lc, lp = write_checkpoint(os.path.join(tmp, "laura"), cfg, lsd)
        del lsd
        cc, cp = write_checkpoint(os.path.join(tmp, "codec"), ccfg, csd)
        t2a = Text2Audio(config_file=lc, model_file=lp, device="cuda", text_emb_model=synthetic_text_embedder(cfg, 5), beam_size=1,
                         sampling=True, continual=True, codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False,
                         exclude_prompt=True, max_length=100, max_positions=256)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    n, N = 16, 4
    texts = [" ".join(f"w{i}x{k}" for k in range(16 + (5 * i) % 11)) for i in range(n)]
    seeds = [[1000 + N * i + k for k in range(N)] for i in range(n)]
    passes = [0]
    real = DecodeSlots.start

    def counting(self, *a, **k):
        passes[0] += 1
        return real(self, *a, **k)
    DecodeSlots.start = counting
    try:
        def shared():
            passes[0] = 0
            return t2a.generate_many(texts, slots=S, seeds=seeds, samples=N)[1]

        def listed():
            passes[0] = 0
            return t2a.generate_many([t for t in texts for _ in range(N)], slots=S, seeds=[v for row in seeds for v in row])[1]
        got, ref = shared(), listed()                          # warm-up, and the same tokens both ways
        p_shared = 0
        for i in range(n):
            for k in range(N):
                assert torch.equal(got[i][k], ref[N * i + k]), (i, k)
        t_listed, t_shared = [], []
        for _ in range(3):
            t_listed.append(timed(listed))
            p_listed = passes[0]
            t_shared.append(timed(shared))
            p_shared = passes[0]
    finally:
        DecodeSlots.start = real
    say(f"  (b) 16 requests x 4 samples, 16 slots, max_length 100, tokens equal; generate_many in all (median of 3, alternating)")
    say(f"      64 requests              {statistics.median(t_listed) * 1e3:8.1f} ms, {p_listed} prefix passes")
    say(f"      16 requests, samples = 4 {statistics.median(t_shared) * 1e3:8.1f} ms, {p_shared} prefix passes")
    del t2a
    torch.cuda.empty_cache()


def copy_child(name, cont_len):
    """What the profiled child runs: one start, then COPY_CALLS copies of its prefix into the other slots."""
    cfg, spec, m = model_of(name)
    n = COPY_TEXT
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, 1, [n], 11)), torch.tensor([n]))
    rng = np.random.Generator(np.random.PCG64(3))
    cont = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(cont_len, spec.predict_nq)).astype(np.int64)) if cont_len else None
    sess = m.engine.open_decode(S, max_positions=1024, logp=False)
    sess.start(0, outs[0], n, 700, sampling=False, continual=cont)
    for r in range(COPY_CALLS):
        sess.start_from(1 + r % (S - 1), 0, 700, sampling=True, seed=r)
    torch.cuda.synchronize()
    sess.free()


def part_c(name, spec, cont_len, say):
    P = COPY_TEXT + 2 + cont_len
    out = tempfile.mkdtemp(prefix="laura_start_from_rp_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "out", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--copy-child", f"{name}:{cont_len}"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"the profiled run failed ({r.returncode}):\n{r.stdout[-2000:]}")
        rows = []
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += [row for row in csv.DictReader(f) if "prefix_import_kernel" in row["Name"]]
        if len(rows) != 1 or int(rows[0]["Calls"]) != COPY_CALLS:
            raise RuntimeError(f"no statistics for {COPY_CALLS} prefix_import_kernel launches: {rows}")
    finally:
        shutil.rmtree(out, ignore_errors=True)
    row = rows[0]
    s = spec.codec_lm
    nbytes = 2 * s.layers * s.d_model * P * 4 * (1 + 1)
    avg = float(row["AverageNs"])
    say(f"  (c) prefix_import_kernel, P = {P:3d}, n = 1: {COPY_CALLS} launches, average {avg / 1e3:.2f} us "
        f"(min {int(row['MinNs']) / 1e3:.2f}, max {int(row['MaxNs']) / 1e3:.2f}); {nbytes} bytes from shapes "
        f"(2 * {s.layers} * {s.d_model} * {P} * 4 * 2) = {nbytes / avg:.1f} GB/s (rocprofv3 --kernel-trace --stats, own run)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laura_start_from.txt"))
    ap.add_argument("--copy-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.copy_child:
        name, cont_len = args.copy_child.split(":")
        copy_child(name, int(cont_len))
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/laura_start_from.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    ok = True
    for name in ("laura", "lauramusic"):
        cfg, spec, m = model_of(name)
        s = spec.codec_lm
        say(f"{name}: codec LM {s.layers} layers, d {s.d_model}, {s.heads} heads, ff {s.ff}; persistent step "
            f"{'available' if m.engine.set_persistent_step(True) else 'not available'} (per S: where its LDS fits)")
        ok = part_a(m, cfg, spec, say) and ok
        assert m.engine.persistent_step_fallbacks == 0
        del m
        torch.cuda.empty_cache()
        part_b(name, cfg, spec, say)
        for cont_len in COPY_CONT:
            part_c(name, spec, cont_len, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
