"""Time ``DecodeSlots.fork`` and ``DecodeSlots.rewind`` (a slot takes up an utterance as it stood after its first `keep` generated
tokens: a device copy and a few counters) on the synthetic checkpoints of the ``laura`` and ``lauramusic`` recipes.

(a) Per keep in 1, 100, 300, with 15 of 16 slots running (texts of 16 .. 26 tokens, forced tokens so that nobody ends): warm-up, then
    synchronised repetitions, the forms alternating; median and min .. max of
      fork        the utterance of a running slot into slot 15,
      rewind      slot 15 back to `keep` in place,
      start       the only way to that state without them: a prefix pass over the prompt plus the kept tokens as `continual`,
      start_from  for scale: the copy of the bare prefix,
    and of one decoding step of the session.  The session keeps log-probabilities, so the fork copies keep x vocab floats of them.
(b) The kernels' times from a ``rocprofv3 --kernel-trace --stats`` run of its own (a child process that does nothing but one start,
    the steps and forks at keep = 300), and the cache copy's bytes from shapes: 2 * layers * d * (P + keep - 1) * 4 * 2.  No bar.

    python tools/laura_fork.py [--out profiles/laura_fork.txt]
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

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from funcodec_amd.synth import synthetic_text                  # noqa: E402
from laura_start_from import REPS, S, model_of, spread, timed  # noqa: E402

KEEPS = (1, 100, 300)
MAXLEN = 750
COPY_TEXT, COPY_KEEP, COPY_CALLS = 26, 300, 32


def crowd(m, cfg, spec, steps):
    """A session of 16 slots, the first 15 running on forced tokens, `steps` steps in; the prompts, their lengths, the forced tokens."""
    lens = [16 + (5 * i) % 11 for i in range(S)]
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, S, lens, 11)), torch.tensor(lens))
    rng = np.random.Generator(np.random.PCG64(9))
    forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(S, MAXLEN, spec.predict_nq)).astype(np.int64)).cuda()
    sess = m.engine.open_decode(S, max_positions=1024, logp=True)
    for b in range(S - 1):
        sess.start(b, outs[b], lens[b], MAXLEN, sampling=False, forced=forced[b])
    sess.step(steps)
    return sess, outs, lens, forced


def part_a(m, cfg, spec, keep, say):
    sess, outs, lens, forced = crowd(m, cfg, spec, max(keep + 8, 32))
    d = S - 1
    t = {k: [] for k in ("fork", "rewind", "start", "start_from", "step")}
    for r in range(REPS + 2):                                  # the first two rounds are warm-up
        j = r % (S - 1)
        assert sess.n_gen(j) >= keep + 8
        one = {}
        one["fork"] = timed(lambda: sess.fork(d, j, keep, MAXLEN, sampling=False))
        one["step"] = timed(lambda: sess.step(4)) / 4
        one["rewind"] = timed(lambda: sess.rewind(d, keep, MAXLEN, sampling=False))
        sess.step(4)
        one["start"] = timed(lambda: sess.start(d, outs[j], lens[j], MAXLEN - keep, sampling=False, continual=forced[j, :keep],
                                                forced=forced[j, keep:]))
        sess.step(4)
        one["start_from"] = timed(lambda: sess.start_from(d, j, MAXLEN, sampling=False, forced=forced[j]))
        sess.step(4)
        if r >= 2:
            for k, v in one.items():
                t[k].append(v)
    assert all(v == "running" for v in sess.step(1).values()), "nobody may have ended"
    sess.free()
    say(f"  (a) keep = {keep:3d}: 15 slots running, text of {min(lens)} .. {max(lens)} tokens, {REPS} repetitions, forms alternating")
    for k in ("fork", "rewind", "start", "start_from", "step"):
        say(f"      {k:10s} {spread(t[k])}")
    med = {k: statistics.median(v) for k, v in t.items()}
    say(f"      fork - start_from = {(med['fork'] - med['start_from']) * 1e6:+.1f} us, rewind - start_from = "
        f"{(med['rewind'] - med['start_from']) * 1e6:+.1f} us, one step = {med['step'] * 1e6:.1f} us;  fork / start = "
        f"{med['fork'] / med['start']:.4f}, rewind / start = {med['rewind'] / med['start']:.4f}")
    return med


def copy_child(name):
    """What the profiled child runs: one start, COPY_KEEP + 8 steps, then COPY_CALLS forks at keep = COPY_KEEP into the other slots."""
    cfg, spec, m = model_of(name)
    n = COPY_TEXT
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, 1, [n], 11)), torch.tensor([n]))
    rng = np.random.Generator(np.random.PCG64(3))
    forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(MAXLEN, spec.predict_nq)).astype(np.int64))
    sess = m.engine.open_decode(S, max_positions=1024, logp=True)
    sess.start(0, outs[0], n, MAXLEN, sampling=False, forced=forced)
    sess.step(COPY_KEEP + 8)
    for r in range(COPY_CALLS):
        sess.fork(1 + r % (S - 1), 0, COPY_KEEP, MAXLEN, sampling=False)
    torch.cuda.synchronize()
    sess.free()


def part_b(name, spec, say):
    P = COPY_TEXT + 2
    out = tempfile.mkdtemp(prefix="laura_fork_rp_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "out", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--copy-child", name]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"the profiled run failed ({r.returncode}):\n{r.stdout[-2000:]}")
        rows = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k in ("prefix_import_kernel", "slot_branch_kernel"):
                        if k in row["Name"]:
                            rows[k] = row
        if set(rows) != {"prefix_import_kernel", "slot_branch_kernel"} or any(int(v["Calls"]) != COPY_CALLS for v in rows.values()):
            raise RuntimeError(f"no statistics for {COPY_CALLS} launches of both kernels: {rows}")
    finally:
        shutil.rmtree(out, ignore_errors=True)
    s = spec.codec_lm
    pos = P + COPY_KEEP - 1
    nbytes = 2 * s.layers * s.d_model * pos * 4 * 2
    row = rows["prefix_import_kernel"]
    avg = float(row["AverageNs"])
    say(f"  (b) prefix_import_kernel, keep = {COPY_KEEP}, {pos} positions: {COPY_CALLS} launches, average {avg / 1e3:.2f} us "
        f"(min {int(row['MinNs']) / 1e3:.2f}, max {int(row['MaxNs']) / 1e3:.2f}); {nbytes} bytes from shapes "
        f"(2 * {s.layers} * {s.d_model} * {pos} * 4 * 2) = {nbytes / avg / 1e3:.2f} TB/s (rocprofv3 --kernel-trace --stats, own run)")
    row = rows["slot_branch_kernel"]
    lbytes = 2 * COPY_KEEP * spec.lm_vocab * 4
    say(f"      slot_branch_kernel: average {float(row['AverageNs']) / 1e3:.2f} us (min {int(row['MinNs']) / 1e3:.2f}, max "
        f"{int(row['MaxNs']) / 1e3:.2f}); {lbytes} bytes of log-probability rows copied ({COPY_KEEP} x {spec.lm_vocab} floats, read and "
        f"written), {(MAXLEN - COPY_KEEP) * spec.lm_vocab * 4} zeroed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laura_fork.txt"))
    ap.add_argument("--copy-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.copy_child:
        copy_child(args.copy_child)
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/laura_fork.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    for name in ("laura", "lauramusic"):
        cfg, spec, m = model_of(name)
        s = spec.codec_lm
        say(f"{name}: codec LM {s.layers} layers, d {s.d_model}, {s.heads} heads, ff {s.ff}; persistent step "
            f"{'available' if m.engine.set_persistent_step(True) else 'not available'} (per S: where its LDS fits)")
        for keep in KEEPS:
            part_a(m, cfg, spec, keep, say)
        assert m.engine.persistent_step_fallbacks == 0
        del m
        torch.cuda.empty_cache()
        part_b(name, spec, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
