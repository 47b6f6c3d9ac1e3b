"""Time WIDE decoding sessions of the LauraTTS engine (``open_decode(wide=True)``: up to 64 slots, the step's GEMV over column blocks of
16 rows) on the synthetic checkpoints of the ``laura`` and ``lauramusic`` recipes.  The method is tools/laura_slots_step.py's.

1. One session step at S = 16 / 32 / 48 / 64 with every slot running: forced tokens (nobody ends), every slot rewound to 8 generated
   tokens ahead of each repetition, ``step(64) / 64``.  Warm-up, then 24 synchronised repetitions, the widths alternating in ONE
   process; median and min .. max, and slots / step time against S = 16.
2. The 64 requests of tools/laura_slots_step.py (lengths 50 .. 750, shuffled; forced tokens, then a forced <eos>) through 16, 32 and 64
   slots kept full (``drive_slots``, a look after every step): steps run and total time, best of 2.
3. The memory of a slot: the difference of two sessions' state sizes, with and without log-probability rows.
4. With ``--parent-tree DIR`` (a checkout of the parent commit with its library built): the S = 16 step of this tree against the
   parent's, measured by the same code in processes of their own, PROCS per tree, the trees alternating.  Condition: this tree's median
   lies inside the parent's min .. max, or beyond it by no more than the parent's own two processes differ (the exit status says so).
   A check that nothing moved for narrow sessions, not a gain.

    python tools/laura_wide_step.py [--parent-tree DIR] [--out profiles/laura_wide_step.txt]
"""
import argparse
import datetime
import inspect
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:                                       # a child measuring another checkout: its package, this file's code
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]))
else:
    sys.path.insert(0, ROOT)

REPS, WIDTHS, MAXLEN, BACK, STEPS, PROCS = 24, (16, 32, 48, 64), 750, 8, 64, 2


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(v):
    v = sorted(v)
    return f"median {statistics.median(v) * 1e6:7.1f} us (min {v[0] * 1e6:.1f}, max {v[-1] * 1e6:.1f})"


def load(name):
    from funcodec_amd.laura import LauraGenMI355X
    from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
    from funcodec_amd.synth import make_laura_state_dict
    cfg = laura_recipe_config(name)
    spec = laura_spec_from_config(cfg)
    m = LauraGenMI355X(spec, "cuda:0", max_positions=1024)
    m.load_state_dict(make_laura_state_dict(cfg, 0))
    return m, cfg, spec


def step_times(m, cfg, spec, widths):
    """{S: [seconds per step, REPS of them]}: one session per width, all open together, the widths alternating"""
    from funcodec_amd.synth import synthetic_text
    wide = "wide" in inspect.signature(m.engine.open_decode).parameters        # the parent commit has no such sessions
    S_max = max(widths)
    lens = [16 + (5 * i) % 11 for i in range(S_max)]
    outs = []
    with torch.no_grad():
        for g in range(0, S_max, 16):
            o, _ = m.encode(torch.from_numpy(synthetic_text(cfg, 16, lens[g: g + 16], 11 + g)), torch.tensor(lens[g: g + 16]))
            outs += [o[b, : lens[g + b]] for b in range(16)]
    rng = np.random.Generator(np.random.PCG64(9))
    forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(S_max, MAXLEN, spec.predict_nq)).astype(np.int64)).cuda()
    sess = {}
    for S in widths:
        s = m.engine.open_decode(S, max_positions=1024, logp=False, wide=True) if wide else m.engine.open_decode(S, max_positions=1024, logp=False)
        for b in range(S):
            s.start(b, outs[b], lens[b], MAXLEN, sampling=False, forced=forced[b])
        s.step(BACK + 8)
        sess[S] = s
    t = {S: [] for S in widths}
    for r in range(REPS + 2):                                  # the first two rounds are warm-up
        for S, s in sess.items():
            for b in range(S):
                s.rewind(b, BACK, MAXLEN, sampling=False)
            one = timed(lambda: s.step(STEPS)) / STEPS
            if r >= 2:
                t[S].append(one)
    for S, s in sess.items():
        st = s.step(1)
        assert len(st) == S and all(v == "running" for v in st.values()), "every slot runs, nobody may have ended"
        s.free()
    return t


def part_steps(m, cfg, spec, say):
    t = step_times(m, cfg, spec, WIDTHS)
    base = statistics.median(t[16])
    say(f" 1. one step, every slot running at {BACK} .. {BACK + STEPS} generated tokens (step({STEPS}) / {STEPS}, {REPS} repetitions, the widths "
        f"alternating in one process)")
    for S in WIDTHS:
        med = statistics.median(t[S])
        say(f"    S = {S:2d}  {spread(t[S])}   x {med / base:4.2f} the S = 16 step   {S / med / 1e3:7.1f} slot-steps / ms = x "
            f"{(S / med) / (16 / base):4.2f} of S = 16")


def part_requests(m, cfg, spec, say):
    from funcodec_amd.laura import drive_slots
    from funcodec_amd.synth import synthetic_text
    N = 64
    K, nq = spec.codebook_size, spec.predict_nq
    lengths = [50 + (700 * i) // (N - 1) for i in range(N)]
    np.random.Generator(np.random.PCG64(0)).shuffle(lengths)
    lens = [16 + (5 * i) % 11 for i in range(N)]
    rng = np.random.Generator(np.random.PCG64(9))
    forced = rng.integers(0, K, size=(N, 750, nq)).astype(np.int64)
    for i, n in enumerate(lengths):
        if n < 750:
            forced[i, n:] = K                                  # a forced <eos>: the row ends after n tokens
    forced = torch.from_numpy(forced).cuda()
    outs = []
    with torch.no_grad():
        for g in range(0, N, 16):
            o, _ = m.encode(torch.from_numpy(synthetic_text(cfg, 16, lens[g: g + 16], 11 + g)), torch.tensor(lens[g: g + 16]))
            outs.append(o)
    steps = [0]

    def session(S):
        sess = m.engine.open_decode(S, max_positions=1024, logp=False, wide=True)
        real_step = sess.step

        def counting(n=1):
            st = real_step(n)
            steps[0] += n
            return st
        sess.step = counting
        steps[0] = 0
        res = drive_slots(sess, S, N, lambda slot, i: sess.start(slot, outs[i // 16][i % 16], lens[i], 750, sampling=False, forced=forced[i]))
        sess.free()
        return [r[1] for r in res]

    say(f" 2. {N} requests, lengths 50 .. 750 shuffled ({sum(lengths)} tokens), slots kept full, a look after every step (best of 2)")
    base = None
    for S in (16, 32, 64):
        assert session(S) == [min(n, 750) for n in lengths]    # warm-up, and the lengths asked for
        t = min(timed(lambda: session(S)) for _ in range(2))
        base = base or t
        say(f"    {S:2d} slots  {steps[0]:5d} steps  {t * 1e3:8.1f} ms   x {t / base:4.2f} the 16-slot time")


def part_memory(m, spec, say):
    lib, h = m.engine.lib, m.engine._h
    say(" 3. state of a session per slot (fc_laura_slots_state_bytes_wide, (64 slots - 48 slots) / 16)")
    s = spec.codec_lm
    for R in (256, 1024):
        per = [(lib.fc_laura_slots_state_bytes_wide(h, 64, R, lp, 0) - lib.fc_laura_slots_state_bytes_wide(h, 48, R, lp, 0)) / 16 for lp in (0, 1)]
        kv = 2 * s.layers * s.d_model * R * 4
        say(f"    max_positions {R:4d}: {per[0] / 2 ** 20:7.2f} MiB without log-probability rows (key / value rows {kv / 2 ** 20:.2f} MiB), "
            f"{per[1] / 2 ** 20:7.2f} MiB with them")


def step_child(name):
    m, cfg, spec = load(name)
    t = step_times(m, cfg, spec, (16,))
    assert m.engine.persistent_step_fallbacks == 0
    print("LAURA_WIDE_JSON " + json.dumps(t[16]), flush=True)


def run_child(name, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--step-child", name] + (["--tree", tree] if tree else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LAURA_WIDE_JSON ")), None)
    if r.returncode != 0 or line is None:
        raise RuntimeError(f"the measuring process failed ({r.returncode}):\n{r.stdout[-2000:]}")
    return json.loads(line[len("LAURA_WIDE_JSON "):])


def part_parent(name, tree, say):
    owns, pars = [], []
    for _ in range(PROCS):
        pars.append(run_child(name, tree))
        owns.append(run_child(name, None))
    own, par = sorted(v for r in owns for v in r), sorted(v for r in pars for v in r)
    meds = lambda runs: " / ".join(f"{statistics.median(r) * 1e6:.1f}" for r in runs)      # noqa: E731
    mo = statistics.median(own)
    gap = abs(statistics.median(pars[0]) - statistics.median(pars[1]))
    beyond = max(par[0] - mo, mo - par[-1], 0.0)
    ok = beyond <= gap
    say(f" 4. the S = 16 step against the parent commit ({PROCS} processes per tree, the trees alternating, {REPS} repetitions each, pooled; "
        f"medians per process in brackets)")
    say(f"    this tree  {spread(own)}  [{meds(owns)}]")
    say(f"    parent     {spread(par)}  [{meds(pars)}]   its two processes differ by {gap * 1e6:.1f} us")
    say(f"    this tree's median is {'inside the parent min .. max' if beyond == 0 else f'{beyond * 1e6:.1f} us beyond the parent min .. max'}: "
        f"{'nothing moved' if ok else 'NOT within the condition'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laura_wide_step.txt"))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--step-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step_child:
        step_child(args.step_child)
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"tools/laura_wide_step.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    ok = True
    for name in ("laura", "lauramusic"):
        m, cfg, spec = load(name)
        s = spec.codec_lm
        say(f"{name}: codec LM {s.layers} layers, d {s.d_model}, {s.heads} heads, ff {s.ff}; above 16 slots the step is the kernel chain, "
            f"key ranges per head 256 / (S x heads) in 1 .. 8")
        part_steps(m, cfg, spec, say)
        part_requests(m, cfg, spec, say)
        part_memory(m, spec, say)
        assert m.engine.persistent_step_fallbacks == 0
        del m
        torch.cuda.empty_cache()
        write()
        if args.parent_tree:
            ok = part_parent(name, args.parent_tree, say) and ok
        else:
            say(" 4. no --parent-tree: the parent's step was not measured")
        write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
