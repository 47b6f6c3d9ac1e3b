"""Time ELASTIC decoding sessions of the LauraTTS engine (``open_decode(elastic=True)``: a step over the column blocks in use, rows
compacted by ``DecodeSlots.move``) on the synthetic checkpoints of the ``laura`` and ``lauramusic`` recipes.  The method of
tools/laura_wide_step.py: warm-up, then 24 synchronised repetitions with the forms alternating in ONE process; median and min .. max.
No ratio is fixed in advance: what is found is reported.

1. The S = 64 session with 16 / 32 / 48 / 64 busy rows, the lowest ones (forced tokens: nobody ends; every slot rewound to 8 generated
   tokens ahead of each repetition): ``step(64) / 64``, elastic against not elastic, and the ratio.
2. ``move`` of 1 / 4 / 16 rows at ~300 positions inside a 64-slot session: the synchronised host time of the call, and the device time
   between two events around it (the table launch and the copy kernel; an upper bound of the copy kernel's own time), with the bytes
   read and written per second that follow from the shapes.
3. The 64 requests of tools/laura_queue.py (lengths 50 .. 750 shuffled, 16 held rows, a look after every step: the decoding loop of
   ``generate_many(prefill=16)``) through 64 and 32 slots, elastic against not: milliseconds (best of 2, alternating), steps, rows
   moved, steps per block count; tokens equal.
4. With ``--parent-tree DIR`` (a checkout of the parent commit with its library built): the S = 16 step, the S = 64 step and -- this
   tree only -- the S = 64 elastic step with every row busy, measured by the same code in processes of their own, PROCS per tree, the
   trees alternating.  Condition per step: this tree's median lies inside the parent's min .. max, or beyond it by no more than the
   parent's own two processes differ (the exit status says so for the first two; the third is reported against the parent's S = 64).

    python tools/laura_elastic.py [--parent-tree DIR] [--out profiles/laura_elastic.txt]
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

REPS, MAXLEN, BACK, STEPS, PROCS, CAP = 24, 750, 8, 64, 2, 1024


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
    m = LauraGenMI355X(spec, "cuda:0", max_positions=CAP)
    m.load_state_dict(make_laura_state_dict(cfg, 0))
    return m, cfg, spec


def texts(m, cfg, n):
    from funcodec_amd.synth import synthetic_text
    lens = [16 + (5 * i) % 11 for i in range(n)]
    outs = []
    with torch.no_grad():
        for g in range(0, n, 16):
            o, _ = m.encode(torch.from_numpy(synthetic_text(cfg, 16, lens[g: g + 16], 11 + g)), torch.tensor(lens[g: g + 16]))
            outs += [o[b, : lens[g + b]] for b in range(16)]
    return outs, lens


def forced_tokens(spec, n):
    rng = np.random.Generator(np.random.PCG64(9))
    return torch.from_numpy(rng.integers(0, spec.codebook_size, size=(n, MAXLEN, spec.predict_nq)).astype(np.int64)).cuda()


def step_times(sessions, reps=REPS):
    """{key: [seconds per step]}: sessions = {key: (session, its busy slots)}, all open together, alternating"""
    t = {k: [] for k in sessions}
    for r in range(reps + 2):                                  # the first two rounds are warm-up
        for k, (s, busy) in sessions.items():
            for b in busy:
                s.rewind(b, BACK, MAXLEN, sampling=False)
            one = timed(lambda: s.step(STEPS)) / STEPS
            if r >= 2:
                t[k].append(one)
    for k, (s, busy) in sessions.items():
        st = s.step(1)
        assert len(st) == len(busy) and all(v == "running" for v in st.values()), "every started slot runs, nobody may have ended"
    return t


def opened(m, S, busy, outs, lens, forced, **kw):
    wide = dict(wide=True) if S > 16 and "wide" in inspect.signature(m.engine.open_decode).parameters else {}
    s = m.engine.open_decode(S, max_positions=CAP, logp=False, **wide, **kw)
    for b in busy:
        s.start(b, outs[b], lens[b], MAXLEN, sampling=False, forced=forced[b])
    s.step(BACK + 8)
    return s


def part_load(m, cfg, spec, say):
    outs, lens = texts(m, cfg, 64)
    forced = forced_tokens(spec, 64)
    say(f" 1. the S = 64 session with the lowest 16 / 32 / 48 / 64 rows busy at {BACK} .. {BACK + STEPS} generated tokens (step({STEPS}) / {STEPS}, "
        f"{REPS} repetitions, the forms alternating in one process)")
    for nbusy in (16, 32, 48, 64):
        busy = list(range(nbusy))
        sess = {"plain": (opened(m, 64, busy, outs, lens, forced), busy), "elastic": (opened(m, 64, busy, outs, lens, forced, elastic=True), busy)}
        t = step_times(sess)
        e = sess["elastic"][0]
        assert e.blocks == nbusy // 16 and e.moves == 0 and sess["plain"][0].blocks == 4
        a, b = statistics.median(t["plain"]), statistics.median(t["elastic"])
        say(f"    {nbusy:2d} busy  not elastic {spread(t['plain'])}   elastic ({e.blocks} blocks) {spread(t['elastic'])}   elastic / not = {b / a:5.3f}")
        for s, _ in sess.values():
            s.free()


def part_move(m, cfg, spec, say):
    outs, lens = texts(m, cfg, 16)
    forced = forced_tokens(spec, 16)
    c = spec.codec_lm
    s = m.engine.open_decode(64, max_positions=CAP, logp=False, wide=True)
    for b in range(16):
        s.start(16 + b, outs[b], lens[b], MAXLEN, sampling=False, forced=forced[b])
    s.step(300 - 26 - 2)                                       # texts of 16 .. 26 tokens: 290 .. 300 positions
    say(" 2. move of k rows of a 64-slot session at ~300 positions (rows 16 .. to rows 40 .. and back; per repetition one call)")
    for k in (1, 4, 16):
        there, back = [(16 + i, 40 + i) for i in range(k)], [(40 + i, 16 + i) for i in range(k)]
        pos = [lens[i] + 2 + 300 - 26 - 2 for i in range(k)]
        nbytes = sum(2 * c.layers * c.d_model * (p + 1) * 4 * 2 for p in pos)
        host, dev = [], []
        for r in range(REPS + 2):
            for pairs in (there, back):
                host_t = timed(lambda: s.move(pairs))
                if r >= 2 and pairs is there:
                    host.append(host_t)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            cur, run = s._run_stream()
            e0.record(run)
            s.move(there)
            e1.record(run)
            torch.cuda.synchronize()
            s.move(back)
            if r >= 2:
                dev.append(e0.elapsed_time(e1) * 1e-3)
        md = statistics.median(dev)
        say(f"    k = {k:2d}   host, synchronised {spread(host)}   device, between events {spread(dev)}   {nbytes} bytes of keys and values "
            f"read and written = {nbytes / md / 1e12:5.2f} TB/s")
    st = s.step(1)
    assert sorted(st) == list(range(16, 32)) and all(v == "running" for v in st.values())
    s.free()


def part_requests(m, cfg, spec, say):
    from funcodec_amd.laura import HeldPrompts, SamplingRules, drive_slots
    N, ROWS = 64, 16
    lengths = [50 + (700 * i) // (N - 1) for i in range(N)]
    np.random.Generator(np.random.PCG64(0)).shuffle(lengths)
    outs, lens = texts(m, cfg, N)
    info = {}

    def loop(S, elastic):
        held = m.engine.open_decode(ROWS, max_positions=CAP, logp=False)
        sess = m.engine.open_decode(S, max_positions=CAP, logp=False, wide=True, **(dict(elastic=True) if elastic else {}))
        plan, steps, hist = HeldPrompts(ROWS, N, 1), [0], {}
        real = sess.step

        def step(n=1):
            steps[0] += n
            st = real(n)
            hist[sess.blocks] = hist.get(sess.blocks, 0) + n
            return st
        sess.step = step

        def start(slot, i):
            todo = plan.need(i)
            if todo:
                held.start_many({row: dict(text_outs=outs[q], text_len=lens[q], max_length=1, sampling=False) for row, q in todo})
            sess.start_from(slot, plan.start(i), lengths[i], sampling=False, rules=SamplingRules(min_length=lengths[i]), source=held)
        res = drive_slots(sess, S, N, start, 1)
        info[(S, elastic)] = (steps[0], sess.moves, dict(sorted(hist.items())))
        sess.free(), held.free()
        return [r[0] for r in res]

    say(f" 3. {N} requests, lengths 50 .. 750 shuffled ({sum(lengths)} tokens), 16 held rows, a look after every step (best of 2, alternating)")
    for S in (64, 32):
        ref = loop(S, False)
        assert [t.shape[0] for t in ref] == lengths
        assert all(torch.equal(a, b) for a, b in zip(loop(S, True), ref)), "tokens differ between the forms"
        best = {False: [], True: []}
        for _ in range(2):
            for el in (False, True):
                best[el].append(timed(lambda: loop(S, el)))
        for el in (False, True):
            steps, moves, hist = info[(S, el)]
            say(f"    {S:2d} slots  {'elastic    ' if el else 'not elastic'}  {min(best[el]) * 1e3:8.1f} ms  {steps:5d} steps  {moves:3d} rows moved  "
                f"steps per block count {hist}   tokens equal")
        say(f"              elastic / not = {min(best[True]) / min(best[False]):5.3f}")


def step_child(name):
    m, cfg, spec = load(name)
    outs, lens = texts(m, cfg, 64)
    forced = forced_tokens(spec, 64)
    own = "elastic" in inspect.signature(m.engine.open_decode).parameters
    sess = {"16": (opened(m, 16, range(16), outs, lens, forced), list(range(16))),
            "64": (opened(m, 64, range(64), outs, lens, forced), list(range(64)))}
    if own:
        sess["64e"] = (opened(m, 64, range(64), outs, lens, forced, elastic=True), list(range(64)))
    t = step_times(sess)
    assert m.engine.persistent_step_fallbacks == 0
    print("LAURA_ELASTIC_JSON " + json.dumps(t), flush=True)


def run_child(name, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--step-child", name] + (["--tree", tree] if tree else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LAURA_ELASTIC_JSON ")), None)
    if r.returncode != 0 or line is None:
        raise RuntimeError(f"the measuring process failed ({r.returncode}):\n{r.stdout[-2000:]}")
    return json.loads(line[len("LAURA_ELASTIC_JSON "):])


def part_parent(name, tree, say):
    owns, pars = [], []
    for _ in range(PROCS):
        pars.append(run_child(name, tree))
        owns.append(run_child(name, None))
    say(f" 4. against the parent commit ({PROCS} processes per tree, the trees alternating, {REPS} repetitions each, pooled; medians per process "
        f"in brackets)")
    meds = lambda runs: " / ".join(f"{statistics.median(r) * 1e6:.1f}" for r in runs)      # noqa: E731
    ok = True
    for key, against, what in (("16", "16", "the S = 16 step"), ("64", "64", "the S = 64 step, not elastic"),
                               ("64e", "64", "the S = 64 step, elastic, every row busy (against the parent's S = 64 step)")):
        own, par = sorted(v for r in owns for v in r[key]), sorted(v for r in pars for v in r[against])
        mo = statistics.median(own)
        gap = abs(statistics.median(pars[0][against]) - statistics.median(pars[1][against]))
        beyond = max(par[0] - mo, mo - par[-1], 0.0)
        fine = beyond <= gap
        say(f"    {what}")
        say(f"      this tree  {spread(own)}  [{meds([r[key] for r in owns])}]")
        say(f"      parent     {spread(par)}  [{meds([r[against] for r in pars])}]   its two processes differ by {gap * 1e6:.1f} us")
        say(f"      this tree's median is {'inside the parent min .. max' if beyond == 0 else f'{beyond * 1e6:.1f} us beyond the parent min .. max'}: "
            f"{'nothing moved' if fine else 'NOT within the condition'}")
        if key != "64e":
            ok = ok and fine
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laura_elastic.txt"))
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

    say(f"tools/laura_elastic.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    ok = True
    for name in ("laura", "lauramusic"):
        m, cfg, spec = load(name)
        s = spec.codec_lm
        say(f"{name}: codec LM {s.layers} layers, d {s.d_model}, {s.heads} heads, ff {s.ff}; above 16 slots the step is the kernel chain at "
            f"every width")
        part_load(m, cfg, spec, say)
        write()
        part_move(m, cfg, spec, say)
        write()
        part_requests(m, cfg, spec, say)
        assert m.engine.persistent_step_fallbacks == 0
        del m
        torch.cuda.empty_cache()
        write()
        if args.parent_tree:
            ok = part_parent(name, args.parent_tree, say) and ok
        else:
            say(" 4. no --parent-tree: the parent's steps were not measured")
        write()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
