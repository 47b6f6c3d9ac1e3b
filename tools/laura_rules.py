"""Time a decoding session whose slots carry sampling rules (``DecodeSlots.start(rules=SamplingRules(...))``: temperature, minimum
length, top-k with top-p, the repeat rule -- all inside the sampler, nothing else in the step changes) on the synthetic checkpoints of
the ``laura`` and ``lauramusic`` recipes, by the method of tools/laura_score.py.

One decoding step, ``step(64) / 64``, top-k 25 on forced tokens (nobody ends; every slot rewound to 264 generated tokens ahead of each
repetition, so the context is the same throughout and a window of 256 is full), S = 1 / 8 / 16 slots, three forms alternating:
neutral rules, all rules on with a window of 32, all rules on with a window of 256 (temperature 0.8, <eos> masked throughout, top_p
0.9, repeat_count 1: with forced tokens drawn uniformly a top-25 draw stands in a full window of 256 about once in five steps, so the
second draw is in the figure at that rate).  Warm-up, then 24 synchronised repetitions per process and form; median and min .. max.
With ``--parent-tree DIR`` (a checkout of the parent commit with its library built) the parent's session step is measured by the same
code in the same run, in processes of its own: PROCS processes per tree, the trees alternating, the repetitions of a tree pooled and
the median of every process shown.
Condition (the exit status says so): the step with neutral rules is the parent's step -- its median lies inside the parent's
min .. max, or outside by no more than the medians of the parent's own processes differ in this run.  The cost of the rules is reported
beside it, with no bar.

    python tools/laura_rules.py [--parent-tree DIR] [--out profiles/laura_rules.txt]
"""
import argparse
import datetime
import inspect
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:                                       # a child measuring another checkout: its package, this file's code
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]))
else:
    sys.path.insert(0, ROOT)

REPS, S_ALL, MAXLEN, BACK, STEPS, PROCS, TOPK = 24, (1, 8, 16), 750, 264, 64, 2, 25
FORMS = ("neutral", "all rules, W = 32", "all rules, W = 256")


def timed(fn):
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(v):
    v = sorted(v)
    return f"median {statistics.median(v) * 1e6:8.1f} us (min {v[0] * 1e6:.1f}, max {v[-1] * 1e6:.1f})"


def step_child(name):
    """{"S:form": [seconds per step, REPS of them]} of the package on sys.path, as one JSON line; the parent commit's package has the
    neutral form only (three sessions without rules, alternating all the same)."""
    from funcodec_amd import laura
    from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
    from funcodec_amd.synth import make_laura_state_dict, synthetic_text
    cfg = laura_recipe_config(name)
    spec = laura_spec_from_config(cfg)
    m = laura.LauraGenMI355X(spec, "cuda:0", max_positions=1024)
    m.load_state_dict(make_laura_state_dict(cfg, 0))
    has_rules = "rules" in inspect.signature(laura.DecodeSlots.start).parameters
    if has_rules:
        forms = [None] + [laura.SamplingRules(temperature=0.8, min_length=MAXLEN, top_p=0.9, repeat_window=w, repeat_count=1) for w in (32, 256)]
    else:
        forms = [None, None, None]
    out = {}
    for S in S_ALL:
        lens = [16 + (5 * i) % 11 for i in range(S)]
        with torch.no_grad():
            outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, S, lens, 11)), torch.tensor(lens))
        rng = np.random.Generator(np.random.PCG64(9))
        forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(S, MAXLEN, spec.predict_nq)).astype(np.int64)).cuda()
        sess = []
        for f in forms:
            kw = {"rules": f} if has_rules else {}
            s = m.engine.open_decode(S, max_positions=1024, logp=False)
            for b in range(S):
                s.start(b, outs[b], lens[b], MAXLEN, sampling=TOPK, seed=b, forced=forced[b], **kw)
            s.step(BACK + 8)
            sess.append((s, kw))
        t = [[] for _ in forms]
        for r in range(REPS + 2):                              # the first two rounds are warm-up
            for i, (s, kw) in enumerate(sess):
                for b in range(S):
                    s.rewind(b, BACK, MAXLEN, sampling=TOPK, seed=b, **kw)
                one = timed(lambda: s.step(STEPS)) / STEPS
                if r >= 2:
                    t[i].append(one)
        for s, _ in sess:
            assert all(v == "running" for v in s.step(1).values()), "nobody may have ended"
            s.free()
        if has_rules:
            for f, v in zip(FORMS, t):
                out[f"{S}:{f}"] = v
        else:
            out[f"{S}:{FORMS[0]}"] = t[0] + t[1] + t[2]
    assert m.engine.persistent_step_fallbacks == 0
    print("LAURA_RULES_JSON " + json.dumps(out), flush=True)


def run_child(name, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--step-child", name] + (["--tree", tree] if tree else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LAURA_RULES_JSON ")), None)
    if r.returncode != 0 or line is None:
        raise RuntimeError(f"the measuring process failed ({r.returncode}):\n{r.stdout[-2000:]}")
    print(f"  .. {name}: a process of {'the parent tree' if tree else 'this tree'} has measured", file=sys.stderr, flush=True)
    return json.loads(line[len("LAURA_RULES_JSON "):])


def measure(name, parent_tree, say):
    owns, pars = [], []
    for _ in range(PROCS if parent_tree else 1):
        if parent_tree:
            pars.append(run_child(name, parent_tree))
        owns.append(run_child(name, None))

    def pooled(runs):
        return {k: [v for r in runs for v in r[k]] for k in runs[0]} if runs else None

    def per_process(runs, key):
        return " / ".join(f"{statistics.median(r[key]) * 1e6:.1f}" for r in runs)
    own, par = pooled(owns), pooled(pars)
    ok = True
    say(f"  step({STEPS}) / {STEPS}, top-k {TOPK} on forced tokens, every slot at {BACK} .. {BACK + STEPS} generated tokens, {REPS} repetitions per "
        f"process and form, forms alternating" + (f"; {PROCS} processes per tree, the trees alternating, pooled (medians per process in "
                                                   f"brackets)" if par else ";  no --parent-tree: the parent's step was not measured"))
    for S in S_ALL:
        neutral = own[f"{S}:{FORMS[0]}"]
        mn = statistics.median(neutral)
        for f in FORMS:
            v = own[f"{S}:{f}"]
            cost = "" if f == FORMS[0] else f"  {(statistics.median(v) - mn) * 1e6:+.1f} us ({(statistics.median(v) / mn - 1) * 100:+.2f} %) on neutral"
            say(f"      S = {S:2d}, {f:19s} {spread(v)}  [{per_process(owns, f'{S}:{f}')}]{cost}")
        if par:
            pv = sorted(par[f"{S}:{FORMS[0]}"])
            meds = [statistics.median(r[f"{S}:{FORMS[0]}"]) for r in pars]
            between = max(meds) - min(meds)
            out_by = max(pv[0] - mn, mn - pv[-1], 0.0)
            good = out_by <= between
            ok = ok and good
            say(f"      {'':27s} parent {spread(pv)}  [{per_process(pars, f'{S}:{FORMS[0]}')}]  ({len(pv)} repetitions; its processes differ by "
                f"{between * 1e6:.1f} us)")
            say(f"      {'':27s} neutral - parent = {(mn - statistics.median(pv)) * 1e6:+.1f} us;  neutral inside the parent's min .. max: "
                f"{'yes' if out_by == 0.0 else f'no, outside by {out_by * 1e6:.1f} us'};  condition {'met' if good else 'NOT met'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laura_rules.txt"))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: its session step, the yardstick")
    ap.add_argument("--only", default=None, help="laura | lauramusic: that recipe alone")
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

    say(f"tools/laura_rules.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    ok = True
    for name in ("laura", "lauramusic"):
        if args.only not in (None, name):
            continue
        from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
        s = laura_spec_from_config(laura_recipe_config(name)).codec_lm
        say(f"{name}: codec LM {s.layers} layers, d {s.d_model}, {s.heads} heads, ff {s.ff}")
        ok = measure(name, args.parent_tree, say) and ok
    say(f"condition (neutral rules = the parent's step): {'met' if ok else 'NOT met'}" if args.parent_tree else "condition not checked: no --parent-tree")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
