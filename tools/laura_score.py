"""Time a decoding session that scores its steps (``open_decode(score=True)``: the sampler keeps the log-probability of every step's
picks) on the synthetic checkpoints of the ``laura`` and ``lauramusic`` recipes.

(a) One decoding step, ``step(64) / 64``, of a session with scores against the same session without: S = 1 / 8 / 16 slots on forced
    tokens (nobody ends; every slot rewound to 8 tokens ahead of each repetition, so the context is the same throughout), greedy and
    top-k 25 separately (greedy gains an exp pass per group that it did not have).  Warm-up, then synchronised repetitions, the forms
    alternating; median and min .. max.  With ``--parent-tree DIR`` (a checkout of the parent commit with its library built) the
    parent's session step is measured by the same code in the same run, in processes of its own (one library per process): PROCS
    processes per tree, the trees alternating, the repetitions of a tree pooled and the median of every process shown, so that the
    spread from one process to the next is on the page beside the spread inside one.
    Condition: the step without scores lies inside the parent's min .. max (reported, and the exit status says so).
(b) 16 requests x 4 samples through 16 slots with ``Text2Audio.generate_many(samples=4)``, max_length 100: keep="best" against
    keep="all", equal tokens first, then total time, and of the keep="all" call the part spent in the fine predictor and the codec
    decoder (``Text2Audio._synthesise``, synchronised).  keep="best" runs that part on 16 of 64 candidates: the saving to expect is 3/4
    of it, and nothing on the decoding steps.  No bar.

    python tools/laura_score.py [--parent-tree DIR] [--out profiles/laura_score.txt]
"""
import argparse
import datetime
import inspect
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.dirname(os.path.abspath(__file__))
if "--tree" in sys.argv:                                       # a child measuring another checkout: its package, this file's code
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]))
else:
    sys.path.insert(0, ROOT)
    sys.path.insert(1, TOOLS)

REPS, S_ALL, MAXLEN, BACK, STEPS, PROCS = 24, (1, 8, 16), 750, 8, 64, 2
MODES = (("greedy", False), ("top-k 25", 25))


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
    """{"S:mode:form": [seconds per step, REPS of them]} of the package on sys.path, as one JSON line; forms: the session without
    scores and, where open_decode has them, with."""
    from funcodec_amd.laura import LauraGenMI355X
    from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
    from funcodec_amd.synth import make_laura_state_dict, synthetic_text
    cfg = laura_recipe_config(name)
    spec = laura_spec_from_config(cfg)
    m = LauraGenMI355X(spec, "cuda:0", max_positions=1024)
    m.load_state_dict(make_laura_state_dict(cfg, 0))
    has_score = "score" in inspect.signature(m.engine.open_decode).parameters
    forms = (False, True) if has_score else (False, False)     # the parent: two sessions without scores, alternating all the same
    out = {}
    for S in S_ALL:
        lens = [16 + (5 * i) % 11 for i in range(S)]
        with torch.no_grad():
            outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, S, lens, 11)), torch.tensor(lens))
        rng = np.random.Generator(np.random.PCG64(9))
        forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(S, MAXLEN, spec.predict_nq)).astype(np.int64)).cuda()
        for mode, sampling in MODES:
            sess = []
            for f in forms:
                s = m.engine.open_decode(S, max_positions=1024, logp=False, score=True) if f else m.engine.open_decode(S, max_positions=1024, logp=False)
                for b in range(S):
                    s.start(b, outs[b], lens[b], MAXLEN, sampling=sampling, seed=b, forced=forced[b])
                s.step(BACK + 8)
                sess.append(s)
            t = [[], []]
            for r in range(REPS + 2):                          # the first two rounds are warm-up
                for i, s in enumerate(sess):
                    for b in range(S):
                        s.rewind(b, BACK, MAXLEN, sampling=sampling, seed=b)
                    one = timed(lambda: s.step(STEPS)) / STEPS
                    if r >= 2:
                        t[i].append(one)
            for i, s in enumerate(sess):
                assert all(v == "running" for v in s.step(1).values()), "nobody may have ended"
                s.free()
            out[f"{S}:{mode}:plain"] = t[0] if has_score else t[0] + t[1]
            if has_score:
                out[f"{S}:{mode}:score"] = t[1]
    assert m.engine.persistent_step_fallbacks == 0
    print("LAURA_SCORE_JSON " + json.dumps(out), flush=True)


def run_child(name, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--step-child", name] + (["--tree", tree] if tree else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LAURA_SCORE_JSON ")), None)
    if r.returncode != 0 or line is None:
        raise RuntimeError(f"the measuring process failed ({r.returncode}):\n{r.stdout[-2000:]}")
    return json.loads(line[len("LAURA_SCORE_JSON "):])


def part_a(name, parent_tree, say):
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
    say(f"  (a) step({STEPS}) / {STEPS}, forced tokens, every slot at {BACK} .. {BACK + STEPS} generated tokens, {REPS} repetitions per "
        f"process and form, forms alternating" + (f"; {PROCS} processes per tree, the trees alternating, pooled (medians per process in "
                                                   f"brackets)" if par else ";  no --parent-tree: the parent's step was not measured"))
    for S in S_ALL:
        for mode, _ in MODES:
            plain, score = own[f"{S}:{mode}:plain"], own[f"{S}:{mode}:score"]
            say(f"      S = {S:2d}, {mode:8s}  score=False {spread(plain)}  [{per_process(owns, f'{S}:{mode}:plain')}]")
            say(f"      {'':19s} score=True  {spread(score)}  [{per_process(owns, f'{S}:{mode}:score')}]")
            mp, ms = statistics.median(plain), statistics.median(score)
            line = f"      {'':19s} score=True - score=False = {(ms - mp) * 1e6:+.1f} us ({(ms / mp - 1) * 100:+.2f} %)"
            if par:
                pv = sorted(par[f"{S}:{mode}:plain"])
                inside = pv[0] <= mp <= pv[-1]
                ok = ok and inside
                say(f"      {'':19s} parent      {spread(pv)}  [{per_process(pars, f'{S}:{mode}:plain')}]  ({len(pv)} repetitions)")
                line += (f";  score=False inside the parent's min .. max: {'yes' if inside else 'NO'};  score=True "
                         f"{'inside it too' if pv[0] <= ms <= pv[-1] else f'{(ms - pv[-1]) * 1e6:+.1f} us from its max' if ms > pv[-1] else 'below its min'}")
            say(line)
    return ok


def part_b(name, say):
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
    from funcodec_amd.synth import make_freq_state_dict, make_laura_state_dict, make_state_dict, synthetic_text_embedder, write_checkpoint
    from laura_start_from import CODEC
    cfg = laura_recipe_config(name)
    spec = laura_spec_from_config(cfg)
    ccfg = recipe_config(CODEC[name])
    csd = make_freq_state_dict(ccfg, 0) if CODEC[name].startswith("freq") else make_state_dict(arch_from_config(ccfg), 0)
    lsd = make_laura_state_dict(cfg, 0)
    lsd["quantizer_codebook.embed"] = csd["quantizer.rq.model.embed"][: spec.num_quantizers].copy()
    tmp = tempfile.mkdtemp(prefix="laura_score_")
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
    syn = [0.0, 0]
    inner = t2a._synthesise

    def synthesise(text_outs, lens, *a):
        out = [None]

        def run():
            out[0] = inner(text_outs, lens, *a)
        syn[0] += timed(run)
        syn[1] += len(lens)
        return out[0]
    t2a._synthesise = synthesise

    def call(keep):
        syn[0], syn[1] = 0.0, 0
        return t2a.generate_many(texts, slots=16, seeds=seeds, samples=N, keep=keep)
    every, best = call("all"), call("best")                    # warm-up, and the same tokens both ways
    for i in range(n):
        k = best[2][i][0]
        assert torch.equal(best[1][i], every[1][i][k]), i
    t_all, t_best, s_all, s_best = [], [], [], []
    for _ in range(3):
        t_all.append(timed(lambda: call("all")))
        s_all.append(syn[0])
        assert syn[1] == n * N
        t_best.append(timed(lambda: call("best")))
        s_best.append(syn[0])
        assert syn[1] == n
    ta, tb, sa, sb = (statistics.median(v) * 1e3 for v in (t_all, t_best, s_all, s_best))
    ends = sum(1 for i in range(n) for k in range(N) if every[1][i][k].shape[1] < 100)
    say(f"  (b) 16 requests x 4 samples, 16 slots, max_length 100 ({ends} of 64 candidates end on <eos>), tokens equal; generate_many in all "
        f"(median of 3, alternating)")
    say(f"      keep=\"all\"   {ta:8.1f} ms, of it fine predictor + codec decoder on 64 candidates {sa:8.1f} ms")
    say(f"      keep=\"best\"  {tb:8.1f} ms, of it fine predictor + codec decoder on 16 candidates {sb:8.1f} ms")
    say(f"      expected from the keep=\"all\" call: {ta:.1f} - 3/4 x {sa:.1f} = {ta - 0.75 * sa:.1f} ms;  found {tb:.1f} ms "
        f"({tb - (ta - 0.75 * sa):+.1f} ms);  saved {ta - tb:.1f} ms = {(1 - tb / ta) * 100:.1f} % of the call")
    del t2a
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laura_score.txt"))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: its session step, for scale")
    ap.add_argument("--only", default=None, help="a | b: that part alone")
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

    say(f"tools/laura_score.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    ok = True
    for name in ("laura", "lauramusic"):
        from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
        s = laura_spec_from_config(laura_recipe_config(name)).codec_lm
        say(f"{name}: codec LM {s.layers} layers, d {s.d_model}, {s.heads} heads, ff {s.ff}")
        if args.only in (None, "a"):
            ok = part_a(name, args.parent_tree, say) and ok
        if args.only in (None, "b"):
            part_b(name, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
