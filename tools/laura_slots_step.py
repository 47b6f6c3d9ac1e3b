"""Time a decoding session of the LauraTTS engine (``LauraEngine.open_decode``) against ``decode_codec`` on the same build, on the
synthetic checkpoints of the ``laura`` and ``lauramusic`` recipes.  No pass / fail bar.

1. One session step at S = 1, 8, 16 with every slot running, against the step of decode_codec at B = S.  Forced tokens (no row ends
   early).  decode_codec's step is the difference of two call lengths per step, so the prefix pass and the call's fixed costs cancel;
   the session's is ``step(n)`` / n with n = the same difference, and ``step(1)`` (one status read-back per step, what generate_many
   does).  Median of 24 synchronised repetitions, the forms alternating.
2. 64 requests whose lengths are spread over 50 .. 750 in shuffled order (forced tokens, then a forced <eos>), through 16 slots kept
   full (``drive_slots``, a look after every step), against four decode_codec calls of 16 rows in arrival order: total time, steps
   run, and the cost of a ``start`` in the middle of a generation (prefix pass and first sample, synchronised around it, 15 other
   slots running).

    python tools/laura_slots_step.py [--out profiles/laura_slots_step.txt]
"""
import argparse
import datetime
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from funcodec_amd.laura import LauraGenMI355X, drive_slots                          # noqa: E402
from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config   # noqa: E402
from funcodec_amd.synth import make_laura_state_dict, synthetic_text                # noqa: E402

REPS, SHORT, LONG = 24, 8, 72


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def med_us(v):
    return statistics.median(v) * 1e6


def step_costs(m, cfg, spec, S, say):
    lens = [16 + (5 * i) % 11 for i in range(S)]
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, S, lens, 3)), torch.tensor(lens))
    rng = np.random.Generator(np.random.PCG64(S))
    M = LONG + 2 * (LONG - SHORT)
    forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(S, M, spec.predict_nq)).astype(np.int64)).cuda()
    sess = m.engine.open_decode(S, max_positions=256, logp=False)
    n = LONG - SHORT

    def call(k):
        return timed(lambda: m.engine.decode_codec(outs, lens, k, sampling=False, forced=forced[:, :k]))

    def restart():
        for b in range(S):
            sess.start(b, outs[b], lens[b], M, sampling=False, forced=forced[b])
        sess.step(SHORT)                                   # the positions decode_codec's difference covers

    call(SHORT), call(LONG), restart(), sess.step(2)      # warm-up (graphs, workspaces)
    ref, many, single = [], [], []
    for _ in range(REPS):
        ref.append((call(LONG) - call(SHORT)) / n)
        restart()
        many.append(timed(lambda: sess.step(n)) / n)
        restart()
        t = timed(lambda: [sess.step(1) for _ in range(n)])
        single.append(t / n)
    sess.free()
    ref.sort()
    say(f"  S = B = {S:2d}   decode_codec step {med_us(ref):7.1f} us (min {ref[0] * 1e6:.1f}, max {ref[-1] * 1e6:.1f})   "
        f"session step(n) / n {med_us(many):7.1f} us   session step(1) {med_us(single):7.1f} us")


def requests(m, cfg, spec, say):
    N, S = 64, 16
    K, nq = spec.codebook_size, spec.predict_nq
    lengths = [50 + (700 * i) // (N - 1) for i in range(N)]
    np.random.Generator(np.random.PCG64(0)).shuffle(lengths)
    lens = [16 + (5 * i) % 11 for i in range(N)]
    rng = np.random.Generator(np.random.PCG64(9))
    forced = rng.integers(0, K, size=(N, 750, nq)).astype(np.int64)
    for i, n in enumerate(lengths):
        if n < 750:
            forced[i, n:] = K                              # a forced <eos>: the row ends after n tokens
    forced = torch.from_numpy(forced).cuda()
    outs = []
    with torch.no_grad():
        for g in range(0, N, S):
            o, _ = m.encode(torch.from_numpy(synthetic_text(cfg, S, lens[g: g + S], 11 + g)), torch.tensor(lens[g: g + S]))
            outs.append(o)

    def lock_step():
        got = []
        for k, g in enumerate(range(0, N, S)):
            _, ol = m.engine.decode_codec(outs[k], lens[g: g + S], 750, sampling=False, forced=forced[g: g + S])
            got += ol
        return got

    steps = [0]

    def session():
        sess = m.engine.open_decode(S, max_positions=1024, logp=False)
        real_step = sess.step

        def counting(n=1):
            st = real_step(n)
            steps[0] += n
            return st
        sess.step = counting
        steps[0] = 0
        res = drive_slots(sess, S, N, lambda slot, i: sess.start(slot, outs[i // S][i % S], lens[i], 750, sampling=False, forced=forced[i]))
        sess.free()
        return [r[1] for r in res]

    a, b = lock_step(), session()                          # warm-up, and the same lengths both ways
    assert a == b == [min(n, 750) for n in lengths], (a[:4], b[:4], lengths[:4])
    t_lock = min(timed(lock_step) for _ in range(2))
    t_sess = min(timed(session) for _ in range(2))
    lock_steps = 0
    for g in range(0, N, S):                               # do_decode's loop: all rows ended? after every 16th sample
        longest, s = max(lengths[g: g + S]), 1
        while s < 750:
            lock_steps += 1
            if (s & 15) == 15 and s + 1 < 750 and longest + 1 <= s + 1:
                break
            s += 1
    say(f"  64 requests, lengths 50 .. 750 shuffled, 16 rows: four decode_codec calls {t_lock * 1e3:8.1f} ms ({lock_steps} steps)   "
        f"session, slots kept full {t_sess * 1e3:8.1f} ms ({steps[0]} steps)")
    # a start in the middle of a generation: 15 slots running
    sess = m.engine.open_decode(S, max_positions=1024, logp=False)
    for b in range(S - 1):
        sess.start(b, outs[0][b], lens[b], 750, sampling=False, forced=forced[b])
    sess.step(32)
    cost = []
    for r in range(9):
        i = S - 1 + r
        cost.append(timed(lambda: sess.start(S - 1, outs[i // S][i % S], lens[i], 750, sampling=False, forced=forced[i])))
        sess.step(4)
    sess.free()
    say(f"  start with 15 slots running (text of {min(lens)} .. {max(lens)} tokens): median {med_us(cost[1:]):7.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laura_slots_step.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/laura_slots_step.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    for name in ("laura", "lauramusic"):
        cfg = laura_recipe_config(name)
        spec = laura_spec_from_config(cfg)
        m = LauraGenMI355X(spec, "cuda:0", max_positions=1024)
        m.load_state_dict(make_laura_state_dict(cfg, 0))
        s = spec.codec_lm
        say(f"{name}: codec LM {s.layers} layers, d {s.d_model}, {s.heads} heads, ff {s.ff}; persistent step "
            f"{'available' if m.engine.set_persistent_step(True) else 'not available'} (per S: where its LDS fits)")
        say(f" 1. one step, every slot running (median of {REPS}, forms alternating; decode_codec: ({LONG} - {SHORT}-step calls) / {LONG - SHORT})")
        for S in (1, 8, 16):
            step_costs(m, cfg, spec, S, say)
        say(" 2. requests through slots kept full")
        requests(m, cfg, spec, say)
        assert m.engine.persistent_step_fallbacks == 0
        del m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
