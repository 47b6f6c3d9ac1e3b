"""Time a 1-frame encode push of a slot session without a noise floor and with one (open_slots(noise_floor_db=...); the push rule of
csrc/rvq_rate_kernels.h), in the fused form (one more launch) and in the chain form (four more launches), and report the bytes per
second of packets a slot session writes for the shipped recordings with and without a floor.

ss320, eager slot pushes of 1 frame, S = 1, 8, 32, every slot running.  Warm-up, then the median of 24 pushes (and their min .. max), the
device synchronised around every push; the forms alternate push by push inside one process, clocks as found.  Per cell: us per push.
What is timed is the wrapper's call for one assembled push (StreamSlots._encode_call), as tools/session_graph_step.py times its slot
pushes.  Before a cell is timed the fused and the chain form are asserted torch.equal.
--plain-only [--tree DIR]: the plain push alone, with funcodec_amd imported from DIR: the same measurement on another checkout (the
parent commit), for the comparison that shows the push without a floor unchanged.  No pass / fail bar.

    python tools/push_floor.py [--out profiles/push_floor.txt]
"""
import argparse
import glob
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUSHES, WARM = 24, 6


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def model(name):
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.model import EncodecMI355X
    from funcodec_amd.synth import make_state_dict
    arch = arch_from_config(recipe_config(name))
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0).items()})
    return m


def running_session(m, S, src, **kw):
    """a slot session whose S slots have taken their START push: () -> one steady 1-frame push of every slot"""
    hop = m.engine.hop_length
    st = m.open_slots(S, **kw)
    first = max(st.min_first_samples // hop, st.min_first_frames)
    from funcodec_amd.stream import FC_SLOT_START
    st._encode_call({b: (src[b:b + 1, :first * hop], FC_SLOT_START) for b in range(S)}, False)
    rows = {b: (src[b:b + 1, first * hop:(first + 1) * hop], 0) for b in range(S)}
    return (lambda: st._encode_call(rows, False)), st


def cell(m, S, plain_only):
    hop = m.engine.hop_length
    g = torch.Generator().manual_seed(14)
    src = (0.1 * torch.randn(S, 64 * hop, generator=g)).cuda()
    forms = [running_session(m, S, src)]
    if not plain_only:
        floors = [-30.0 - (b % 4) * 5.0 for b in range(S)]
        forms.append(running_session(m, S, src, noise_floor_db=floors))
        forms.append(running_session(m, S, src, noise_floor_db=floors))
        forms[2][1]._fused = False
        for _ in range(3):
            a, b = forms[1][0](), forms[2][0]()
            assert all(torch.equal(a[s][0], b[s][0]) and torch.equal(a[s][1], b[s][1]) for s in a), "the chain form differs from the fused one"
            assert forms[1][1].last_n_q_rows == forms[2][1].last_n_q_rows
    times = [[] for _ in forms]
    for i in range(WARM + PUSHES):
        for k, (fn, _) in enumerate(forms):
            times[k].append(timed(fn))
    show = lambda t: f"{statistics.median(t[WARM:]):7.0f} ({min(t[WARM:]):5.0f} .. {max(t[WARM:]):5.0f})"
    names = ["plain"] if plain_only else ["plain", "floor fused", "floor chain"]
    line = " | ".join(f"{n} {show(t)}" for n, t in zip(names, times))
    if not plain_only:
        counts = sorted(set(forms[1][1].last_n_q_rows.values()))
        line += f" | fused / plain {statistics.median(times[1][WARM:]) / statistics.median(times[0][WARM:]):5.3f}, chain / plain " \
                f"{statistics.median(times[2][WARM:]) / statistics.median(times[0][WARM:]):5.3f}   [counts {counts}]"
    return line


def packet_rate(m, db):
    """bytes per second of audio of the packets of one slot session fed the shipped recordings in pushes of 20 frames, one per slot"""
    from funcodec_amd.io import read_wav
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "wav", "*.wav")))
    if not paths:
        return None
    hop = m.engine.hop_length
    wavs = [torch.from_numpy(read_wav(p)[0].copy()) for p in paths]
    st = m.open_slots(len(wavs), noise_floor_db=db)
    step, pos, nbytes = 20 * hop, 0, 0
    hist = {}
    while any(pos < len(w) for w in wavs):
        push = {s: (w[pos:pos + step], pos + step >= len(w)) for s, w in enumerate(wavs) if pos < len(w)}
        _, packets = st.encode(push, packed=True)
        nbytes += sum(len(p) for p in packets.values())
        if db is not None:
            for s in packets:
                k = st.last_n_q_rows[s]
                hist[k] = hist.get(k, 0) + 1
        pos += step
    seconds = sum(len(w) for w in wavs) / m.arch.sample_rate
    return nbytes / seconds, len(wavs), seconds, dict(sorted(hist.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    lines = [f"push_floor: ss320 slot session, 1-frame encode pushes, eager; us per push: median of {PUSHES} (min .. max); tree {'parent' if a.plain_only else 'this'}",
             f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}"]
    m = model("ss320")
    for S in (1, 8, 32):
        lines.append(f"S = {S:2d}: " + cell(m, S, a.plain_only))
        print(lines[-1], flush=True)
    if not a.plain_only:
        lines.append("packets of a slot session on the shipped recordings, pushes of 20 frames (the synthetic checkpoint is UNTRAINED: this says what "
                     "the rule does on random codebooks and nothing about trained ones):")
        for db in (None, -20.0, -40.0, -60.0):
            r = packet_rate(m, db)
            if r is None:
                lines.append("  no recordings found")
                break
            lines.append(f"  noise_floor_db {str(db):>6}: {r[0]:9.0f} bytes / s over {r[1]} recordings, {r[2]:.1f} s" + (f"; pushes per count {r[3]}" if db is not None else ""))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
