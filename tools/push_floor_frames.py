"""Time an encode push of a slot session under a noise floor per push (open_slots(noise_floor_db=...); the push rule of
csrc/rvq_rate_kernels.h) against the same push under a noise floor per FRAME (per_frame=True; the push frame rule), in its fused form
(one launch, a workgroup per 16 frames of a row) and its chain form (four launches); and report the bytes per second of packets a slot
session writes for the shipped recordings without a floor, with a floor per push and with a floor per frame.

The method of tools/push_floor.py: ss320, eager slot pushes, every slot running.  Warm-up, then the median of 24 pushes (and their
min .. max), the device synchronised around every push; the forms alternate push by push inside one process, clocks as found.  Per cell:
us per push.  What is timed is the wrapper's call for one assembled push (StreamSlots._encode_call).  Cells: 1-frame pushes at
S = 1, 8, 32, and a 100-frame push at S = 1 and S = 8.  Before a cell is timed the fused and the chain form of the frame rule are
asserted torch.equal.
--plain-only [--tree DIR]: the plain 1-frame push alone, with funcodec_amd imported from DIR: the same measurement on another checkout
(the parent commit), for the comparison that shows the push without a floor unchanged.  No pass / fail bar.
The packets: the codebooks are scaled to half the level of the encoder's output (as the tests' _matched_model does: on the synthetic
checkpoint as it is no stage lowers the error and every floor picks min_n_q); the nets are UNTRAINED all the same.

    python tools/push_floor_frames.py [--out profiles/push_floor_frames.txt]
"""
import argparse
import glob
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUSHES, WARM = 24, 6


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def model(name, matched=False):
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.model import EncodecMI355X
    from funcodec_amd.synth import make_state_dict
    arch = arch_from_config(recipe_config(name))
    sd = make_state_dict(arch, 0)

    def load(state):
        m = EncodecMI355X(arch, "cuda:0")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        return m
    m = load(sd)
    if not matched:
        return m
    hop = m.engine.hop_length
    st = m.open_stream(1)
    first = max(st.min_first_samples // hop, st.min_first_frames)
    t = torch.arange((first + 8) * hop, dtype=torch.float32) / arch.sample_rate
    tones = 0.3 * torch.sin(2 * math.pi * 220.0 * t) + 0.2 * torch.sin(2 * math.pi * 1333.0 * t)
    enc = st.encode(tones.view(1, 1, -1), want_enc_out=True)[2]
    e_enc = float(enc.double().pow(2).sum(-1).mean())
    cb = sd["quantizer.rq.model.embed"]
    e_cb = float((cb[0].astype(np.float64) ** 2).sum(-1).mean())
    scaled = dict(sd)
    scaled["quantizer.rq.model.embed"] = (cb * np.float32(0.5 * math.sqrt(e_enc / e_cb))).astype(np.float32)
    level_db = 10.0 * math.log10(e_enc / arch.codebook_dim)        # the encoder output's mean square per element, in dB re 1
    return load(scaled), level_db


def running_session(m, S, src, frames, **kw):
    """a slot session whose S slots have taken their START push: () -> one steady push of `frames` frames of every slot"""
    hop = m.engine.hop_length
    st = m.open_slots(S, **kw)
    first = max(st.min_first_samples // hop, st.min_first_frames)
    from funcodec_amd.stream import FC_SLOT_START
    st._encode_call({b: (src[b:b + 1, :first * hop], FC_SLOT_START) for b in range(S)}, False)
    rows = {b: (src[b:b + 1, first * hop:(first + frames) * hop], 0) for b in range(S)}
    return (lambda: st._encode_call(rows, False)), st


def cell(m, S, frames, plain_only):
    hop = m.engine.hop_length
    g = torch.Generator().manual_seed(14)
    src = (0.1 * torch.randn(S, (64 + frames) * hop, generator=g)).cuda()
    forms = [running_session(m, S, src, frames)]
    if not plain_only:
        floors = [-30.0 - (b % 4) * 5.0 for b in range(S)]
        forms.append(running_session(m, S, src, frames, noise_floor_db=floors))
        forms.append(running_session(m, S, src, frames, noise_floor_db=floors, per_frame=True, min_n_q=0))
        forms.append(running_session(m, S, src, frames, noise_floor_db=floors, per_frame=True, min_n_q=0))
        forms[3][1]._fused = False
        for _ in range(3):
            a, b = forms[2][0](), forms[3][0]()
            assert all(torch.equal(a[s][0], b[s][0]) and torch.equal(a[s][1], b[s][1]) for s in a), "the chain form differs from the fused one"
            ka, kb = forms[2][1].last_n_q_frames, forms[3][1].last_n_q_frames
            assert all(torch.equal(ka[s], kb[s]) for s in ka)
    times = [[] for _ in forms]
    for i in range(WARM + PUSHES):
        for k, (fn, _) in enumerate(forms):
            times[k].append(timed(fn))
    show = lambda t: f"{statistics.median(t[WARM:]):7.0f} ({min(t[WARM:]):5.0f} .. {max(t[WARM:]):5.0f})"
    names = ["plain"] if plain_only else ["plain", "row fused", "frame fused", "frame chain"]
    line = " | ".join(f"{n} {show(t)}" for n, t in zip(names, times))
    if not plain_only:
        med = [statistics.median(t[WARM:]) for t in times]
        line += f" | frame fused - row fused {med[2] - med[1]:+6.0f} us, frame chain - row fused {med[3] - med[1]:+6.0f} us"
    return line


def packet_rate(m, db, per_frame):
    """bytes per second of audio of the packets of one slot session fed the shipped recordings in pushes of 20 frames, one per slot"""
    from funcodec_amd.io import read_wav
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "wav", "*.wav")))
    if not paths:
        return None
    hop = m.engine.hop_length
    wavs = [torch.from_numpy(read_wav(p)[0].copy()) for p in paths]
    st = m.open_slots(len(wavs), noise_floor_db=db, per_frame=per_frame, min_n_q=0 if per_frame else 1)
    step, pos, nbytes = 20 * hop, 0, 0
    hist = {}
    while any(pos < len(w) for w in wavs):
        push = {s: (w[pos:pos + step], pos + step >= len(w)) for s, w in enumerate(wavs) if pos < len(w)}
        _, packets = st.encode(push, packed=True)
        nbytes += sum(len(p) for p in packets.values())
        if db is not None:
            if per_frame:
                ks = [k for v in st.last_n_q_frames.values() for k in v.tolist()]
            else:
                ks = [st.last_n_q_rows[s] for s in packets]
            for k in ks:
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
    lines = [f"push_floor_frames: ss320 slot session, encode pushes, eager; us per push: median of {PUSHES} (min .. max); tree "
             f"{'parent' if a.plain_only else 'this'}", f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}"]
    m = model("ss320")
    cells = [(1, 1), (8, 1), (32, 1)] + ([] if a.plain_only else [(1, 100), (8, 100)])
    for S, frames in cells:
        lines.append(f"S = {S:2d}, {frames:3d} frame(s): " + cell(m, S, frames, a.plain_only))
        print(lines[-1], flush=True)
    if not a.plain_only:
        lines.append("packets of a slot session on the shipped recordings, pushes of 20 frames, codebooks scaled to the encoder's output (the "
                     "synthetic checkpoint is UNTRAINED: this says what the rules do on random codebooks and nothing about trained ones):")
        mm, level = model("ss320", matched=True)
        lines.append(f"  the encoder output's level: {level:.2f} dB re 1 per element; floors are given below it (1024 random codes in 512 dimensions "
                     "lower the error by a fraction of a dB per stage)")
        cases = [(None, False)] + [(level - d, pf) for d in (0.25, 0.5, 1.0, 2.0) for pf in (False, True)]
        for db, per_frame in cases:
            r = packet_rate(mm, db, per_frame)
            if r is None:
                lines.append("  no recordings found")
                break
            what = "no floor" if db is None else f"level {db - level:+5.2f} dB per {'frame' if per_frame else 'push '}"
            lines.append(f"  {what:>26}: {r[0]:9.0f} bytes / s over {r[1]} recordings, {r[2]:.1f} s" +
                         (f"; {'frames' if per_frame else 'pushes'} per count {r[3]}" if db is not None else ""))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
