"""Time one push of a slot session (funcodec_amd/stream.py StreamSlots) against the two ways to stream S utterances without it.

ss320 and ds320wn at S = 1, 8, 32; 1 and 25 frames per push, encode and decode separately; median of 24 pushes after warm-up, the stream
synchronised around every push.  The slots are deliberately out of phase: in every measured push a third of them START an utterance (with
the start-up length, or the push length if that is longer), the others continue one and one of those ends its utterance (FINAL, one sample
short of whole frames on the encoder side); S = 1 cycles through the three.  The time is that of the wrapper's call for one assembled
push, the assembly of the common-width batch included.  Against it, re-measured in the same run:
  lock-step   one push of CodecStream(batch=S): all rows move together (what the parent offers for a batch)
  S x single  S pushes of CodecStream(batch=1) sessions, one after the other: the only way to the same results without slots
No pass / fail bar.

    python tools/slots_step.py [--out profiles/slots_step.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from funcodec_amd.config import arch_from_config, recipe_config      # noqa: E402
from funcodec_amd.model import EncodecMI355X                          # noqa: E402
from funcodec_amd.stream import FC_SLOT_FINAL, FC_SLOT_START          # noqa: E402
from funcodec_amd.synth import make_state_dict, synthetic_audio       # noqa: E402

PUSHES, WARM = 24, 4


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def roles(S, i):
    """per slot of push i: flags, cycling START -> continue -> continue; the first slot in its second continue also ends"""
    out, ended = [], False
    for b in range(S):
        r = (b + i) % 3
        f = FC_SLOT_START if r == 0 else 0
        if r == 2 and not ended:
            f, ended = FC_SLOT_FINAL, True
        out.append(f)
    return out


def slot_pushes(m, S, nf, decode):
    """median us of a slot push; rows are cut from one long signal per slot"""
    st = m.open_slots(S, max_chunk=max(100, 2 * nf) * m.engine.hop_length)
    hop, nq = m.engine.hop_length, m.arch.num_quantizers
    first = max(st.min_first_frames if decode else st.min_first_samples // hop, nf)
    if decode:
        src = torch.randint(0, m.arch.codebook_size, (S, first, nq), device="cuda")
    else:
        src = torch.from_numpy(synthetic_audio(S, first * hop, 7, "tones")).cuda()

    def rows_of(flags):
        rows = {}
        for b, f in enumerate(flags):
            n = first if f & FC_SLOT_START else nf
            if decode:
                rows[b] = (src[b, :n], f)
            else:
                rows[b] = (src[b:b + 1, :n * hop - (1 if f & FC_SLOT_FINAL else 0)], f)
        return rows
    call = (lambda rows: st._decode_call(rows, True, False)) if decode else (lambda rows: st._encode_call(rows, False))
    call(rows_of([FC_SLOT_START] * S))
    times = []
    for i in range(1, WARM + PUSHES + 1):
        rows = rows_of(roles(S, i))
        times.append(timed(lambda: call(rows)))
    return statistics.median(times[WARM:])


def stream_pushes(m, B, nf, decode, sessions=1):
    """median us of one push of each of `sessions` CodecStream(batch=B) sessions, one after the other"""
    hop, nq = m.engine.hop_length, m.arch.num_quantizers
    sts = [m.open_stream(B) for _ in range(sessions)]
    head = sts[0].min_first_frames if decode else sts[0].min_first_samples // hop
    if decode:
        src = torch.randint(0, m.arch.codebook_size, (B, max(head, nf), nq), device="cuda")
        push = lambda st, n: st.decode(src[:, :n])
    else:
        src = torch.from_numpy(synthetic_audio(B, max(head, nf) * hop, 7, "tones")).cuda()
        push = lambda st, n: st.encode(src[:, :n * hop])
    for st in sts:
        push(st, head)
    times = []
    for i in range(WARM + PUSHES):
        times.append(timed(lambda: [push(st, nf) for st in sts]))
    return statistics.median(times[WARM:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["config   S  frames/push side   | slots us/push | lock-step B=S us/push  ratio | S x single us  ratio (slots / S x single)"]
    for name in ("ss320", "ds320wn"):
        arch = arch_from_config(recipe_config(name))
        m = EncodecMI355X(arch, "cuda:0")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0).items()})
        for S in (1, 8, 32):
            for nf in (1, 25):
                for decode in (False, True):
                    t_slots = slot_pushes(m, S, nf, decode)
                    t_lock = stream_pushes(m, S, nf, decode)
                    t_single = stream_pushes(m, 1, nf, decode, sessions=S)
                    lines.append(f"{name:8s} {S:2d} {nf:6d}      {'decode' if decode else 'encode'} | {t_slots:10.0f}    | {t_lock:10.0f}   {t_slots / t_lock:12.2f} | "
                                 f"{t_single:10.0f}   {t_slots / t_single:8.3f}")
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
