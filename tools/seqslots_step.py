"""Time one push of a slot session of a causal transformer net (``open_slots(S, max_frames=N)``) against the two ways to stream S
utterances of such a net without it.

ss320tfc, 1 frame per push, S = 1, 8, 32; encode and decode separately; median of 24 pushes after warm-up, the stream synchronised
around every push.  The slots are out of phase as in tools/slots_step.py, with one difference that the key / value cache forces: a
START puts a slot back to position 0, so the roles do not rotate.  Every third slot STARTs an utterance in every measured push (the
start-up length at position 0; the first of them also ends it, START | FINAL), the others continue theirs with one frame at cached
positions spread evenly between 7 and 1500, one frame further with every push.  S = 1 is one running slot at 1500.  The time is that of
the wrapper's call for one assembled push, the assembly of the common-width batch included.  Against it, from the same run:
  lock-step   one push of CodecStream(batch=S, max_frames): every row at the LARGEST of those positions (the code of the parent commit)
  S x single  one push of each of S CodecStream(batch=1, max_frames) sessions at the slots' own positions, one after the other: the
              only way to these results without slots
and the engine's event time of the cached-attention launches of a push (both blocks; append not included).  No pass / fail bar.

    python tools/seqslots_step.py [--out profiles/seqslots_step.txt]
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

PUSHES, WARM, PROFILED = 24, 4, 4
LOW, HIGH = 7, 1500
BOUND = HIGH + WARM + PUSHES + PROFILED + 8


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def measure(eng, push, prefix):
    """(median us of PUSHES pushes after WARM, us per push in the cached-attention launches over PROFILED more)"""
    for _ in range(WARM):
        push()
    t = statistics.median(timed(push) for _ in range(PUSHES))
    eng.set_profiling(True)
    eng.read_profile()
    for _ in range(PROFILED):
        push()
    prof = eng.read_profile()
    eng.set_profiling(False)
    return t, sum(p["total_ms"] for p in prof if p["kernel"].startswith(prefix)) * 1e3 / PROFILED


def positions(S):
    """(the slots that START in every push, the cached position of every other slot)"""
    if S == 1:
        return [], {0: HIGH}
    run = [b for b in range(S) if b % 3]
    return [b for b in range(S) if b % 3 == 0], {b: LOW + (HIGH - LOW) * i // (len(run) - 1) for i, b in enumerate(run)}


def slot_pushes(m, S, decode):
    st = m.open_slots(S, max_frames=BOUND)
    hop, nq = m.engine.hop_length, m.arch.num_quantizers
    first = st.min_first_frames if decode else st.min_first_samples // hop
    starts, pos = positions(S)
    if decode:
        src = torch.randint(0, m.arch.codebook_size, (S, HIGH, nq), device="cuda")
        st.decode({b: src[b, :p] for b, p in pos.items()})             # the caches of the running slots hold their positions from here on
    else:
        src = torch.from_numpy(synthetic_audio(S, HIGH * hop, 7, "tones")).cuda()
        st.encode({b: src[b:b + 1, :p * hop] for b, p in pos.items()})
    rows = {}
    for b in range(S):
        f = (FC_SLOT_START | (FC_SLOT_FINAL if b == starts[0] else 0)) if b in starts else 0
        n = (first + (1 if f & FC_SLOT_FINAL else 0)) if b in starts else 1      # the ending one: one sample short of whole frames (encode)
        rows[b] = (src[b, :n], f) if decode else (src[b:b + 1, :n * hop - (1 if f & FC_SLOT_FINAL else 0)], f)
    call = (lambda: st._decode_call(rows, True, False)) if decode else (lambda: st._encode_call(rows, False))
    return measure(m.engine, call, "seq_attn_rows_kernel")


def stream_pushes(m, rows_pos, decode):
    """one push of each CodecStream(batch=len(p)) session of rows_pos (a list of per-session position lists, equal within a session)"""
    hop, nq = m.engine.hop_length, m.arch.num_quantizers
    sts = []
    for p in rows_pos:
        st = m.open_stream(len(p), max_frames=BOUND)
        if decode:
            src = torch.randint(0, m.arch.codebook_size, (len(p), p[0] + 1, nq), device="cuda")
            st.decode(src[:, :p[0]])
            sts.append((st, src[:, p[0]:].contiguous()))
        else:
            src = torch.from_numpy(synthetic_audio(len(p), (p[0] + 1) * hop, 7, "tones")).cuda()
            st.encode(src[:, :p[0] * hop])
            sts.append((st, src[:, p[0] * hop:].contiguous()))
    push = (lambda: [st.decode(x) for st, x in sts]) if decode else (lambda: [st.encode(x) for st, x in sts])
    return measure(m.engine, push, "seq_attn_cached_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    arch = arch_from_config(recipe_config("ss320tfc"))
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0).items()})
    lines = [f"measured {time.strftime('%Y-%m-%d')}",
             "ss320tfc, 1 frame per push: us/push (median of 24) and us of the push in the cached-attention launches (events)",
             " S side   | (a) slots  attention | (b) lock-step B=S at 1500  attention   a / b | (c) S x single  attention   a / c"]
    for S in (1, 8, 32):
        starts, pos = positions(S)
        own = [pos.get(b, LOW) for b in range(S)]              # a starting slot's single session: the shortest position a stream can stand at
        for decode in (False, True):
            a, a_at = slot_pushes(m, S, decode)
            b, b_at = stream_pushes(m, [[HIGH] * S], decode)
            c, c_at = stream_pushes(m, [[p] for p in own], decode)
            lines.append(f"{S:2d} {'decode' if decode else 'encode'} | {a:9.0f} {a_at:10.1f} | {b:14.0f} {b_at:21.1f} {a / b:7.2f} | {c:14.0f} {c_at:10.1f} {a / c:7.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
