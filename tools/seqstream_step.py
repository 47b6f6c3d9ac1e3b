"""Time one streaming push of a causal transformer net (ss320tfc, a session opened with max_frames) as its key / value cache fills.

ss320tfc, 1 frame per push, B = 1, 8, 32, with 7, 500 and 1500 frames in the cache; encode and decode separately; median of 24 pushes
after warm-up, the stream synchronised around every push.  Beside it, from the same run: a push of ss320 (the same net without a
sequence model: the difference is the price of the bottleneck) and the offline encode of the whole prefix of that length (the only way
to these frames without a cache).  The engine's profiler gives the time of the cached-attention launches of a push (both blocks, the
partial and the merge launch, event-timed) and the sum over all booked kernels of the push.  No pass / fail bar.

    python tools/seqstream_step.py [--out profiles/seqstream_step.txt]
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
from funcodec_amd.synth import make_state_dict, synthetic_audio       # noqa: E402

PUSHES = 24
WARM = 4
PROFILED = 4
FILLS = (7, 500, 1500)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def profiled(eng, fns):
    """(us in the cached-attention launches, us in all booked kernels) per push, over the pushes `fns`"""
    eng.set_profiling(True)
    eng.read_profile()
    for fn in fns:
        fn()
    prof = eng.read_profile()
    eng.set_profiling(False)
    attn = sum(p["total_ms"] for p in prof if p["kernel"].startswith("seq_attn_cached_kernel"))
    return attn * 1e3 / len(fns), sum(p["total_ms"] for p in prof) * 1e3 / len(fns)


def model(name):
    arch = arch_from_config(recipe_config(name))
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0).items()})
    return m


def side(eng, push, chunks):
    """median us of PUSHES pushes after WARM warm-up pushes, then the profile of PROFILED more"""
    for c in chunks[:WARM]:
        push(c)
    t = [timed(lambda c=c: push(c)) for c in chunks[WARM:WARM + PUSHES]]
    attn, booked = profiled(eng, [lambda c=c: push(c) for c in chunks[WARM + PUSHES:]])
    return statistics.median(t), attn, booked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tf, plain = model("ss320tfc"), model("ss320")
    hop, nq = tf.engine.hop_length, tf.arch.num_quantizers
    n = WARM + PUSHES + PROFILED
    lines = ["ss320tfc, 1 frame per push: us/push (median of 24) | us of the push in the cached-attention launches (events) / in all booked kernels",
             " B  cached | encode us  attention / booked | decode us  attention / booked | ss320 push encode / decode us | offline encode of the prefix us"]
    for B in (1, 8, 32):
        ps = plain.open_stream(B)
        head = max(ps.min_first_frames, ps.min_first_samples // hop)
        wav = torch.from_numpy(synthetic_audio(B, (head + 2 * n) * hop, 7, "tones")).cuda()
        codes = [ps.encode(wav[:, :head * hop])[0]]
        pe = [timed(lambda i=i: codes.append(ps.encode(wav[:, (head + i) * hop:(head + i + 1) * hop])[0])) for i in range(n)]
        tok = torch.cat(codes, -1).permute(1, 2, 0).contiguous()
        ps.decode(tok[:, :head])
        pd = [timed(lambda i=i: ps.decode(tok[:, head + i:head + i + 1].contiguous())) for i in range(n)]
        plain_e, plain_d = statistics.median(pe[WARM:]), statistics.median(pd[WARM:])
        for fill in FILLS:
            st = tf.open_stream(B, max_frames=fill + n)
            wav = torch.from_numpy(synthetic_audio(B, (fill + n) * hop, 7, "tones")).cuda()
            parts = [st.encode(wav[:, :fill * hop])[0]]            # the cache holds `fill` frames from here on
            chunks = [wav[:, (fill + i) * hop:(fill + i + 1) * hop] for i in range(n)]
            e_us, e_attn, e_all = side(tf.engine, lambda c: parts.append(st.encode(c)[0]), chunks)
            tok = torch.cat(parts, -1).permute(1, 2, 0).contiguous()
            st.decode(tok[:, :fill])
            d_us, d_attn, d_all = side(tf.engine, lambda c: st.decode(c), [tok[:, fill + i:fill + i + 1].contiguous() for i in range(n)])
            prefix = wav[:, :(fill + 1) * hop].contiguous()
            tf.engine.encode(prefix, nq)                              # warm-up
            off = statistics.median(timed(lambda: tf.engine.encode(prefix, nq)) for _ in range(5))
            lines.append(f"{B:2d} {fill:7d} | {e_us:9.0f} {e_attn:10.1f} / {e_all:6.0f} | {d_us:9.0f} {d_attn:10.1f} / {d_all:6.0f} | "
                         f"{plain_e:8.0f} / {plain_d:8.0f}      | {off:10.0f}  ({fill + 1} frames)")
            print(lines[-1], flush=True)
            del st
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
