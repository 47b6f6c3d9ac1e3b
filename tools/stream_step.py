"""Time one streaming push (funcodec_amd/stream.py) against the offline call for the same audio.

ss320 and ds320wn at B = 1, 8, 32; pushes of 1, 5 and 25 frames, encode and decode separately; median of >= 20 pushes after warm-up,
the stream synchronised around every push.  Prints microseconds per push, the launches of one push that the engine's profiler books (staging, conv and RVQ
kernels; one LSTM block counts once; the few layout passes around the quantiser are not booked) and the offline encode / decode of the same total audio.  No pass / fail bar.

    python tools/stream_step.py [--out profiles/stream_step.txt]
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def launches_of(eng, fn):
    eng.set_profiling(True)
    eng.read_profile()
    fn()
    n = sum(p["launches"] for p in eng.read_profile())
    eng.set_profiling(False)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["config   B  frames/push | encode us/push  launches | decode us/push  launches | offline encode / decode us (same total audio)"]
    for name in ("ss320", "ds320wn"):
        arch = arch_from_config(recipe_config(name))
        m = EncodecMI355X(arch, "cuda:0")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 0).items()})
        hop, nq = m.engine.hop_length, arch.num_quantizers
        for B in (1, 8, 32):
            for nf in (1, 5, 25):
                st = m.open_stream(B)
                head = st.min_first_frames
                total = head + nf * (PUSHES + 4)
                wav = torch.from_numpy(synthetic_audio(B, total * hop, 7, "tones")).cuda()
                codes = st.encode(wav[:, :head * hop])[0]
                enc_t, pos = [], head * hop
                enc_l = 0
                parts = [codes]
                for i in range(PUSHES + 4):
                    chunk = wav[:, pos:pos + nf * hop]
                    pos += nf * hop
                    if i == 1:
                        enc_l = launches_of(m.engine, lambda: parts.append(st.encode(chunk)[0]))
                    else:
                        enc_t.append(timed(lambda: parts.append(st.encode(chunk)[0])))
                tok = torch.cat(parts, -1).permute(1, 2, 0).contiguous()
                st.decode(tok[:, :head])
                dec_t, dec_l, pos = [], 0, head
                for i in range(PUSHES + 4):
                    part = tok[:, pos:pos + nf].contiguous()
                    pos += nf
                    if i == 1:
                        dec_l = launches_of(m.engine, lambda: st.decode(part))
                    else:
                        dec_t.append(timed(lambda: st.decode(part)))
                m.engine.encode(wav, nq); m.engine.decode_codes(tok)                                # warm-up
                off_e = statistics.median(timed(lambda: m.engine.encode(wav, nq)) for _ in range(5))
                off_d = statistics.median(timed(lambda: m.engine.decode_codes(tok)) for _ in range(5))
                lines.append(f"{name:8s} {B:2d} {nf:6d}      | {statistics.median(enc_t[3:]):10.0f} {enc_l:10d}    | "
                             f"{statistics.median(dec_t[3:]):10.0f} {dec_l:10d}    | {off_e:8.0f} / {off_d:8.0f}  ({total} frames)")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
