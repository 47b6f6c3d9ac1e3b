"""Per-step time of the text-to-music LauraTTS decoding step (config ``lauramusic``: 12 layers, d 1024, 16 heads, ff 4096) on cuda:0.

    python tools/laura_music_step.py [--reps 5] [--json out.json]

Times teacher-forced greedy decode calls of two lengths (forced tokens: no utterance stops early) and reports the difference per
step, so the prefix pass and the call's fixed costs cancel.  Forms: the kernel chain at B = 1, 8, 16 and the persistent step at
B = 1, 2 (the batches whose step fits its LDS at d = 1024).  The HBM floor is the codec-LM weights one step streams,
12 x (4 d^2 + 2 d ff) x 4 B plus the output layer, at 8 TB/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from funcodec_amd.laura import LauraGenMI355X  # noqa: E402
from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config  # noqa: E402
from funcodec_amd.synth import make_laura_state_dict, synthetic_text  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--long", type=int, default=72)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cfg = laura_recipe_config("lauramusic")
    spec = laura_spec_from_config(cfg)
    s = spec.codec_lm
    weight_bytes = s.layers * (4 * s.d_model ** 2 + 2 * s.d_model * s.ff) * 4 + s.d_model * spec.lm_vocab * 4
    floor_us = weight_bytes / HBM_BYTES_PER_S * 1e6
    m = LauraGenMI355X(spec, "cuda:0", max_positions=256)
    m.load_state_dict(make_laura_state_dict(cfg, 0))
    rows = []
    for form, B in (("chain", 1), ("chain", 8), ("chain", 16), ("persistent", 1), ("persistent", 2)):
        on = m.engine.set_persistent_step(form == "persistent")
        assert on == (form == "persistent"), (form, on)
        lens = [16 + (5 * i) % 11 for i in range(B)]
        with torch.no_grad():
            outs, _ = m.encode(torch.from_numpy(synthetic_text(cfg, B, lens, 3)), torch.tensor(lens))
        rng = np.random.Generator(np.random.PCG64(B))
        forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(B, args.long, spec.predict_nq)).astype(np.int64))

        def run(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.engine.decode_codec(outs, lens, n, sampling=False, forced=forced[:, :n])
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        run(args.short), run(args.long)                       # warm-up (graphs, workspaces)
        per = sorted((run(args.long) - run(args.short)) / (args.long - args.short) for _ in range(args.reps))
        us = per[len(per) // 2] * 1e6
        row = dict(form=form, B=B, step_us=round(us, 1), hbm_floor_us=round(floor_us, 1), floor_fraction=round(floor_us / us, 3),
                   spread_us=[round(per[0] * 1e6, 1), round(per[-1] * 1e6, 1)])
        rows.append(row)
        print(json.dumps(row), flush=True)
    assert m.engine.persistent_step_fallbacks == 0
    m.engine.set_persistent_step(True)
    out = dict(device=torch.cuda.get_device_name(0), weight_bytes=weight_bytes, rows=rows)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
