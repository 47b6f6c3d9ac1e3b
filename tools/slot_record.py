"""Measurements of the slot record (csrc/slots_kernels.h; fc_slotrec_export / fc_slotrec_import, StreamSlots.migrate), written to
profiles/slot_record.txt:

  for ss320 (no sequence model) and ss320tfc (two transformer blocks, max_frames 1500 with every slot at 7, 750 and 1500 cached frames),
  two 32-slot sessions and n = 1 / 8 / 32 named slots: the export launch, the import launch and ``migrate`` (both, no host copy of the
  floats), each as host time around the synchronised call and as device time between two events; the record's size per slot, the bytes
  moved (every float of a record is read once and written once) and GB/s by the device time; and a plain 1-frame encode push of the
  same 32-slot session in the same run.  The forms alternate in one process, median of 24.

The slots are brought to their frame counts by importing records of random floats (what a record holds does not change what moving it
costs); the layout fingerprint comes from one real export.  The ``move`` lines of profiles/laura_elastic.txt (LauraTTS sessions: rows of
keys and values moved inside one session) are copied beside the figures as context, not as a bar.

    python tools/slot_record.py [--out profiles/slot_record.txt]
"""
import argparse
import datetime
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from rvq_rate import REPS, model, timed  # noqa: E402
from funcodec_amd.stream import _Side, slot_record_floats  # noqa: E402
from funcodec_amd.synth import synthetic_audio  # noqa: E402

S = 32
MAX_FRAMES = 1500


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def both(forms, reps=REPS, warm=3):
    """{form: (host ms, device ms)}: medians, the forms taking turns; host = wall clock around the synchronised call"""
    for _ in range(warm):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    host, dev = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            host[k].append(wall(fn))
        for k, fn in forms.items():
            dev[k].append(timed(fn))
    return {k: (statistics.median(host[k]), statistics.median(dev[k])) for k in forms}


def side(frames):
    sd = _Side()
    sd.started, sd.frames = True, frames
    return sd


def load(sess, layout, frames, cached):
    """every slot of the session Running on both sides with `frames` cached frames: records of random floats, one import launch"""
    f = frames if cached else 0
    n = slot_record_floats(sess.arch, f, f, cached)
    buf = torch.randn((S, -(-n // 4) * 4), device=sess.device) * 0.1
    sess._import_rows(list(range(S)), buf, [(layout, 1, 1, f, f)] * S)
    for b in range(S):
        sess._adopt(b, side(frames), side(frames), sess.n_q, None, 1.0)
    return n


def measure(say, net):
    m = model(net)
    cached = net == "ss320tfc"
    kw = {"max_frames": MAX_FRAMES} if cached else {}
    hop = m.engine.hop_length
    src, dst = m.open_slots(S, max_chunk=16 * hop, **kw), m.open_slots(S, max_chunk=16 * hop, **kw)
    wav = torch.from_numpy(synthetic_audio(1, src.min_first_samples, 0, "noise")).cuda()
    src.encode({0: wav})                                # one real START push: the session's own fingerprint
    layout = src.export(0).meta[0]
    one = {b: wav[..., :hop] for b in range(S)}
    say(f"{net}: two sessions of {S} slots" + (f", max_frames {MAX_FRAMES}" if cached else "") + f"; median of {REPS}, the forms alternating (us)")
    for frames in ((7, 750, 1500) if cached else (7,)):
        floats = load(src, layout, frames, cached)
        load(dst, layout, frames, cached)
        say(f"  {frames} frames per slot and side: a record holds {floats} floats = {4 * floats} bytes" if cached
            else f"  a record holds {floats} floats = {4 * floats} bytes")
        for n in (1, 8, 32):
            rows = list(range(n))
            sides = [(src._enc[b], src._dec[b]) for b in rows]
            buf, metas = src._export_rows(m.engine.lib.fc_slotrec_export, rows, sides)
            t = both({"export": lambda: src._export_rows(m.engine.lib.fc_slotrec_export, rows, sides),
                      "import": lambda: dst._import_rows(rows, buf, metas),
                      "migrate": lambda: src.migrate(dst, {b: S - 1 - b for b in rows})})
            moved = 2 * 4 * floats * n                   # read once, written once
            for k in ("export", "import", "migrate"):
                by = moved * (2 if k == "migrate" else 1)
                say(f"    n = {n:2d}  {k:7s}  host, synchronised {1e3 * t[k][0]:8.1f}   device, between events {1e3 * t[k][1]:8.1f}   "
                    f"{by} bytes read and written = {by / (t[k][1] * 1e-3) / 1e9:7.1f} GB/s")
        if frames < MAX_FRAMES:
            load(src, layout, frames, cached)           # the pushes below advance every slot by one frame each
            t = both({"push": lambda: src.encode(one)}, reps=REPS, warm=3)
            say(f"    a plain 1-frame encode push of the same session, all {S} slots active:  host, synchronised {1e3 * t['push'][0]:8.1f}   "
                f"device, between events {1e3 * t['push'][1]:8.1f}")
        else:
            say("    (no plain push at 1500 frames: the caches are full, the bound refuses it)")
    del src, dst
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slot_record.txt"))
    args = ap.parse_args()
    lines = [f"tools/slot_record.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}"]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    for net in ("ss320", "ss320tfc"):
        measure(say, net)
    say("no function that a push runs was changed by the slot record: the table of segments is built at create, export and import are calls of their own")
    say("context, not a bar -- the move of LauraTTS rows inside one session (profiles/laura_elastic.txt):")
    with open(os.path.join(ROOT, "profiles", "laura_elastic.txt")) as f:
        for ln in f.read().split("lauramusic")[0].splitlines():
            if ln.lstrip().startswith("k ="):
                say("  " + ln.strip())
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
