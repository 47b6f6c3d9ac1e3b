"""Starting a decoding slot from the prompt another slot holds (fc_laura_slots_start_from, DecodeSlots.start_from,
Text2Audio.generate_many(samples=N)), the parts that need no device: the C ABI's declaration, and the sharing rule of generate_many
(funcodec_amd.laura.drive_samples) against a stand-in session that counts calls."""
import ctypes
import os
import re

import numpy as np

from funcodec_amd import _lib
from funcodec_amd.laura import drive_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fc_laura_slots_start_from"


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    m = re.search(r"\b" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{NAME} is not declared in include/funcodec_amd.h"
    assert NAME in _lib.SYMBOLS
    assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SYMBOLS[NAME][1]) == 10
    assert hasattr(ctypes.CDLL(_lib.lib_path()), NAME), f"{NAME} is not exported"
    # inside the session's section, behind take, with the reference callable it stands for; a pure addition: the ABI version stays
    start = hdr.index("typedef struct fc_laura_slots")
    sect = hdr[start: hdr.index("#ifdef __cplusplus", start)]
    assert NAME in sect and sect.index("fc_laura_slots_take(") < sect.index(NAME + "(")
    own = sect[sect.index("fc_laura_slots_take("): sect.index(NAME + "(")]
    assert "decode_codec" in own and "laura_model.py:501-548" in own
    assert _lib.FC_ABI_VERSION == 7 and re.search(r"#define\s+FC_ABI_VERSION\s+7\b", hdr)


class CountingSession:
    """A stand-in for DecodeSlots: a candidate of `length` samples has drawn one at its start and ends after length - 1 steps.  It knows
    which request every slot holds, so it can say whether a start_from names a slot that holds the same request at that moment."""

    def __init__(self, slots, samples, lengths):
        self.left, self.holds = [None] * slots, [None] * slots
        self.samples, self.lengths = samples, lengths
        self.starts, self.copies = [], []          # (slot, candidate) / (slot, source slot, candidate)

    def _begin(self, slot, c):
        assert self.left[slot] is None, "a slot that holds an utterance must not be restarted by the policy"
        self.left[slot], self.holds[slot] = self.lengths[c] - 1, c // self.samples

    def start(self, slot, c):
        self._begin(slot, c)
        self.starts.append((slot, c))

    def start_from(self, slot, src, c):
        assert src != slot and self.left[src] is not None, f"slot {src} holds nothing"
        assert self.holds[src] == c // self.samples, f"slot {src} holds request {self.holds[src]}, not {c // self.samples}"
        self._begin(slot, c)
        self.copies.append((slot, src, c))

    def step(self, n):
        out = {}
        for i, v in enumerate(self.left):
            if v is not None:
                self.left[i] = v - n if v > 0 else v
                out[i] = "done" if self.left[i] <= 0 else "running"
        return out

    def take(self, slot):
        assert self.left[slot] is not None and self.left[slot] <= 0, "take on a slot that has not ended"
        self.left[slot] = None
        return ("result", slot)


def run(slots, n, samples, lengths):
    fs = CountingSession(slots, samples, lengths)
    res = drive_samples(fs, slots, n, samples, fs.start, fs.start_from)
    assert len(res) == n and all(len(r) == samples for r in res)
    started = sorted([c for _, c in fs.starts] + [c for _, _, c in fs.copies])
    assert started == list(range(n * samples))                              # every candidate exactly once
    return fs


def test_equal_lengths_share_every_prefix():
    """4 requests x 3 samples of equal length through 6 slots: two requests at a time, one prefix pass each."""
    fs = run(6, 4, 3, [9] * 12)
    assert len(fs.starts) == 4 and len(fs.copies) == 8
    assert [c for _, c in fs.starts] == [0, 3, 6, 9]                        # the first candidate of each request runs the pass


def test_unequal_lengths_never_cost_more_than_a_start_each():
    """5 x 3 through 4 slots, lengths differ: a request's candidates meet in time or not; every start_from names a slot that holds
    the same request at that moment (the stand-in asserts it), and no candidate is started twice."""
    rng = np.random.Generator(np.random.PCG64(5))
    lengths = [int(v) for v in rng.integers(2, 40, size=15)]
    fs = run(4, 5, 3, lengths)
    assert len(fs.starts) + len(fs.copies) == 15 and 5 <= len(fs.starts) <= 15
    assert len(fs.copies) >= 1
    first = {}
    for _, c in fs.starts:
        first.setdefault(c // 3, c)
    assert sorted(first) == list(range(5))                                  # every request ran its own prefix pass at least once


def test_one_sample_makes_the_calls_it_made_before():
    lengths = [5, 9, 3, 7, 4, 6, 8]
    fs = run(3, 7, 1, lengths)
    assert fs.copies == [] and [c for _, c in fs.starts] == list(range(7))
    # the same slots as drive_slots alone gives these requests
    from funcodec_amd.laura import drive_slots
    plain = CountingSession(3, 1, lengths)
    drive_slots(plain, 3, 7, plain.start)
    assert plain.starts == fs.starts
