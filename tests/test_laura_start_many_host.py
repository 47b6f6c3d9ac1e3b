"""Several prompts per prefix pass, held for free slots (fc_laura_slots_start_many, fc_laura_slots_start_from_session,
DecodeSlots.start_many / start_from(source=), Text2Audio.generate_many(prefill=P)), the parts that need no device: the C ABI's
declarations, the prefill rule of generate_many (funcodec_amd.laura.prefill / HeldPrompts) driven through the real drivers against a
stand-in session, and the argument checks of the Python wrappers."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from funcodec_amd import _lib
from funcodec_amd.engine import EngineError
from funcodec_amd.laura import DecodeSlots, HeldPrompts, drive_samples, prefill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fc_laura_slots_start_many_workspace_bytes": 4, "fc_laura_slots_start_many": 17, "fc_laura_slots_start_from_session": 11}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_the_calls_are_declared_bound_and_exported(name):
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/funcodec_amd.h"
    assert name in _lib.SYMBOLS
    assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SYMBOLS[name][1]) == NAMES[name]
    assert hasattr(ctypes.CDLL(_lib.lib_path()), name), f"{name} is not exported"
    start = hdr.index("typedef struct fc_laura_slots")
    assert name + "(" in hdr[start: hdr.index("#ifdef __cplusplus", start)], "inside the session's section"
    # pure additions: the ABI version stays
    assert _lib.FC_ABI_VERSION == 7 and re.search(r"#define\s+FC_ABI_VERSION\s+7\b", hdr)


def test_the_import_says_that_both_sessions_share_a_stream():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    own = hdr[hdr.index("fc_laura_slots_start_many("): hdr.index("fc_laura_slots_start_from_session(")]
    assert "ONE STREAM" in own.upper()


# ---- the prefill rule ---------------------------------------------------------------------------------------------------------
def test_prefill_is_a_plain_function_of_what_is_held():
    assert prefill(0, {}, 4, 10, 0) == [(0, 0), (1, 1), (2, 2), (3, 3)]
    assert prefill(2, {0: 0, 1: 1, 2: 2, 3: 3}, 4, 10, 4) == []                       # held: nothing to do
    assert prefill(4, {}, 4, 10, 4) == [(0, 4), (1, 5), (2, 6), (3, 7)]
    assert prefill(8, {}, 4, 10, 8) == [(0, 8), (1, 9)]                               # the tail: fewer requests than rows
    assert prefill(4, {1: 3}, 4, 10, 4) == [(0, 4), (2, 5), (3, 6)]                   # row 1 still waits for candidates of request 3
    assert prefill(1, {}, 4, 10, 6) == [(0, 1), (1, 6), (2, 7), (3, 8)]               # a request that comes back: itself, then fresh ones
    assert prefill(9, {0: 4, 1: 7, 2: 5, 3: 6}, 4, 10, 9) == [(1, 9)]                 # no free row: the request needed last gives way
    with pytest.raises(ValueError):
        prefill(10, {}, 4, 10, 0)
    with pytest.raises(ValueError):
        prefill(0, {}, 0, 10, 0)


class HeldSession:
    """A stand-in for the pair (main session, holding session) as generate_many(prefill=P) drives them: candidates of `lengths` steps,
    every start a copy from a row of the holding session, which must hold the candidate's request at that moment."""

    def __init__(self, slots, rows, n, samples, lengths):
        self.left = [None] * slots
        self.plan = HeldPrompts(rows, n, samples)
        self.samples, self.lengths = samples, lengths
        self.row_holds = {}                       # what the holding session's rows REALLY hold (start_many overwrites a row)
        self.passes, self.begun, self.released_after = [], [], {}

    def begin(self, slot, c):
        assert self.left[slot] is None
        i = c // self.samples
        todo = self.plan.need(i)
        if todo:
            assert len({r for r, _ in todo}) == len(todo) and all(0 <= r < self.plan.rows for r, _ in todo)
            self.passes.append([q for _, q in todo])
            for r, q in todo:
                self.row_holds[r] = q
        row = self.plan.start(i)
        assert self.row_holds.get(row) == i, f"row {row} holds request {self.row_holds.get(row)}, not {i}: not held before it is started"
        self.begun.append(c)
        if i not in self.plan.held.values():
            self.released_after[i] = c
        self.left[slot] = self.lengths[c] - 1

    def start(self, slot, c):
        self.begin(slot, c)

    def start_from(self, slot, src, c):
        self.begin(slot, c)

    def step(self, n):
        out = {}
        for i, v in enumerate(self.left):
            if v is not None:
                self.left[i] = v - n if v > 0 else v
                out[i] = "done" if self.left[i] <= 0 else "running"
        return out

    def take(self, slot):
        assert self.left[slot] is not None and self.left[slot] <= 0
        self.left[slot] = None
        return ("result", slot)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("slots", [1, 2, 3, 7])
def test_four_rows_over_ten_requests_in_any_order_of_releases(slots, seed):
    """Lengths drawn at random decide which slot is released when.  Every request is held before it is started (the stand-in asserts
    it at every start) and exactly ceil(10 / 4) passes run."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = [int(v) for v in rng.integers(1, 30, size=10)]
    fs = HeldSession(slots, 4, 10, 1, lengths)
    res = drive_samples(fs, slots, 10, 1, fs.start, fs.start_from)
    assert len(res) == 10 and sorted(fs.begun) == list(range(10))
    assert fs.plan.passes == len(fs.passes) == math.ceil(10 / 4) == 3
    assert fs.passes == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert fs.plan.held == {}, "every row is released at the end"


@pytest.mark.parametrize("slots,rows", [(2, 4), (4, 2), (5, 1), (3, 16)])
def test_with_three_samples_a_row_is_released_only_after_its_third_candidate(slots, rows):
    rng = np.random.Generator(np.random.PCG64(slots * 17 + rows))
    lengths = [int(v) for v in rng.integers(1, 20, size=21)]
    fs = HeldSession(slots, rows, 7, 3, lengths)
    res = drive_samples(fs, slots, 7, 3, fs.start, fs.start_from)
    assert len(res) == 7 and all(len(r) == 3 for r in res) and sorted(fs.begun) == list(range(21))
    assert fs.released_after == {i: 3 * i + 2 for i in range(7)}                      # behind candidate 3 i + 2, the third
    assert fs.plan.passes == math.ceil(7 / rows)


def test_held_prompts_counts_candidates_per_request():
    h = HeldPrompts(2, 3, 3)
    assert h.need(0) == [(0, 0), (1, 1)] and h.need(1) == [] and h.passes == 1
    assert [h.start(0), h.start(0)] == [0, 0] and h.held == {0: 0, 1: 1}
    assert h.start(0) == 0 and h.held == {1: 1}                                       # the third candidate releases the row
    assert h.start(1) == 1 and h.need(2) == [(0, 2)] and h.passes == 2                # row 1 still held: request 2 into row 0
    with pytest.raises(KeyError):
        h.row_of(0)


# ---- argument checks that need no device ------------------------------------------------------------------------------------------
def bare(slots=4):
    s = DecodeSlots.__new__(DecodeSlots)              # no engine behind it: _many_rows reads the slot count only
    s.slots = slots
    return s


REQ = dict(text_outs=None, text_len=3)


def test_start_many_checks_its_requests_before_any_device_work():
    s = bare(4)
    rows = s._many_rows({2: REQ, 0: dict(REQ, max_length=5, sampling=5, seed=9)})
    assert [r[0] for r in rows] == [2, 0]                                             # the order given
    assert rows[0][1]["max_length"] == 750 and rows[0][1]["sampling"] is True and rows[0][1]["seed"] == 0
    assert rows[0][1]["continual"] is None and rows[0][1]["rules"] is None           # start's defaults
    assert rows[1][1]["max_length"] == 5 and rows[1][1]["sampling"] == 5 and rows[1][1]["seed"] == 9
    with pytest.raises(EngineError, match="no requests"):
        s._many_rows({})
    with pytest.raises(EngineError, match="slot 4 outside"):
        s._many_rows({1: REQ, 4: REQ})
    with pytest.raises(EngineError, match="slot -1 outside"):
        s._many_rows({-1: REQ})
    with pytest.raises(EngineError, match="slot 1 is named twice"):
        s._many_rows([(1, REQ), (3, REQ), (1, REQ)])
    with pytest.raises(EngineError, match=r"slot 2.*forced"):
        s._many_rows({2: dict(REQ, forced=None)})
    with pytest.raises(EngineError, match=r"slot 2.*text_outs and text_len"):
        s._many_rows({2: dict(text_outs=None)})
    with pytest.raises(EngineError, match=r"slot 3.*max_length 0"):
        s._many_rows({3: dict(REQ, max_length=0)})
    with pytest.raises(EngineError, match=r"slot 1.*dict"):
        s._many_rows({1: 5})


def test_start_many_takes_at_most_sixteen_prompts():
    with pytest.raises(EngineError, match=r"slot 16 outside"):
        bare(16)._many_rows({i: REQ for i in range(17)})                              # 17 distinct slots: one is out of range


def test_generate_many_refuses_a_prefill_outside_its_range():
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    t2a = Text2Audio.__new__(Text2Audio)              # the check comes before anything of the model is used
    t2a.model = type("M", (), {"predict_nq": 2})()
    for bad in (-1, 17):
        with pytest.raises(ValueError, match="prefill"):
            t2a.generate_many(["a"], prefill=bad)
