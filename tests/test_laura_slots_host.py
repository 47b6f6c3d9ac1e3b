"""Decoding session of the LauraTTS engine (fc_laura_slots_*, LauraEngine.open_decode, Text2Audio.generate_many), the parts that need no
device: the C ABI's declarations, and the refill policy of generate_many (funcodec_amd.laura.refill / drive_slots) against a stand-in
session whose slots end after given numbers of steps."""
import ctypes
import os
import re

import numpy as np
import pytest

from funcodec_amd import _lib
from funcodec_amd.laura import drive_slots, refill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["fc_laura_slots_state_bytes", "fc_laura_slots_create", "fc_laura_slots_destroy", "fc_laura_slots_workspace_bytes",
         "fc_laura_slots_start", "fc_laura_slots_step", "fc_laura_slots_take"]


def test_the_session_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    lib = ctypes.CDLL(_lib.lib_path())
    for name in CALLS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/funcodec_amd.h"
        assert name in _lib.SYMBOLS, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(lib, name), f"{name} is not exported"
    # each is declared with the reference callable it stands for; pure additions: the ABI version stays
    sect = hdr[hdr.index("typedef struct fc_laura_slots"): hdr.index("#ifdef __cplusplus", hdr.index("typedef struct fc_laura_slots"))]
    before = hdr[hdr.index("decoding session"): hdr.index("typedef struct fc_laura_slots")]
    assert "decode_codec" in before and "laura_model.py:501-548" in before and "decode_codec" in sect
    assert _lib.FC_ABI_VERSION == 7 and re.search(r"#define\s+FC_ABI_VERSION\s+7\b", hdr)


class FakeSession:
    """A stand-in for DecodeSlots: a slot started with `length` samples has drawn one at its start and ends after length - 1 steps."""

    def __init__(self, slots, fail_at=None):
        self.left = [None] * slots
        self.owner = [None] * slots
        self.steps = 0
        self.calls = 0
        self.log = []                      # (steps run when it happened, what, slot, request)
        self.fail_at = fail_at             # the step call that reports every running slot failed, once

    def start(self, slot, req, length):
        assert self.left[slot] is None or self.left[slot] <= 0, "a running slot must not be restarted by the policy"
        self.left[slot] = length - 1
        self.owner[slot] = req
        self.log.append((self.steps, "start", slot, req))

    def step(self, n):
        self.calls += 1
        running = [i for i, v in enumerate(self.left) if v is not None and v > 0]
        ended = [i for i, v in enumerate(self.left) if v is not None and v <= 0]
        if not running and not ended:
            return {}
        if running:
            self.steps += n
        out = {i: "done" for i in ended}
        failing = self.fail_at is not None and self.calls == self.fail_at
        for i in running:
            self.left[i] -= n
            out[i] = "failed" if failing else ("done" if self.left[i] <= 0 else "running")
            if failing:
                self.left[i] = 0
        return out

    def take(self, slot):
        assert self.left[slot] is not None and self.left[slot] <= 0, "take on a slot that has not ended"
        req = self.owner[slot]
        self.left[slot] = None
        self.log.append((self.steps, "take", slot, req))
        return ("result", req)


def lock_step_steps(lengths, slots, max_length):
    """Steps that decode_codec calls of `slots` rows in arrival order run: a call samples once from the prefix, then steps until every row
    has ended, which it checks after every 16th sample (do_decode's loop), or until max_length samples."""
    total = 0
    for i in range(0, len(lengths), slots):
        longest = max(lengths[i: i + slots])
        s = 1
        while s < max_length:
            total += 1
            if (s & 15) == 15 and s + 1 < max_length and longest <= s + 1:
                break
            s += 1
    return total


def test_refill_is_arrival_order_into_ascending_free_slots():
    assert refill([], [0, 1]) == []
    assert refill([4, 5, 6], []) == []
    assert refill([4, 5, 6], [3, 1]) == [(1, 4), (3, 5)]
    assert refill([7], [2, 0, 1]) == [(0, 7)]


@pytest.mark.parametrize("step_n", [1, 16])
@pytest.mark.parametrize("slots,n", [(2, 5), (4, 9), (16, 64), (3, 3), (5, 2)])
def test_every_request_runs_once_slots_are_reused_and_results_keep_request_order(slots, n, step_n):
    rng = np.random.Generator(np.random.PCG64(slots * 100 + n))
    lengths = [int(v) for v in rng.integers(2, 90, size=n)]
    fs = FakeSession(slots)
    res = drive_slots(fs, slots, n, lambda slot, req: fs.start(slot, req, lengths[req]), step_n=step_n)
    assert res == [("result", i) for i in range(n)]                         # request order
    starts = [e for e in fs.log if e[1] == "start"]
    assert sorted(e[3] for e in starts) == list(range(n))                    # each exactly once
    assert [e[3] for e in starts] == list(range(n))                          # in arrival order
    takes = {e[3]: e for e in fs.log if e[1] == "take"}
    assert sorted(takes) == list(range(n))
    # a freed slot is reused at the next step boundary: while requests wait, the next start on a slot happens at the step count of its take
    for k, (at, _, slot, req) in enumerate(starts):
        prev = [e for e in fs.log[: fs.log.index((at, "start", slot, req))] if e[2] == slot and e[1] == "take"]
        if prev:
            assert prev[-1][0] == at, (slot, req, prev[-1], at)
    assert all(v is None for v in fs.left)


def test_a_failed_step_puts_the_requests_back_at_the_head_of_the_queue():
    lengths = [40, 40, 40, 40, 40]
    fs = FakeSession(2, fail_at=2)
    res = drive_slots(fs, 2, 5, lambda slot, req: fs.start(slot, req, lengths[req]), step_n=16)
    assert res == [("result", i) for i in range(5)]
    starts = [e[3] for e in fs.log if e[1] == "start"]
    assert starts == [0, 1, 0, 1, 2, 3, 4]


@pytest.mark.parametrize("order", ["rising", "falling", "shuffled0", "shuffled1", "shuffled2"])
def test_the_session_never_runs_more_steps_than_lock_step_calls(order):
    """64 requests with lengths spread over 50 .. 750 through 16 slots kept full, against four decode_codec calls of 16 rows in arrival
    order (max_length 750): a lock-step call runs until its longest row ends, the session refills a slot as soon as its row does.
    Rising lengths are the lock-step calls' best case (rows of a call end together); drive_slots' default, a look after every step,
    is what makes the bound hold there too (its docstring has the argument)."""
    slots, n = 16, 64
    lengths = [50 + (700 * i) // (n - 1) for i in range(n)]
    assert min(lengths) == 50 and max(lengths) == 750
    if order == "falling":
        lengths.reverse()
    elif order.startswith("shuffled"):
        np.random.Generator(np.random.PCG64(int(order[-1]))).shuffle(lengths)
    fs = FakeSession(slots)
    drive_slots(fs, slots, n, lambda slot, req: fs.start(slot, req, lengths[req]))
    lock = lock_step_steps(lengths, slots, 750)
    assert fs.steps <= lock, (order, fs.steps, lock)
    print(order, "session steps", fs.steps, "lock-step steps", lock)
