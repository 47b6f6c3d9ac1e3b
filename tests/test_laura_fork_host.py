"""Forking and rewinding a decoding slot (fc_laura_slots_fork, DecodeSlots.fork / rewind, Text2Audio.generate_many(retries=R)), the
parts that need no device: the C ABI's declaration, the argument checks of the binding that come before any library call, and the
retry policy of generate_many (funcodec_amd.laura.drive_retries) against a scripted session."""
import ctypes
import os
import re

import pytest

from funcodec_amd import _lib
from funcodec_amd.engine import EngineError
from funcodec_amd.laura import RETRY_SEED_STRIDE, DecodeSlots, drive_retries, drive_samples, drive_slots, retry_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fc_laura_slots_fork"


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    m = re.search(r"\b" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{NAME} is not declared in include/funcodec_amd.h"
    assert NAME in _lib.SYMBOLS
    assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SYMBOLS[NAME][1]) == 10
    assert hasattr(ctypes.CDLL(_lib.lib_path()), NAME), f"{NAME} is not exported"
    # inside the session's section, behind start_from, with the reference callable it stands for; a pure addition: the ABI version stays
    start = hdr.index("typedef struct fc_laura_slots")
    sect = hdr[start: hdr.index("#ifdef __cplusplus", start)]
    assert sect.index("fc_laura_slots_start_from(") < sect.index(NAME + "(")
    own = sect[sect.index("fc_laura_slots_start_from("): sect.index(NAME + "(")]
    assert "decode_codec" in own and "laura_model.py:501-548" in own
    assert _lib.FC_ABI_VERSION == 7 and re.search(r"#define\s+FC_ABI_VERSION\s+7\b", hdr)


def test_a_null_session_is_refused_by_the_library():
    lib = _lib.load()
    assert lib.fc_laura_slots_fork(None, 0, 1, -1, 0, 1, 0, 0.0, 0, None) != 0
    assert "null session" in _lib.last_error()


def bare_session(slots=4):
    """A DecodeSlots without an engine: enough for the checks that come before the first library call."""
    s = DecodeSlots.__new__(DecodeSlots)
    s.slots, s.device, s._h = slots, "cpu", ctypes.c_void_p(1)
    s._max_length = [12] * slots
    s._n_gen = (ctypes.c_int32 * slots)()
    s.state = None
    return s


def test_the_binding_checks_its_arguments_before_any_call():
    s = bare_session()
    try:
        with pytest.raises(EngineError, match="source slot 4"):
            s.fork(0, 4)
        with pytest.raises(EngineError, match="source slot -1"):
            s.fork(0, -1, 2)
        with pytest.raises(EngineError, match=r"slot 2.*keep -3"):
            s.fork(2, 1, -3)
        with pytest.raises(EngineError, match=r"slot 2.*keep -2"):
            s.rewind(2, -2)
        with pytest.raises(EngineError, match=r"slot 0.*max_length 0"):
            s.fork(0, 1, 2, max_length=0)
        with pytest.raises(NotImplementedError):
            s.fork(0, 1, 2, sampling="beam")
        with pytest.raises(EngineError, match="slot 9"):
            s.n_gen(9)
        assert s.n_gen(3) == 0
        s._h = None
        with pytest.raises(EngineError, match="used after free"):
            s.fork(0, 1)
    finally:
        s._h = None                                 # nothing to destroy


def test_retry_seeds():
    assert retry_seed(5, 0) == 5 and retry_seed(5, 1) == 5 + 0x9E3779B97F4A7C15 and RETRY_SEED_STRIDE == 0x9E3779B97F4A7C15
    assert retry_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C15 - 1                     # mod 2^64
    assert retry_seed(7, 3) == (7 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64


class ScriptedSession:
    """A stand-in for DecodeSlots.  script[c] lists candidate c's attempts: ("len", n) ends by length with n_gen = n = max_length,
    ("eos", n) ends on <eos> with n_gen = n < max_length.  An attempt that starts with k tokens ends after n - k steps (a start has
    drawn its first token: k = 1).  Everything asked of it is recorded in arrival order."""

    def __init__(self, slots, script, max_length):
        self.script, self.max_length = script, max_length
        self.cand, self.attempt, self.gen = [None] * slots, [0] * slots, [0] * slots
        self.log = []

    def _end(self, slot):
        return self.script[self.cand[slot]][self.attempt[slot]]

    def start(self, slot, c):
        assert self.cand[slot] is None, "a slot that holds an utterance must not be restarted by the policy"
        self.cand[slot], self.attempt[slot], self.gen[slot] = c, 0, 1
        self.log.append(("start", slot, c))

    def start_from(self, slot, src, c):
        assert self.cand[src] is not None and src != slot
        self.start(slot, c)
        self.log[-1] = ("start_from", slot, src, c)

    def rewind(self, slot, c, keep, attempt):
        kind, n = self._end(slot)
        assert self.cand[slot] == c and self.gen[slot] == n, "rewound before its end"
        assert kind == "len", "a slot that ended on <eos> must not be rewound"
        assert attempt == self.attempt[slot] + 1
        self.attempt[slot], self.gen[slot] = attempt, keep
        self.log.append(("rewind", slot, c, keep, attempt, retry_seed(1000 + c, attempt)))

    def step(self, n):
        assert n == 1
        out = {}
        for slot, c in enumerate(self.cand):
            if c is None:
                continue
            end = self._end(slot)[1]
            self.gen[slot] = min(self.gen[slot] + 1, end)
            out[slot] = "done" if self.gen[slot] >= end else "running"
        return out

    def n_gen(self, slot):
        return self.gen[slot]

    def take(self, slot):
        kind, n = self._end(slot)
        assert self.gen[slot] == n, "take on a slot that has not ended"
        c, a = self.cand[slot], self.attempt[slot]
        self.cand[slot] = None
        self.log.append(("take", slot, c, a))
        return (c, a, kind, n)


def drive(slots, script, retries, max_length=10, samples=1):
    fs = ScriptedSession(slots, script, max_length)
    res = drive_retries(fs, slots, len(script) // samples, samples, retries, max_length, fs.start, fs.start_from, fs.rewind)
    return fs, [t for row in res for t in row]


def test_a_slot_that_ends_by_length_is_rewound_to_half_with_the_next_seed():
    # candidate 0 ends by length twice, then on <eos>; candidate 1 ends on <eos> at once; candidate 2 by length every time
    script = [[("len", 10), ("len", 10), ("eos", 7)], [("eos", 4)], [("len", 10)] * 4]
    fs, res = drive(2, script, retries=2)
    assert res == [(0, 2, "eos", 7), (1, 0, "eos", 4), (2, 2, "len", 10)]      # at most R rewinds: the last attempt is kept
    rew = [e for e in fs.log if e[0] == "rewind"]
    assert [(e[2], e[3], e[4]) for e in rew if e[2] == 0] == [(0, 5, 1), (0, 5, 2)]      # keep = n_gen // 2, attempts 1, 2
    assert [(e[2], e[3], e[4]) for e in rew if e[2] == 2] == [(2, 5, 1), (2, 5, 2)]
    assert [e[5] for e in rew if e[2] == 0] == [(1000 + k * 0x9E3779B97F4A7C15) % 2 ** 64 for k in (1, 2)]
    assert all(e[2] != 1 for e in rew), "a slot that ends on <eos> is never retried"


def test_an_odd_length_keeps_the_smaller_half_and_one_retry_is_one():
    fs, res = drive(1, [[("len", 9), ("len", 9)]], retries=1, max_length=9)
    assert [e for e in fs.log if e[0] == "rewind"] == [("rewind", 0, 0, 4, 1, retry_seed(1000, 1))]
    assert res == [(0, 1, "len", 9)]


def test_no_retries_rewinds_nothing_and_the_arrival_order_is_drive_slots_own():
    lengths = [("len", 10), ("eos", 3), ("len", 10), ("eos", 6), ("eos", 2), ("len", 10), ("eos", 8)]
    script = [[e] * 3 for e in lengths]
    fs, res = drive(3, script, retries=0)
    assert not [e for e in fs.log if e[0] == "rewind"]
    plain = ScriptedSession(3, script, 10)
    assert drive_slots(plain, 3, 7, plain.start) == res and plain.log == fs.log
    # with retries the requests still enter in arrival order, each exactly once, and go to the slots refill gives them
    fs2, res2 = drive(3, script, retries=2)
    starts = [e for e in fs2.log if e[0] == "start"]
    assert [e[2] for e in starts] == list(range(7))
    assert [r[0] for r in res2] == list(range(7))
    assert all(r[1] == (2 if lengths[r[0]][0] == "len" else 0) for r in res2)
    taken = {}
    for e in fs2.log:                           # a slot is refilled only after its candidate was taken
        if e[0] == "start":
            assert taken.get(e[1], True)
            taken[e[1]] = False
        elif e[0] == "take":
            taken[e[1]] = True


def test_retries_leave_the_sharing_of_prefixes_alone():
    # 2 requests x 2 samples through 4 slots: candidates 1 and 3 start from their siblings whether or not anything is rewound
    script = [[("len", 6)] * 2, [("eos", 5)], [("eos", 3)], [("len", 6), ("eos", 4)]]
    fs, res = drive(4, script, retries=1, max_length=6, samples=2)
    plain = ScriptedSession(4, script, 6)
    drive_samples(plain, 4, 2, 2, plain.start, plain.start_from)
    begin = ("start", "start_from")
    assert [e for e in fs.log if e[0] in begin] == [e for e in plain.log if e[0] in begin]
    assert [e for e in fs.log if e[0] == "start_from"] == [("start_from", 1, 0, 1), ("start_from", 3, 2, 3)]
    assert res == [(0, 1, "len", 6), (1, 0, "eos", 5), (2, 0, "eos", 3), (3, 1, "eos", 4)]
