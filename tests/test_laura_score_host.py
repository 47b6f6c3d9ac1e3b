"""Scores of a decoding session (fc_laura_slots_*_scored, fc_laura_slots_score, DecodeSlots.score, generate_many(keep="best")), the
parts that need no device: the ranking rule (funcodec_amd.laura.pick_best), the keep="best" driver (drive_best) against a scripted
session, the C ABI's declarations and the refusals of the binding that come before any library call."""
import ctypes
import os
import re

import pytest
import torch

from funcodec_amd import _lib
from funcodec_amd.engine import EngineError
from funcodec_amd.laura import drive_best, drive_retries, pick_best

from test_laura_fork_host import ScriptedSession, bare_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fc_laura_slots_state_bytes_scored": 5, "fc_laura_slots_create_scored": 8, "fc_laura_slots_score": 6}


# ---- the ranking rule -------------------------------------------------------------------------------------------------------
def test_eos_ranks_above_length_whatever_the_means():
    assert pick_best([(-1.0, 10, False), (-500.0, 10, True), (-0.5, 10, False)]) == 1
    assert pick_best([(-500.0, 10, True), (-1.0, 10, False)]) == 0
    assert pick_best([(0.0, 1, False), (-1e9, 1, True)]) == 1


def test_the_higher_mean_wins_within_a_class():
    # sums -30 / 10 steps, -20 / 5 steps, -28 / 10 steps: means -3, -4, -2.8 -- the mean ranks, not the sum
    assert pick_best([(-30.0, 10, True), (-20.0, 5, True), (-28.0, 10, True)]) == 2
    assert pick_best([(-30.0, 10, False), (-20.0, 5, False), (-28.0, 10, False)]) == 2
    assert pick_best([(-30.0, 10, False), (-20.0, 5, True), (-10.0, 2, True), (-1.0, 10, False)]) == 1      # means -4 and -5 among <eos>
    assert pick_best([(-7.5, 3, True)]) == 0


def test_ties_go_to_the_lower_index():
    assert pick_best([(-6.0, 3, True), (-4.0, 2, True), (-2.0, 1, True)]) == 0
    assert pick_best([(-9.0, 3, False), (-6.0, 3, False), (-4.0, 2, False)]) == 1
    assert pick_best([(-6.0, 3, False), (-6.0, 3, True), (-2.0, 1, True)]) == 1


def test_count_zero_and_no_candidates_are_refused():
    with pytest.raises(ValueError, match="candidate 1.*count 0"):
        pick_best([(-1.0, 4, True), (0.0, 0, True)])
    with pytest.raises(ValueError, match="count 0"):
        pick_best([(0.0, 0, False)])
    with pytest.raises(ValueError, match="no candidates"):
        pick_best([])


# ---- the keep="best" driver ---------------------------------------------------------------------------------------------------
class ScoredSession(ScriptedSession):
    """ScriptedSession whose takes carry a score: mean[c][attempt] is the mean log-probability per step of candidate c's attempt; an
    attempt that ends on <eos> has one term more than tokens."""

    def __init__(self, slots, script, max_length, mean):
        super().__init__(slots, script, max_length)
        self.mean = mean

    def take(self, slot, return_score=False):
        assert return_score, "the driver must ask for the score with the take"
        c, a, kind, n = super().take(slot)
        count = n + 1 if kind == "eos" else n
        return (c, a, kind, n, (self.mean[c][a] * count, count, kind == "eos"))


def best(slots, script, mean, retries, samples, max_length=10):
    fs = ScoredSession(slots, script, max_length, mean)
    return fs, drive_best(fs, slots, len(script) // samples, samples, retries, max_length, fs.start, fs.start_from, fs.rewind)


def test_the_driver_keeps_pick_best_of_every_request():
    # request 0: a run-away with the best mean, two <eos> candidates;  request 1: all run-aways;  request 2: a tie between 1 and 2
    script = [[("len", 10)], [("eos", 6)], [("eos", 4)],
              [("len", 10)], [("len", 10)], [("len", 10)],
              [("eos", 3)], [("eos", 5)], [("eos", 7)]]
    mean = [[-0.1], [-2.0], [-3.0], [-4.0], [-2.5], [-3.0], [-5.0], [-1.0], [-1.0]]
    fs, kept = best(4, script, mean, 0, 3)
    assert [k for k, _ in kept] == [1, 1, 1]
    assert [t[:4] for _, t in kept] == [(1, 0, "eos", 6), (4, 0, "len", 10), (7, 0, "eos", 5)]
    assert [t[-1] for _, t in kept] == [(-2.0 * 7, 7, True), (-2.5 * 10, 10, False), (-1.0 * 6, 6, True)]
    # every candidate ran and was taken exactly once, and nothing was rewound
    assert sorted(e[2] for e in fs.log if e[0] == "take") == list(range(9))
    assert not [e for e in fs.log if e[0] == "rewind"]


def test_with_retries_the_last_attempt_is_the_one_ranked():
    # candidate 0 runs away (mean -0.5), is rewound and ends on <eos> with mean -4: ranked by that;  candidate 1 ends on <eos> at once
    # with -5;  request 1: candidate 2 runs away twice (last attempt -1), candidate 3 runs away, then on <eos> with -9
    script = [[("len", 10), ("eos", 8)], [("eos", 5)], [("len", 10), ("len", 10)], [("len", 10), ("eos", 7)]]
    mean = [[-0.5, -4.0], [-5.0], [-0.2, -1.0], [-0.1, -9.0]]
    fs, kept = best(2, script, mean, 1, 2)
    assert [(k, t[:4]) for k, t in kept] == [(0, (0, 1, "eos", 8)), (1, (3, 1, "eos", 7))]
    assert kept[0][1][-1] == (-4.0 * 9, 9, True)
    # the policy underneath is drive_retries' own: the same calls in the same order
    plain = ScriptedSession(2, script, 10)
    drive_retries(plain, 2, 2, 2, 1, 10, plain.start, plain.start_from, plain.rewind)
    assert plain.log == fs.log
    assert [e[2:5] for e in fs.log if e[0] == "rewind"] == [(0, 5, 1), (2, 5, 1), (3, 5, 1)]


def test_one_sample_keeps_it():
    fs, kept = best(2, [[("eos", 3)], [("len", 10)], [("eos", 9)]], [[-1.0], [-2.0], [-3.0]], 0, 1)
    assert [k for k, _ in kept] == [0, 0, 0] and [t[0] for _, t in kept] == [0, 1, 2]


# ---- the C ABI and the binding ------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    lib = ctypes.CDLL(_lib.lib_path())
    start = hdr.index("typedef struct fc_laura_slots")
    sect = hdr[start: hdr.index("#ifdef __cplusplus", start)]
    for name, nargs in NAMES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", sect, re.S)
        assert m, f"{name} is not declared in the session's section of include/funcodec_amd.h"
        assert name in _lib.SYMBOLS
        assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported"
    # pure additions behind fork, with the reference callable the score stands for: the earlier calls and the ABI version stay
    assert sect.index("fc_laura_slots_fork(") < sect.index("fc_laura_slots_state_bytes_scored(")
    assert "sampling_ids" in sect[sect.index("fc_laura_slots_fork("):] and "laura_model.py:466-499" in sect
    assert len(_lib.SYMBOLS["fc_laura_slots_state_bytes"][1]) == 4 and len(_lib.SYMBOLS["fc_laura_slots_create"][1]) == 7
    assert len(_lib.SYMBOLS["fc_laura_slots_take"][1]) == 6
    assert _lib.FC_ABI_VERSION == 7 and re.search(r"#define\s+FC_ABI_VERSION\s+7\b", hdr)


def test_a_null_session_and_a_null_engine_are_refused_by_the_library():
    lib = _lib.load()
    n, e = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.fc_laura_slots_score(None, 0, None, 0, ctypes.byref(n), ctypes.byref(e)) != 0
    assert "null session" in _lib.last_error()
    assert lib.fc_laura_slots_state_bytes_scored(None, 4, 64, 0, 1) == 0


def test_a_session_without_scores_refuses_before_any_call():
    s = bare_session()
    s.with_score, s.max_positions = False, 64
    if torch.cuda.is_available():                   # the methods make the session's device current first
        s.device = "cuda:0"
    s._status = (ctypes.c_int32 * 4)(2, 2, 2, 2)
    try:
        with pytest.raises(EngineError, match=r"slot 2.*without scores"):
            s.score(2)
        with pytest.raises(EngineError, match=r"slot 1.*without scores"):
            s.take(1, return_score=True)
        with pytest.raises(EngineError, match=r"slot 3.*without scores"):
            s.score_row(3)
        with pytest.raises(EngineError, match="slot 4 outside"):
            s.score(4)
        s._h = None
        with pytest.raises(EngineError, match="used after free"):
            s.score(0)
    finally:
        s._h = None                                 # nothing to destroy


def test_keep_is_checked():
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    t2a = Text2Audio.__new__(Text2Audio)
    t2a.model = type("M", (), {"predict_nq": 2})()
    with pytest.raises(ValueError, match="keep must be"):
        t2a.generate_many(["a"], keep="first")
