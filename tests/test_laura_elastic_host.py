"""Elastic decoding sessions (fc_laura_slots_set_elastic / _step_blocks / _move, open_decode(elastic=True), DecodeSlots.move,
generate_many(elastic=True)), the parts that need no device: the C ABI's declarations and the binding's argument types, the
compaction rule, the slot -> row table of an ElasticSlots against a stand-in for the session underneath, and the keyword refusals."""
import ctypes
import os
import re
import types

import pytest

from funcodec_amd import _lib
from funcodec_amd import laura
from funcodec_amd.engine import EngineError
from funcodec_amd.laura import DecodeSlots, ElasticSlots, LauraEngine, LauraGenMI355X, RowTable, compact_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fc_laura_slots_set_elastic": 2, "fc_laura_slots_step_blocks": 1, "fc_laura_slots_move": 5}


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
        assert sect.index("fc_laura_slots_collect(") < sect.index(name + "(")        # pure additions behind everything there was
    assert _lib.FC_ABI_VERSION == 7 and re.search(r"#define\s+FC_ABI_VERSION\s+7\b", hdr)


def test_a_null_session_is_refused_by_the_library():
    lib = _lib.load()
    one = (ctypes.c_int32 * 1)(0)
    assert lib.fc_laura_slots_move(None, 1, one, one, None) != 0 and "null session" in _lib.last_error()
    assert lib.fc_laura_slots_set_elastic(None, 1) != 0 and "null session" in _lib.last_error()
    assert lib.fc_laura_slots_step_blocks(None) == 0


# ---- the compaction rule ------------------------------------------------------------------------------------------------------------
def test_compact_plan_already_compact():
    assert compact_plan([], 64) == []
    assert compact_plan([0, 1, 2], 64) == []
    assert compact_plan(range(16), 64) == []
    assert compact_plan([3, 15], 17) == []
    assert compact_plan(range(20), 33) == []                         # 20 rows need two blocks and lie in two


def test_compact_plan_one_straggler_in_the_top_block():
    assert compact_plan([0, 1, 2, 63], 64) == [(63, 3)]
    assert compact_plan([0, 2, 48], 64) == [(48, 1)]
    assert compact_plan(list(range(16)) + [40], 64) == [(40, 16)]    # 17 rows: two blocks instead of three, one move
    assert compact_plan([16], 17) == [(16, 0)]


def test_compact_plan_highest_rows_into_lowest_free_rows():
    assert compact_plan([17, 30, 33, 40], 64) == [(40, 0), (33, 1), (30, 2), (17, 3)]
    # the fewest moves: rows that already lie under the new top stay where they are
    assert compact_plan([1, 5, 20, 47], 64) == [(47, 0), (20, 2)]
    assert compact_plan(list(range(4, 18)) + [35, 50], 64) == [(50, 0), (35, 1), (17, 2), (16, 3)]
    assert compact_plan(list(range(0, 64, 2)), 64) == [(62 - 2 * i, 1 + 2 * i) for i in range(16)]      # every other row: four blocks into two


def test_compact_plan_nothing_to_gain():
    assert compact_plan(list(range(16)) + [16], 64) == []            # 17 rows in two blocks
    assert compact_plan(list(range(0, 34)), 64) == []
    assert compact_plan([0, 16, 32], 33, held=[r for r in range(16) if r]) == [(32, 17)]     # block 0 has no room: two blocks is the best
    assert compact_plan([0, 16], 33, held=[r for r in range(16) if r]) == []


def test_compact_plan_S_not_a_multiple_of_16():
    assert compact_plan([32], 33) == [(32, 0)]
    assert compact_plan(list(range(15)) + [16], 17) == [(16, 15)]
    assert compact_plan(list(range(16)) + [32], 33) == [(32, 16)]
    assert compact_plan(list(range(17, 33)), 33) == [(32 - i, i) for i in range(16)]
    with pytest.raises(ValueError, match="outside 0 .. 32"):
        compact_plan([33], 33)


def test_compact_plan_every_row_busy():
    for S in (16, 17, 33, 64):
        assert compact_plan(range(S), S) == []


def test_compact_plan_held_rows_are_no_destination_and_hold_nothing_up():
    assert compact_plan([20], 33, held=[0, 1, 32]) == [(20, 2)]
    assert compact_plan([3], 64, held=[63]) == []                    # an ended row in the top block does not hold the width up
    plan = compact_plan([40, 41], 64, held=range(0, 15))
    assert plan == [(41, 15), (40, 16)]                              # one free row in block 0: two blocks


def test_a_plan_is_a_legal_move():
    """sources busy, destinations free, all distinct, and the block count falls"""
    import random
    rnd = random.Random(5)
    for _ in range(300):
        S = rnd.choice([17, 20, 33, 48, 64])
        rows = list(range(S))
        rnd.shuffle(rows)
        nb, nh = rnd.randrange(0, S + 1), rnd.randrange(0, 8)
        busy, held = rows[:nb], rows[nb: nb + nh]
        plan = compact_plan(busy, S, held)
        srcs, dsts = [a for a, _ in plan], [b for _, b in plan]
        assert len(set(srcs + dsts)) == 2 * len(plan)
        assert set(srcs) <= set(busy) and not set(dsts) & (set(busy) | set(held))
        if plan:
            after = (set(busy) - set(srcs)) | set(dsts)
            assert max(after) // 16 < max(busy) // 16
            assert srcs == sorted(srcs, reverse=True) and dsts == sorted(dsts)


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_row_table():
    t = RowTable(20)
    assert [t.place(s) for s in (7, 19, 3)] == [(0, True), (1, True), (2, True)]       # the lowest free row, whatever the slot
    assert t.place(19) == (1, False)
    t.release(7)
    assert t.place(0) == (0, True) and t.free_rows()[0] == 3
    t.moved([(2, 10), (5, 6)])                                                          # row 5 holds nothing: no entry changes
    assert t.row == {19: 1, 3: 10, 0: 0} and t.slot_of() == {1: 19, 10: 3, 0: 0}


class Lib:
    """the library as an ElasticSlots sees it when it is opened and asked for its blocks"""
    blocks = 0

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def call(*args):
            self.log.append(name)
            return self.blocks if name == "fc_laura_slots_step_blocks" else 0
        return call


class Under:
    """The session underneath, in ROWS: what DecodeSlots' own methods do, without a device.  A row runs until `end` names it."""

    def __init__(self):
        self.state, self.calls, self.end = {}, [], set()

    def install(self, monkeypatch):
        u = self

        def start(self, row, *a, **k):
            if k.get("refuse"):
                raise EngineError(f"decoding session: slot {row}: refused")
            u.calls.append(("start", row))
            u.state[row] = "running"

        def start_many(self, reqs):
            u.calls.append(("start_many", [row for row, _ in reqs]))
            for row, _ in reqs:
                u.state[row] = "running"

        def start_from(self, dst, src, *a, source=None, **k):
            held = self if source is None else source
            u.calls.append(("start_from", dst, held._phys(src)))       # as DecodeSlots.start_from: the source's row through ITS table
            u.state[dst] = "running"

        def fork(self, dst, src, *a, **k):
            u.calls.append(("fork", dst, self._phys(src)))
            u.state[dst] = "running"

        def step(self, n=16):
            u.calls.append(("step", n))
            for row in u.end:
                if u.state.get(row) == "running":
                    u.state[row] = "done"
            return dict(u.state)

        def take(self, row, return_logp=False, return_score=False):
            assert u.state[row] == "done" and not return_score
            del u.state[row]
            return ("tokens of row", row)

        def move(self, pairs):
            u.calls.append(("move", list(pairs)))
            for a, b in pairs:
                assert a in u.state and b not in u.state
                u.state[b] = u.state.pop(a)
            self.moves += len(pairs)

        for f in (start, start_many, start_from, fork, step, take, move):
            monkeypatch.setattr(DecodeSlots, f.__name__, f)
        monkeypatch.setattr(DecodeSlots, "n_gen", lambda self, row: 100 + row)
        monkeypatch.setattr(DecodeSlots, "score_row", lambda self, row: ("score row of", row))
        monkeypatch.setattr(DecodeSlots, "_open", DecodeSlots._open.__wrapped__)
        monkeypatch.setattr(DecodeSlots, "free", lambda self: None)


def elastic(slots, **kw):
    lib = Lib()
    eng = types.SimpleNamespace(lib=lib, device="cpu", max_positions=64, _h=ctypes.c_void_p(1), _check=lambda rc: None)
    s = ElasticSlots(eng, slots, wide=slots > 16, **kw)
    s._h = ctypes.c_void_p(1)
    return s, lib


def test_the_table_through_a_stand_in_session(monkeypatch):
    u = Under()
    u.install(monkeypatch)
    s, lib = elastic(33, logp=False)
    assert lib.log == ["fc_laura_slots_state_bytes_wide", "fc_laura_slots_create_wide", "fc_laura_slots_set_elastic"]
    s.start(30, "text", 3)
    s.start_many({12: dict(text_outs="t", text_len=1), 31: dict(text_outs="t", text_len=1)})
    s.start_from(5, 30)
    s.fork(32, 12)
    assert s.rows() == {30: 0, 12: 1, 31: 2, 5: 3, 32: 4}                # the lowest free row, in the order of starting
    assert u.calls == [("start", 0), ("start_many", [1, 2]), ("start_from", 3, 0), ("fork", 4, 1)]
    s.rewind(31, 0)                                                       # in place: the slot keeps its row
    assert u.calls[-1] == ("fork", 2, 2) and s.rows()[31] == 2
    lib.blocks = 1
    assert s.step(2) == {30: "running", 12: "running", 31: "running", 5: "running", 32: "running"}
    assert s.blocks == 1 and s.blocks_hist == {1: 2} and s.moves == 0
    assert s.n_gen(5) == 103 and s.score_row(32) == ("score row of", 4)
    u.end = {0, 3}
    assert s.step(1) == {30: "done", 12: "running", 31: "running", 5: "done", 32: "running"}
    assert s.take(30) == ("tokens of row", 0) and s.take(5) == ("tokens of row", 3)
    assert s.rows() == {12: 1, 31: 2, 32: 4}                              # take frees the row; the others stay where they are
    s.start(9, "text", 3)
    assert s.rows()[9] == 0                                               # the lowest free row again
    with pytest.raises(EngineError, match=r"slot 30 holds no utterance"):
        s.take(30)
    with pytest.raises(EngineError, match=r"slot 33 outside 0 \.\. 32"):
        s.start(33, "text", 3)
    with pytest.raises(EngineError, match=r"slot 20 \(row 3\): decoding session: slot 3: refused"):
        s.start(20, "text", 3, refuse=True)
    assert 20 not in s.rows()                                             # a refused start takes no row
    with pytest.raises(EngineError, match="slot 4 holds no utterance"):
        s.start_from(6, 4)
    assert 6 not in s.rows()


def test_step_compacts_and_the_slots_keep_their_numbers(monkeypatch):
    u = Under()
    u.install(monkeypatch)
    s, lib = elastic(33, logp=False)
    for i in range(0, 32, 16):
        s.start_many({j: dict(text_outs="t", text_len=1) for j in range(i, i + 16)})
    s.start(32, "text", 3)
    assert s.rows() == {i: i for i in range(33)}
    lib.blocks = 3
    u.end = set(range(15)) | {20}
    s.step(1)
    assert s.moves == 0 and not [c for c in u.calls if c[0] == "move"]    # ended rows that are not taken are no destination
    for i in range(15):
        s.take(i)
    u.end = set()
    lib.blocks = 2
    st = s.step(1)                                                        # 17 rows run (15, 16 .. 19, 21 .. 32): two blocks, row 32 moves
    assert u.calls[-2:] == [("move", [(32, 0)]), ("step", 1)] and s.moves == 1
    assert s.rows()[32] == 0 and st[32] == "running" and st[20] == "done"
    assert s.blocks_hist == {3: 1, 2: 1}
    s.take(20)
    u.end = set(range(21, 32))
    s.step(1)
    for i in range(21, 32):
        s.take(i)
    lib.blocks = 1
    st = s.step(1)                                                        # 6 rows run: 0 (slot 32), 15 .. 19 -> one block, four moves
    assert u.calls[-2] == ("move", [(19, 1), (18, 2), (17, 3), (16, 4)])
    assert s.rows() == {15: 15, 16: 4, 17: 3, 18: 2, 19: 1, 32: 0} and s.moves == 5
    assert st == {i: "running" for i in (15, 16, 17, 18, 19, 32)}
    s.start_from(7, 19)                                                   # a slot's number follows it through the moves
    assert u.calls[-1] == ("start_from", 5, 1) and s.rows()[7] == 5


def test_a_session_used_as_a_source_translates_its_own_slots(monkeypatch):
    u = Under()
    u.install(monkeypatch)
    held, _ = elastic(4, logp=False)
    held.start(3, "text", 3)
    plain = DecodeSlots.__new__(DecodeSlots)
    plain.slots = 8
    plain.start_from(6, 3, source=held)
    assert u.calls[-1] == ("start_from", 6, 0)                            # slot 3 of the elastic source lies in its row 0
    assert DecodeSlots._phys(plain, 5) == 5


def test_elastic_is_inert_up_to_16_slots_and_needs_wide_above(monkeypatch):
    monkeypatch.setattr(DecodeSlots, "_open", DecodeSlots._open.__wrapped__)
    monkeypatch.setattr(DecodeSlots, "free", lambda self: None)
    s, lib = elastic(16, logp=False)
    assert lib.log == ["fc_laura_slots_state_bytes", "fc_laura_slots_create", "fc_laura_slots_set_elastic"]
    assert compact_plan(range(3, 16), 16) == []                           # one block: nothing to plan, whatever runs


# ---- the keywords -------------------------------------------------------------------------------------------------------------------
def test_open_decode_passes_elastic_on_and_refuses_a_queue():
    seen = []

    class Eng:
        open_decode = LauraEngine.open_decode

    class Model:
        open_decode = LauraGenMI355X.open_decode

    real = laura.ElasticSlots
    laura.ElasticSlots = lambda *a: seen.append(a[1:]) or "elastic session"
    try:
        m = Model()
        m.engine = Eng()
        assert m.open_decode(33, 64, False, True, wide=True, elastic=True) == "elastic session"
        assert m.open_decode(4, elastic=True) == "elastic session"
        for kw in (dict(queue=8, source="held"), dict(queue=8), dict(source="held")):
            with pytest.raises(EngineError, match="elastic=True is refused with queue=.*cannot know the busy rows"):
                m.open_decode(4, logp=False, elastic=True, **kw)
    finally:
        laura.ElasticSlots = real
    assert seen == [(33, 64, False, True, True), (4, None, True, False, False)]


class Stop(Exception):
    pass


def t2a_asking(asked):
    from funcodec_amd.bin.text2audio_inference import Text2Audio

    class Model:
        predict_nq = 2

        def open_decode(self, n, **kw):
            asked.append((n, kw))
            raise Stop

    t2a = Text2Audio.__new__(Text2Audio)
    t2a.model, t2a.continual = Model(), False
    return t2a


@pytest.mark.parametrize("slots,keep,want", [(4, "all", dict(logp=False, elastic=True)), (20, "all", dict(logp=False, wide=True, elastic=True)),
                                             (64, "best", dict(logp=False, score=True, wide=True, elastic=True))])
def test_generate_many_opens_the_main_session_elastic(slots, keep, want):
    asked = []
    with pytest.raises(Stop):
        t2a_asking(asked).generate_many(["a", "b"], slots=slots, seeds=[1, 2], keep=keep, elastic=True)
    assert asked == [(slots, want)]
    asked = []
    with pytest.raises(Stop):
        t2a_asking(asked).generate_many(["a", "b"], slots=slots, seeds=[1, 2], keep=keep)
    assert asked == [(slots, {k: v for k, v in want.items() if k != "elastic"})]


def test_generate_many_refuses_elastic_with_a_queue():
    asked = []
    with pytest.raises(ValueError, match="elastic=True is refused with queue=True.*cannot know the busy rows"):
        t2a_asking(asked).generate_many(["a"], slots=20, prefill=4, queue=True, elastic=True)
    assert asked == []
