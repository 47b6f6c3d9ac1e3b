"""Queued decoding sessions (fc_laura_slots_create_queued / _submit / _queue_status / _collect, open_decode(queue=, source=),
generate_many(queue=True)), the parts that need no device: the rule for which held rows may be refilled and the driver around it, the
C ABI's declarations and the binding's argument types, and the argument checks that come before any library call."""
import ctypes
import os
import re
import types

import pytest

from funcodec_amd import _lib
from funcodec_amd.engine import EngineError
from funcodec_amd.laura import DecodeSlots, drive_queue, queue_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fc_laura_slots_state_bytes_queued": 5, "fc_laura_slots_create_queued": 9, "fc_laura_slots_submit": 14,
         "fc_laura_slots_queue_status": 7, "fc_laura_slots_collect": 10}


# the refill rule -------------------------------------------------------------------------------------------------------------
def test_queue_rows_is_a_plain_function_of_the_claim_count():
    assert queue_rows({}, 0, 4) == [0, 1, 2, 3]
    held = {0: 2, 1: 4, 3: 6}                          # row -> the number behind its last ticket
    assert queue_rows(held, 0, 4) == [2]
    assert queue_rows(held, 1, 4) == [2], "ticket 1 of row 0 still waits"
    assert queue_rows(held, 2, 4) == [0, 2]
    assert queue_rows(held, 5, 4) == [0, 1, 2], "ticket 5 of row 3 still waits"
    assert queue_rows(held, 6, 4) == [0, 1, 2, 3]
    assert queue_rows(held, 2, 4) == queue_rows(dict(held), 2, 4) and held == {0: 2, 1: 4, 3: 6}, "nothing is kept or changed"
    for bad in (lambda: queue_rows({}, 0, 0), lambda: queue_rows({}, -1, 2), lambda: queue_rows({2: 1}, 0, 2), lambda: queue_rows({0: -1}, 0, 2)):
        with pytest.raises(ValueError, match="queue_rows"):
            bad()


class FakeQueued:
    """A queued session of S slots as drive_queue sees it: tickets are claimed in order by free slots at the head of every step, a
    ticket runs `length(ticket)` steps; it records which row every claim read and whether that row still held the ticket's request."""

    def __init__(self, S, length):
        self.S, self.slots, self.length = S, S, length
        self.claimed, self.waiting, self.running, self.done = 0, [], {}, []
        self.steps, self.calls = 0, []

    def submit(self, ticket):
        self.waiting.append(ticket)

    def slot_tickets(self):
        return {slot: r[0] for slot, r in self.running.items()}

    def step(self, n):
        self.calls.append(n)
        for _ in range(n):
            if not self.waiting and not self.running:
                break
            self.steps += 1
            for slot in range(self.S):
                if slot in self.running and self.running[slot][1] == 0:
                    self.done.append(self.running.pop(slot)[0])
                if slot not in self.running and self.waiting:
                    t = self.waiting.pop(0)
                    self.on_claim(t)
                    self.running[slot] = [t, self.length(t)]
                    self.claimed += 1
            for slot in self.running:
                self.running[slot][1] = max(0, self.running[slot][1] - 1)
        for slot in [s for s in self.running if self.running[s][1] == 0]:       # retired before the read-back
            self.done.append(self.running.pop(slot)[0])
        return {}

    def collect(self):
        out, self.done = [(t, ("tokens", t), 1, None) for t in self.done], []
        return out


@pytest.mark.parametrize("S,rows,n,N", [(2, 4, 9, 1), (3, 2, 5, 2), (16, 4, 9, 2), (1, 1, 3, 2), (4, 16, 5, 1)])
def test_drive_queue_never_refills_a_row_before_its_tickets_are_claimed(S, rows, n, N):
    row_holds, ticket_of, fills = {}, {}, []
    sess = FakeQueued(S, lambda t: 1 + (7 * t) % 5)

    def on_claim(t):
        row, c = ticket_of[t]
        assert row_holds[row] == c // N, f"ticket {t} was claimed after row {row} had been refilled"
    sess.on_claim = on_claim

    def fill(batch):
        fills.append(batch)
        assert [r for r, _ in batch] == sorted(r for r, _ in batch)
        for row, q in batch:
            row_holds[row] = q

    def submit(row, c):
        t = len(ticket_of)
        ticket_of[t] = (row, c)
        sess.submit(t)
        return t

    out = drive_queue(sess, rows, n, N, fill, submit, step_n=4)
    assert [r[0] for r in out] == [("tokens", t) for t in range(n * N)], "candidate c is ticket c: arrival order"
    assert [q for b in fills for _, q in b] == list(range(n)), "every request is prefilled once, in arrival order"
    assert len(fills[0]) == min(rows, n)
    if S >= 2 * rows * N and n > 2 * rows:          # the slots can take two fills' tickets, and more requests are left
        assert sess.calls[:2] == [1, 1], "a session wider than the holding session is filled step by step"


def test_drive_queue_raises_on_a_failed_ticket():
    class Failing(FakeQueued):
        def collect(self):
            return [(t, None, 0, None) for t in self.done]
    sess = Failing(1, lambda t: 1)
    sess.on_claim = lambda t: None
    with pytest.raises(EngineError, match="ticket 0 failed"):
        drive_queue(sess, 1, 1, 1, lambda batch: None, lambda row, c: sess.submit(c) or c)


# the C ABI -------------------------------------------------------------------------------------------------------------------
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
        assert sect.index("fc_laura_slots_start_from_session(") < sect.index(name + "("), "additions behind the earlier calls"
    assert _lib.FC_ABI_VERSION == 7 and re.search(r"#define\s+FC_ABI_VERSION\s+7\b", hdr)


def test_null_arguments_are_refused_by_the_library():
    lib = _lib.load()
    assert lib.fc_laura_slots_state_bytes_queued(None, 4, 64, 0, 8) == 0
    h, t, n = ctypes.c_void_p(), ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert lib.fc_laura_slots_create_queued(None, 4, 64, 0, 8, None, None, 0, ctypes.byref(h)) != 0
    assert "null engine" in _lib.last_error()
    assert lib.fc_laura_slots_submit(None, 0, 5, 1, 0, 0.0, 1, 1.0, 0, 0.0, 0, 1, ctypes.byref(t), None) != 0 and t.value == -1
    assert "null session" in _lib.last_error()
    assert lib.fc_laura_slots_queue_status(None, None, None, None, None, None, None) != 0
    assert lib.fc_laura_slots_collect(None, 0, None, None, None, None, None, None, None, ctypes.byref(n)) != 0 and n.value == -1


# the binding's own checks ----------------------------------------------------------------------------------------------------
class Calls:
    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def call(*args):
            self.log.append((name, args[1:5]))
            return 0
        return call


def stub_engine():
    lib = Calls()
    # "cuda:0": the calls below are bracketed by the engine's device where there is one; nothing is ever allocated on it
    return types.SimpleNamespace(lib=lib, device="cuda:0", max_positions=64, _h=ctypes.c_void_p(1), _check=lambda rc: None), lib


@pytest.fixture
def opened(monkeypatch):
    monkeypatch.setattr(DecodeSlots, "_open", DecodeSlots._open.__wrapped__)
    monkeypatch.setattr(DecodeSlots, "free", lambda self: None)


def test_open_decode_checks_a_queue_before_any_call(opened):
    eng, lib = stub_engine()
    held = DecodeSlots(eng, 4, logp=False)
    other, _ = stub_engine()
    foreign = DecodeSlots(other, 4, logp=False)
    held._h = foreign._h = ctypes.c_void_p(2)          # the stub's create hands no handle out
    n = len(lib.log)
    for kw, why in ((dict(logp=True, queue=8, source=held), "queue= needs logp=False"),
                    (dict(logp=False, queue=8), "queue= needs source="),
                    (dict(logp=False, source=held), "source= goes with queue="),
                    (dict(logp=False, queue=8, source=foreign), "another engine"),
                    (dict(logp=False, queue=0, source=held), r"queue must be 1 \.\. 65536"),
                    (dict(logp=False, queue=65537, source=held), r"queue must be 1 \.\. 65536")):
        with pytest.raises(EngineError, match=why):
            DecodeSlots(eng, 2, **kw)
    with pytest.raises(EngineError, match=r"decoding session has 1 \.\. 16 slots, got 17"):
        DecodeSlots(eng, 17, logp=False, queue=8, source=held)
    with pytest.raises(EngineError, match=r"wide decoding session has 1 \.\. 64 slots, got 65"):
        DecodeSlots(eng, 65, logp=False, wide=True, queue=8, source=held)
    assert len(lib.log) == n, "refused before any library call"
    qs = DecodeSlots(eng, 17, logp=False, score=True, wide=True, queue=8, source=held)
    assert [c[0] for c in lib.log[n:]] == ["fc_laura_slots_state_bytes_queued", "fc_laura_slots_create_queued"]
    assert lib.log[n][1] == (17, 64, 1, 8) and lib.log[n + 1][1] == (17, 64, 1, 8)
    with pytest.raises(EngineError, match="itself queued"):
        DecodeSlots(eng, 2, logp=False, queue=8, source=qs)
    # a session without a queue opens through the calls it always did, and has no queue calls
    assert qs.queue == 8 and held.queue is None
    for call in (lambda: held.submit(0), lambda: held.collect(), lambda: held.claimed, lambda: held.pending):
        with pytest.raises(EngineError, match="opened without a queue"):
            call()
    # a queued session refuses the calls that put a prompt into a slot or take one out, before it touches anything
    n = len(lib.log)
    for name, call in (("start", lambda: qs.start(0, None, 1)), ("start_many", lambda: qs.start_many({})),
                       ("start_from", lambda: qs.start_from(0, 1)), ("start_from", lambda: qs.start_from(0, 1, source=held)),
                       ("fork", lambda: qs.fork(0, 1)), ("rewind", lambda: qs.rewind(0, 1)), ("take", lambda: qs.take(0)),
                       ("score_row", lambda: qs.score_row(0))):
        with pytest.raises(EngineError, match=name + ": a queued session is fed by its queue only"):
            call()
    assert len(lib.log) == n


def test_generate_many_checks_queue_before_anything_runs():
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    t2a = Text2Audio.__new__(Text2Audio)
    t2a.model = type("M", (), {"predict_nq": 2})()
    with pytest.raises(ValueError, match="queue=True needs prefill >= 1"):
        t2a.generate_many(["a"], slots=4, queue=True)
    with pytest.raises(ValueError, match="queue=True goes with retries = 0, got 2"):
        t2a.generate_many(["a"], slots=4, prefill=4, queue=True, retries=2)


class Stop(Exception):
    pass


@pytest.mark.parametrize("slots,keep,samples", [(4, "all", 1), (17, "best", 3)])
def test_generate_many_opens_the_holding_session_and_a_queued_one_on_it(slots, keep, samples):
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    asked = []

    class Held:
        freed = 0

        def free(self):
            Held.freed += 1

    class Model:
        predict_nq = 2

        def open_decode(self, n, **kw):
            asked.append((n, kw))
            if len(asked) == 2:
                raise Stop
            return Held()

    t2a = Text2Audio.__new__(Text2Audio)
    t2a.model, t2a.continual = Model(), False
    with pytest.raises(Stop):
        t2a.generate_many(["a", "b"], slots=slots, seeds=[[1] * samples, [2] * samples] if samples > 1 else [1, 2], keep=keep,
                          samples=samples, prefill=8, queue=True)
    assert asked[0] == (8, dict(logp=False))
    want = dict(logp=False, queue=slots + 8 * samples)
    if keep == "best":
        want["score"] = True
    if slots > 16:
        want["wide"] = True
    source = asked[1][1].pop("source")
    assert isinstance(source, Held) and asked[1] == (slots, want) and Held.freed == 1
