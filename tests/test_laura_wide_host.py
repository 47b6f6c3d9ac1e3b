"""Wide decoding sessions (fc_laura_slots_state_bytes_wide / fc_laura_slots_create_wide, open_decode(wide=True),
generate_many(slots > 16)), the parts that need no device: the C ABI's declarations and the binding's argument types, the slot-count
checks that come before any library call, and which sessions generate_many asks for."""
import ctypes
import os
import re
import types

import pytest

from funcodec_amd import _lib
from funcodec_amd.engine import EngineError
from funcodec_amd.laura import DecodeSlots, LauraEngine, LauraGenMI355X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fc_laura_slots_state_bytes_wide": 5, "fc_laura_slots_create_wide": 8}


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
    # pure additions, typed as the _scored pair: the earlier calls and the ABI version stay
    for wide, scored in (("fc_laura_slots_state_bytes_wide", "fc_laura_slots_state_bytes_scored"),
                         ("fc_laura_slots_create_wide", "fc_laura_slots_create_scored")):
        assert _lib.SYMBOLS[wide][0] is _lib.SYMBOLS[scored][0]
        assert _lib.SYMBOLS[wide][1] == _lib.SYMBOLS[scored][1]
        assert sect.index(scored + "(") < sect.index(wide + "(")
    assert _lib.FC_ABI_VERSION == 7 and re.search(r"#define\s+FC_ABI_VERSION\s+7\b", hdr)


def test_a_null_engine_is_refused_by_the_library():
    lib = _lib.load()
    assert lib.fc_laura_slots_state_bytes_wide(None, 33, 64, 0, 1) == 0
    h = ctypes.c_void_p()
    assert lib.fc_laura_slots_create_wide(None, 33, 64, 0, 0, None, 0, ctypes.byref(h)) != 0
    assert "null engine" in _lib.last_error()
    assert lib.fc_laura_slots_state_bytes_scored(None, 17, 64, 0, 1) == 0


class Calls:
    """the library as DecodeSlots._open sees it: every call is recorded, every state is 0 bytes and every create succeeds"""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def call(*args):
            self.log.append((name, args[1]))          # (entry point, slots)
            return 0
        return call


def stub_engine():
    lib = Calls()
    eng = types.SimpleNamespace(lib=lib, device="cpu", max_positions=64, _h=ctypes.c_void_p(1), _check=lambda rc: None)
    return eng, lib


@pytest.fixture
def opened(monkeypatch):
    """DecodeSlots._open without its device bracket: the library calls it makes, against the stub"""
    monkeypatch.setattr(DecodeSlots, "_open", DecodeSlots._open.__wrapped__)
    monkeypatch.setattr(DecodeSlots, "free", lambda self: None)


def test_wide_allows_1_to_64_and_is_checked_before_any_call():
    eng, lib = stub_engine()
    for bad in (0, -1, 65, 100):
        with pytest.raises(EngineError, match=r"wide decoding session has 1 \.\. 64 slots, got " + str(bad)):
            DecodeSlots(eng, bad, wide=True)
    assert lib.log == []
    assert (DecodeSlots.MAX_SLOTS, DecodeSlots.MAX_SLOTS_WIDE) == (16, 64)


def test_which_entry_points_a_session_opens_through(opened):
    def through(slots, **kw):
        eng, lib = stub_engine()
        DecodeSlots(eng, slots, **kw)
        return lib.log

    for n in (17, 33, 64):
        assert through(n, wide=True) == [("fc_laura_slots_state_bytes_wide", n), ("fc_laura_slots_create_wide", n)]
        assert through(n, wide=True, score=True) == [("fc_laura_slots_state_bytes_wide", n), ("fc_laura_slots_create_wide", n)]
    # up to 16 slots a wide session is the session without the flag, call for call
    for n in (1, 3, 16):
        assert through(n, wide=True) == through(n) == [("fc_laura_slots_state_bytes", n), ("fc_laura_slots_create", n)]
        assert through(n, wide=True, score=True) == through(n, score=True) == [("fc_laura_slots_state_bytes_scored", n),
                                                                                 ("fc_laura_slots_create_scored", n)]
    # without the flag 17 goes to the library as before, which refuses it
    assert through(17) == [("fc_laura_slots_state_bytes", 17), ("fc_laura_slots_create", 17)]


def test_open_decode_passes_wide_on():
    seen = []

    class Eng:
        open_decode = LauraEngine.open_decode

    class Model:
        open_decode = LauraGenMI355X.open_decode

    import funcodec_amd.laura as laura
    real = laura.DecodeSlots
    laura.DecodeSlots = lambda *a: seen.append(a[1:]) or "session"
    try:
        m = Model()
        m.engine = Eng()
        assert m.open_decode(33, 64, False, True, wide=True) == "session"
        assert m.open_decode(4) == "session"
    finally:
        laura.DecodeSlots = real
    assert seen == [(33, 64, False, True, True), (4, None, True, False, False)]


class Stop(Exception):
    pass


@pytest.mark.parametrize("slots,keep,want", [(4, "all", [dict(logp=False)]), (16, "best", [dict(logp=False, score=True)]),
                                             (17, "all", [dict(logp=False, wide=True)]), (64, "best", [dict(logp=False, score=True, wide=True)])])
def test_generate_many_opens_a_wide_session_above_16_slots(slots, keep, want):
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    asked = []

    class Model:
        predict_nq = 2

        def open_decode(self, n, **kw):
            asked.append((n, kw))
            raise Stop

    t2a = Text2Audio.__new__(Text2Audio)
    t2a.model, t2a.continual = Model(), False
    with pytest.raises(Stop):
        t2a.generate_many(["a", "b"], slots=slots, seeds=[1, 2], keep=keep)
    assert asked == [(slots, want[0])]


def test_generate_many_keeps_prefill_at_16_rows():
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    t2a = Text2Audio.__new__(Text2Audio)
    t2a.model = type("M", (), {"predict_nq": 2})()
    with pytest.raises(ValueError, match="prefill must be"):
        t2a.generate_many(["a"], slots=64, prefill=17)
