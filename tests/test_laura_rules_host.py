"""Per-slot sampling rules of a decoding session (fc_laura_slots_set_rules, funcodec_amd.laura.SamplingRules, the rules= keyword of
DecodeSlots.start / start_from / fork / rewind and of Text2Audio.generate_many), the parts that need no device: the ranges SamplingRules
accepts and refuses, the C ABI's declaration, the library's refusal of a null session, and that every call of the binding sets the
slot's rules ahead of the call that writes them."""
import ctypes
import inspect
import math
import os
import re

import pytest

from funcodec_amd import _lib
from funcodec_amd.laura import DecodeSlots, SamplingRules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fc_laura_slots_set_rules"


def test_the_defaults_are_the_neutral_rules():
    r = SamplingRules()
    assert (r.temperature, r.min_length, r.top_p, r.repeat_window, r.repeat_count) == (1.0, 0, None, 0, 1)
    assert r.args() == (1.0, 0, 0.0, 0, 1)


@pytest.mark.parametrize("kw,args", [
    (dict(temperature=0.5), (0.5, 0, 0.0, 0, 1)),
    (dict(temperature=1e-3, min_length=750), (1e-3, 750, 0.0, 0, 1)),
    (dict(top_p=1.0), (1.0, 0, 1.0, 0, 1)),
    (dict(top_p=1e-6), (1.0, 0, 1e-6, 0, 1)),
    (dict(repeat_window=1, repeat_count=1), (1.0, 0, 0.0, 1, 1)),
    (dict(repeat_window=256, repeat_count=256), (1.0, 0, 0.0, 256, 256)),
    (dict(temperature=2, min_length=3, top_p=0.8, repeat_window=32, repeat_count=2), (2.0, 3, 0.8, 32, 2)),
])
def test_the_ranges_are_accepted(kw, args):
    assert SamplingRules(**kw).args() == args


@pytest.mark.parametrize("kw,msg", [
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(temperature=math.inf), "temperature"),
    (dict(temperature=math.nan), "temperature"), (dict(temperature=1e-60), "temperature"), (dict(temperature=1e60), "temperature"),
    (dict(min_length=-1), "min_length"), (dict(min_length=1.5), "min_length"),
    (dict(top_p=0.0), "top_p"), (dict(top_p=-0.5), "top_p"), (dict(top_p=1.0001), "top_p"), (dict(top_p=math.nan), "top_p"),
    (dict(top_p=1e-60), "top_p"),
    (dict(repeat_window=-1), "repeat_window"), (dict(repeat_window=257), "repeat_window"), (dict(repeat_window=True), "repeat_window"),
    (dict(repeat_window=4, repeat_count=0), "repeat_count"), (dict(repeat_window=4, repeat_count=5), "repeat_count"),
    (dict(repeat_count=0), "repeat_count"),
])
def test_out_of_range_values_are_refused(kw, msg):
    with pytest.raises(ValueError, match=msg):
        SamplingRules(**kw)


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    start = hdr.index("typedef struct fc_laura_slots")
    sect = hdr[start: hdr.index("#ifdef __cplusplus", start)]
    m = re.search(r"\b" + NAME + r"\s*\(([^;]*?)\)\s*;", sect, re.S)
    assert m, f"{NAME} is not declared in the session's section of include/funcodec_amd.h"
    assert NAME in _lib.SYMBOLS
    assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SYMBOLS[NAME][1]) == 7
    assert hasattr(ctypes.CDLL(_lib.lib_path()), NAME), f"{NAME} is not exported"
    # a pure addition behind the scores; the semantics are stated there, once; the earlier calls and the ABI version stay
    assert sect.index("fc_laura_slots_score(") < sect.index(NAME + "(")
    own = sect[sect.index("fc_laura_slots_score("): sect.index(NAME + "(")]
    for word in ("temperature", "min_length", "top_p", "repeat_window", "repeat_count", "8 + k", "neutral"):
        assert word in own, word
    assert len(_lib.SYMBOLS["fc_laura_slots_start"][1]) == 15 and len(_lib.SYMBOLS["fc_laura_slots_start_from"][1]) == 10
    assert len(_lib.SYMBOLS["fc_laura_slots_fork"][1]) == 10
    assert _lib.FC_ABI_VERSION == 7 and re.search(r"#define\s+FC_ABI_VERSION\s+7\b", hdr)


def test_a_null_session_is_refused_by_the_library():
    lib = _lib.load()
    assert lib.fc_laura_slots_set_rules(None, 0, 1.0, 0, 0.0, 0, 1) != 0
    assert "null session" in _lib.last_error()


def test_every_call_takes_rules_and_sets_them_first():
    for name in ("start", "start_from", "fork", "rewind"):
        p = inspect.signature(getattr(DecodeSlots, name)).parameters
        assert "rules" in p and p["rules"].default is None, name
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    assert inspect.signature(Text2Audio.generate_many).parameters["rules"].default is None

    class Lib:
        def __init__(self):
            self.calls = []

        def fc_laura_slots_set_rules(self, h, slot, *a):
            self.calls.append(("set_rules", slot) + a)
            return 0

        def fc_laura_slots_fork(self, h, dst, src, *a):
            self.calls.append(("fork", dst, src))
            return 0

    s = DecodeSlots.__new__(DecodeSlots)
    s.lib, s.slots, s._h = Lib(), 4, ctypes.c_void_p(1)
    s.engine = type("E", (), {"_check": staticmethod(lambda rc: None), "_side": None})()
    s._max_length, s._n_gen = [8] * 4, (ctypes.c_int32 * 4)()
    stream = type("Stream", (), {"cuda_stream": 0})()
    s._run_stream = lambda: (stream, stream)
    s.device = None
    try:
        fork = getattr(DecodeSlots.fork, "__wrapped__", DecodeSlots.fork)      # without the decorator that makes the device current
        fork(s, 2, 1, 3, rules=SamplingRules(0.5, 2, None, 6, 2))
        fork(s, 3, 3, 1)                                                      # a rewind without rules: the neutral ones
        assert s.lib.calls == [("set_rules", 2, 0.5, 2, 0.0, 6, 2), ("fork", 2, 1), ("set_rules", 3, 1.0, 0, 0.0, 0, 1), ("fork", 3, 3)]
        with pytest.raises(ValueError, match="slot 1.*SamplingRules"):
            fork(s, 1, 0, 1, rules={"temperature": 0.5})
    finally:
        s._h = None                                                           # nothing to destroy
