"""Graph replay of session pushes, what can be checked without a GPU: the entry points are exported, declared and bound; the ABI version
stands; the wrapper's refusal is the library's; a session opened without graph=True constructs none of the fixed buffers."""
import ctypes as C
import os
import re
import types

import pytest

from funcodec_amd import _lib, build
from funcodec_amd import stream as fstream
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.engine import EngineError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fc_graphstream_set", "fc_graphstream_enabled", "fc_graphstream_counts", "fc_graphslots_set", "fc_graphslots_enabled", "fc_graphslots_counts"]


def test_the_six_entry_points_are_exported_declared_and_bound_and_the_abi_version_stands():
    header = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    lib = C.CDLL(build.LIB_PATH)
    for name in NEW:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), name
        assert getattr(lib, name) is not None
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[0] is C.c_void_p
    assert _lib.SYMBOLS["fc_graphstream_set"][1] == [C.c_void_p, C.c_int] == _lib.SYMBOLS["fc_graphslots_set"][1]
    assert _lib.SYMBOLS["fc_graphstream_counts"][1][1] == C.POINTER(C.c_int64) == _lib.SYMBOLS["fc_graphslots_counts"][1][1]
    assert re.search(r"#define FC_ABI_VERSION 7\b", header) and _lib.FC_ABI_VERSION == 7
    lib.fc_abi_version.restype = C.c_int
    assert lib.fc_abi_version() == 7


def test_null_sessions_are_refused_with_a_message_and_report_off():
    lib = _lib.load()
    out = (C.c_int64 * 4)()
    assert lib.fc_graphstream_set(None, 1) != 0 and "null" in _lib.last_error()
    assert lib.fc_graphslots_set(None, 1) != 0 and "null" in _lib.last_error()
    assert lib.fc_graphstream_counts(None, out) != 0 and lib.fc_graphslots_counts(None, out) != 0
    assert lib.fc_graphstream_enabled(None) == 0 and lib.fc_graphslots_enabled(None) == 0


def _model(name):
    arch = arch_from_config(recipe_config(name))
    return types.SimpleNamespace(arch=arch, engine=types.SimpleNamespace(lib=None, device="cpu", hop_length=8))


def test_the_wrappers_refusal_is_the_librarys_and_comes_before_anything_is_opened(monkeypatch):
    opened = []
    monkeypatch.setattr(fstream._Session, "_open", lambda self, rows, max_chunk: opened.append(rows))
    source = open(os.path.join(ROOT, "funcodec_amd", "csrc", "engine.hip")).read()
    said = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', source[source.index("int fc_graphstream_set("):source.index("int fc_graphstream_enabled(")]))
    assert fstream.GRAPH_MAX_FRAMES_REFUSAL in said and "max_frames" in fstream.GRAPH_MAX_FRAMES_REFUSAL and "slot session" in fstream.GRAPH_MAX_FRAMES_REFUSAL
    from test_seqstream_host import causal_tinytf
    m = types.SimpleNamespace(arch=arch_from_config(causal_tinytf()), engine=types.SimpleNamespace(lib=None, device="cpu", hop_length=8))
    with pytest.raises(EngineError) as ei:
        fstream.CodecStream(m, 1, max_frames=64, graph=True)
    assert str(ei.value) == fstream.GRAPH_MAX_FRAMES_REFUSAL and not opened
    # without max_frames the net's own refusal comes first, as ever
    with pytest.raises(EngineError, match="seq_model: transformer"):
        fstream.CodecStream(m, 1, graph=True)
    assert not opened


def test_a_session_without_graph_constructs_no_fixed_buffers(monkeypatch):
    made = []
    monkeypatch.setattr(fstream._Session, "_open", lambda self, rows, max_chunk: None)
    monkeypatch.setattr(fstream._Session, "_graph_open", lambda self, rows: made.append(rows))
    monkeypatch.setattr(fstream._GraphBuffers, "__init__", lambda self, *a: made.append("buffers"))
    st = fstream.StreamSlots(_model("tinywn"), 3)
    assert st._g is None and st.graph is False and not made
    assert isinstance(st._push_stream(), type(__import__("contextlib").nullcontext()))
    t = object()
    assert st._out(t) is t and st._given("wav_in", t) is t
    fstream.StreamSlots(_model("tinywn"), 3, graph=True)
    assert made == [3]
    import inspect
    from funcodec_amd.model import EncodecMI355X
    from funcodec_amd.bin.codec_inference import Speech2Token
    for fn in (EncodecMI355X.open_stream, EncodecMI355X.open_slots, Speech2Token.open_stream, Speech2Token.open_slots):
        assert inspect.signature(fn).parameters["graph"].default is False
