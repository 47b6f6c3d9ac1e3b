"""CPU tests of the per-row bit rate (fc_engine_set_row_nq and the wrappers' ``bit_width`` / ``n_q`` per row): the C-ABI surface and the
refusals, all of which come before any engine call (there is no GPU here)."""
import ctypes
import os
import re

import pytest
import torch

from funcodec_amd import _lib
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.engine import EngineError, row_nq_list, row_nq_refusal
from funcodec_amd.model import EncodecMI355X
from funcodec_amd.stream import CodecStream, StreamSlots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "funcodec_amd.h")) as f:
        return f.read()


def test_entry_point_is_declared_bound_and_exported():
    hdr = _header()
    m = re.search(r"\bint\s+fc_engine_set_row_nq\s*\(([^;]*)\)\s*;", hdr)
    assert m, "fc_engine_set_row_nq is not declared in include/funcodec_amd.h"
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    assert "fc_engine_set_row_nq" in _lib.SYMBOLS
    res, args = _lib.SYMBOLS["fc_engine_set_row_nq"]
    assert res is ctypes.c_int and len(args) == len(params) == 4, (params, args)
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "fc_engine_set_row_nq")
    # the two session symbol sets are pinned by their own tests: the new name belongs to neither
    assert not "fc_engine_set_row_nq".startswith(("fc_stream_", "fc_slots_"))


def test_abi_version_stays_7():
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", _header())
    assert _lib.FC_ABI_VERSION == 7 and _lib.load().fc_abi_version() == 7


def test_null_engine_is_refused():
    lib = _lib.load()
    rows = (ctypes.c_int32 * 2)(1, 2)
    assert lib.fc_engine_set_row_nq(None, rows, 2, None) != 0
    assert b"null engine" in lib.fc_last_error()


class _NoEngineCall:
    """stands in for the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the refusal must come before any engine call")


def _model(cfg_name):
    m = EncodecMI355X(arch_from_config(recipe_config(cfg_name)), "cuda:0")
    real = m.engine.lib
    m.engine.lib = _NoEngineCall()
    return m, real


@pytest.fixture
def tiny():
    m, real = _model("tiny")
    yield m
    m.engine.lib = real          # the engine's destructor frees the handle through it


def test_row_nq_list_rules():
    arch = arch_from_config(recipe_config("tiny"))          # 6 quantisers
    assert row_nq_list(arch, [1, 6, 2], 3) == [1, 6, 2]
    assert row_nq_list(arch, torch.tensor([3, 4]), 2) == [3, 4]
    assert row_nq_list(arch, (2, 2), 2, cap=2) == [2, 2]
    for rows, B, cap in (([1, 2], 3, None), ([1, 2, 3, 4], 3, None), ([0, 1, 2], 3, None), ([1, 7, 2], 3, None), ([1, 3], 2, 2),
                         ([1.5, 2], 2, None), ([True, 2], 2, None), (torch.ones(2, 2), 2, None)):
        with pytest.raises(EngineError):
            row_nq_list(arch, rows, B, cap)


def test_one_bit_width_for_the_batch_is_still_one_value(tiny):
    """numbers of any kind and 0-dim tensors / arrays are the reference's single bit_width; sequences, tensors and arrays are per row"""
    import numpy as np
    for bw in (24000, 24000.0, np.float32(24000), np.int64(24000), torch.tensor(24000.0), np.array(24000.0)):
        assert tiny._bit_widths(bw, 3) == (2, None), type(bw)
    assert tiny._bit_widths(None, 3) == (6, None)
    for bw in ([12000, 24000, 36000], np.array([12000.0, 24000.0, 36000.0]), torch.tensor([12000.0, 24000.0, 36000.0])):
        assert tiny._bit_widths(bw, 3) == (3, [1, 2, 3]), type(bw)
    with pytest.raises(EngineError, match="1-D"):
        tiny._bit_widths(np.ones((3, 1)), 3)


def test_offline_wrappers_refuse_before_any_engine_call(tiny):
    wav = torch.zeros(3, 64)
    bw = 12000.0                                             # one tiny quantiser: log2(64) * 16000 / 8 bits per second
    for call in (tiny.inference, tiny.inference_encoding):
        with pytest.raises(EngineError, match="one entry per row"):
            call(wav, bit_width=[bw, 2 * bw])
        with pytest.raises(EngineError, match="one entry per row"):
            call(wav, bit_width=torch.tensor([bw] * 4))
        with pytest.raises(EngineError, match="1-D tensor"):
            call(wav, bit_width=torch.full((3, 1), bw))
    tok = torch.zeros(3, 5, 4, dtype=torch.long)             # 4 stages in the tokens: a row may not ask for 5
    with pytest.raises(EngineError, match="one entry per row"):
        tiny.inference_decoding(tok, bit_width=[bw, bw])
    with pytest.raises(EngineError, match=r"row 1: a stage count lies in \[1, 4\]"):
        tiny.inference_decoding(tok, bit_width=[bw, 5 * bw, bw])
    eng = tiny.engine
    for rows in ([1, 2], [1, 2, 0], [1, 2, 7], [1, 2, 4]):   # the call's n_q (3) is the cap
        with pytest.raises(EngineError):
            eng.encode(wav, 3, n_q_rows=rows)
        with pytest.raises(EngineError):
            eng.encode_decode(wav, 3, n_q_rows=rows)
    with pytest.raises(EngineError):
        eng.decode_codes(tok, n_q_rows=[1, 5, 1])
    with pytest.raises(EngineError, match="utterances of equal length"):
        eng.rvq_encode(torch.zeros(10, 16), 6, n_q_rows=[1, 2, 3])


@pytest.mark.parametrize("cfg_name,key", [("ds320seg", "model_conf.segment_dur"), ("tinybypass", "model_conf.bypass_quantizer"),
                                          ("tinybypassseg", "model_conf.segment_dur")])
def test_segmented_and_bypass_configurations_are_refused_by_name(cfg_name, key):
    arch = arch_from_config(recipe_config(cfg_name))
    assert key in row_nq_refusal(arch)
    m, real = _model(cfg_name)
    try:
        wav = torch.zeros(2, 64)
        for call in (m.inference, m.inference_encoding):
            with pytest.raises(EngineError, match=re.escape(key)):
                call(wav, bit_width=[12000.0, 24000.0])
        with pytest.raises(EngineError, match=re.escape(key)):
            m.inference_decoding(torch.zeros(2, 5, 6, dtype=torch.long), bit_width=[12000.0, 24000.0])
        with pytest.raises(EngineError, match=re.escape(key)):
            m.engine.encode(wav, 6, n_q_rows=[1, 2])
    finally:
        m.engine.lib = real
    assert row_nq_refusal(arch_from_config(recipe_config("tiny"))) is None


def test_open_stream_refuses_a_bad_list_before_anything_is_opened():
    m, real = _model("tinywn")
    try:
        for n_q in ([1, 2], [1, 2, 3, 4], [1, 0, 2], [1, 7, 2]):
            with pytest.raises(EngineError):
                m.open_stream(3, n_q=n_q)
    finally:
        m.engine.lib = real


def _bare(cls, arch, n_q, rows):
    """a session object without its library session (no GPU here): what set_n_q / start look at"""
    s = cls.__new__(cls)
    s._h, s.arch, s.n_q = None, arch, n_q
    if cls is CodecStream:
        s.batch, s._row_nq = rows, None
    else:
        s.slots, s._row_nq = rows, [n_q] * rows
        from funcodec_amd.stream import _Side
        s._enc, s._dec = [_Side() for _ in range(rows)], [_Side() for _ in range(rows)]
        s._scale, s._poisoned = [1.0] * rows, [False] * rows
    return s


def test_a_refused_set_n_q_changes_nothing():
    arch = arch_from_config(recipe_config("tinyss"))
    cs = _bare(CodecStream, arch, 4, 3)
    cs.set_n_q([1, 4, 2])
    assert cs._row_nq == [1, 4, 2] and cs._push_row_nq() == [1, 4, 2]
    for rows in ([1, 2], [1, 5, 2], [0, 1, 1], [1, 2, 3, 4]):
        with pytest.raises(EngineError):
            cs.set_n_q(rows)
        assert cs._row_nq == [1, 4, 2]
    cs.set_n_q([4, 4, 4])
    assert cs._push_row_nq() is None                         # every row at the cap: nothing is set on the engine

    ss = _bare(StreamSlots, arch, 5, 3)
    assert ss._push_row_nq() is None
    ss.set_n_q(1, 2)
    ss.start(2, scale=0.5, n_q=3)
    assert ss._row_nq == [5, 2, 3] and ss._scale[2] == 0.5
    ss._enc[0].started = True
    for bad in (0, 6, 2.5):
        with pytest.raises(EngineError):
            ss.set_n_q(0, bad)
        with pytest.raises(EngineError):
            ss.start(0, scale=0.25, n_q=bad)
    with pytest.raises(EngineError):
        ss.set_n_q(3, 1)                                     # no such slot
    assert ss._row_nq == [5, 2, 3] and ss._enc[0].started and ss._scale[0] == 1.0
    ss.start(1)                                              # None: the cap
    assert ss._row_nq == [5, 5, 3]
