"""CPU tests of the stage count per push chosen by a noise floor (fc_engine_set_floor, ``noise_floor_db=``): the host statement of the
push rule (``floor_pick``), the C-ABI surface, and the refusals that come before anything reaches the device.  No GPU is needed."""
import inspect
import os
import re

import numpy as np
import pytest

from funcodec_amd import _lib
from funcodec_amd.engine import CodecEngine, EngineError, floor_pick, floor_refusal, floor_value, floor_values, rate_min_nq
from funcodec_amd.model import EncodecMI355X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
ARCH_KW = dict(num_quantizers=6, codebook_dim=16, segment_length=None, bypass_quantizer=False, q0_ds_ratio=1)
ARCH = type("A", (), ARCH_KW)()
#          k =   0     1    2    3    4    5    6
CURVE = [[100.0, 40.0, 9.0, 4.0, 4.0, 1.0, 2.0]]


def _header():
    with open(os.path.join(ROOT, "include", "funcodec_amd.h")) as f:
        return f.read()


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def test_the_first_count_that_meets_the_floor():
    # thr = floor * frames: 5 * 2 = 10 -> the first E[k] <= 10 is k = 2
    assert floor_pick(CURVE, 2, 5.0, 1, 6).tolist() == [2]
    assert floor_pick(CURVE, 1, 5.0, 1, 6).tolist() == [3]             # half the frames, half the threshold: 4 <= 5
    assert floor_pick(CURVE, 2, 4.5, 1, 6).tolist() == [2]             # 9 <= 9: the comparison is <=
    assert floor_pick(CURVE, 2, 5.0, 3, 6).tolist() == [3]             # min_n_q holds a row up
    out = floor_pick(CURVE, 2, 5.0, 1, 6)
    assert out.dtype == np.int32 and out.shape == (1,)


def test_a_missed_floor_takes_the_argmin_first_on_ties():
    assert floor_pick(CURVE, 1, 0.5, 1, 6).tolist() == [5]             # nothing reaches 0.5: the smallest E, not the cap
    assert floor_pick(CURVE, 1, 0.5, 1, 4).tolist() == [3]             # E[3] == E[4]: the first
    assert floor_pick(CURVE, 1, 0.5, 4, 4).tolist() == [4]
    assert floor_pick(CURVE, 1, floor_value(ARCH, -INF), 1, 6).tolist() == [5]      # -inf dB: the best k
    assert floor_value(ARCH, -INF) == 0.0
    assert floor_pick([[3.0, 2.0, 0.0, 0.0]], 4, 0.0, 1, 3).tolist() == [2]         # an exact residual of 0 meets a floor of 0


def test_an_input_at_or_below_the_floor_takes_min_n_q():
    assert floor_pick(CURVE, 1, 100.0, 1, 6).tolist() == [1]           # E[0] <= thr, although E[1] < E[0]
    assert floor_pick(CURVE, 1, 100.0, 3, 6).tolist() == [3]
    assert floor_pick(CURVE, 4, 25.0, 2, 6).tolist() == [2]
    assert floor_pick([[0.0] * 7], 3, 1e-9, 2, 6).tolist() == [2]      # digital silence
    assert floor_pick([[0.0] * 7], 3, 0.0, 1, 6).tolist() == [1]
    assert floor_pick(CURVE, 1, floor_value(ARCH, INF), 2, 6).tolist() == [2] and floor_value(ARCH, INF) == INF      # +inf dB: always min_n_q


def test_a_row_that_is_not_finite_takes_its_cap():
    for bad in (NAN, INF):
        E = [list(CURVE[0])]
        E[0][4] = bad
        assert floor_pick(E, 1, 5.0, 1, 6).tolist() == [6]
        assert floor_pick(E, 1, 5.0, 1, 3).tolist() == [3]             # a NaN behind the cap is not looked at: 4 <= 5 at k = 3
        assert floor_pick(E, 1, INF, 1, 6).tolist() == [6]             # even under a floor of +inf
    assert floor_pick([[NAN] * 7], 1, 5.0, 1, 4).tolist() == [4]


def test_caps_floors_frames_per_row_and_idle_rows():
    E = np.array(CURVE * 5)
    got = floor_pick(E, [1, 1, 2, 0, 1], [5.0, 5.0, 5.0, 5.0, None], 1, [6, 2, 6, 6, 4])
    # row 1: the cap holds it down (nothing meets 5 in [1, 2]: the argmin); row 3 has no frame in the push: -1, its entry is left alone;
    # row 4 is switched off: its cap
    assert got.tolist() == [3, 2, 2, -1, 4]
    assert floor_pick(E, 1, 5.0, 9, [6, 2, 6, 6, 4]).tolist() == [6, 2, 6, 6, 4]        # min_n_q above a cap is clamped to it
    # the floor in dB: D * 10^(dB / 10) per element
    assert floor_value(ARCH, 0.0) == 16.0 and floor_value(ARCH, -10.0) == pytest.approx(1.6, rel=1e-15)
    assert floor_values(ARCH, -10.0, 3) == [floor_value(ARCH, -10.0)] * 3
    assert floor_values(ARCH, np.array([0.0, -INF]), 2) == [16.0, 0.0]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported():
    lib = _lib.load()
    text = _header()
    for name, nargs in {"fc_engine_set_floor": 6, "fc_engine_set_floor_form": 7}.items():
        assert hasattr(lib, name) and name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert re.search(r"\bint " + name + r"\(", text), name
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int fc_engine_set_floor\(", text, re.S)
    assert m and "csrc/rvq_rate_kernels.h" in m.group(1) and "THE PUSH RULE" in m.group(1)
    for word in ("fc_stream_encode", "fc_slots_encode", "fc_rvq_encode_rate", "session pushes only", "fc_engine_set_rate", "NaN", "q0_ds_ratio"):
        assert word in m.group(1), word
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", text) and _lib.FC_ABI_VERSION == 7 and lib.fc_abi_version() == 7
    with open(os.path.join(ROOT, "funcodec_amd", "csrc", "rvq_rate_kernels.h")) as f:
        rule = f.read()
    for word in ("THE PUSH RULE", "thr_b = floor_b * (double)F_b", "one IEEE double product, no division", "E_b[0] <= thr_b takes lo",
                 "first on ties", "neither read nor written", "stateless", "launch_rvq_push_floor", "at most 256 frames"):
        assert word in rule, word
    from funcodec_amd import build
    assert "rvq_rate_kernels.hip" in build.sources() and "rvq_rate_kernels.h" in build.HEADERS
    # a null engine is refused by name, nothing is touched
    assert lib.fc_engine_set_floor(None, None, 0, 1, None, None) != 0 and "engine" in _lib.last_error()
    assert lib.fc_engine_set_floor_form(None, 0, None, None, None, None, None) != 0 and "engine" in _lib.last_error()


def test_the_new_keywords_default_to_off():
    from funcodec_amd.bin.codec_inference import Speech2Token
    from funcodec_amd.stream import CodecStream, StreamSlots
    for fn in (EncodecMI355X.open_stream, EncodecMI355X.open_slots, Speech2Token.open_stream, Speech2Token.open_slots, CodecStream.__init__,
               StreamSlots.__init__, CodecEngine.rvq_encode):
        p = inspect.signature(fn).parameters
        assert p["noise_floor_db"].default is None and p["min_n_q"].default == 1, fn
    assert inspect.signature(CodecEngine.rvq_encode).parameters["fused"].default is True
    assert "noise_floor_db" in inspect.signature(StreamSlots.start).parameters
    assert callable(CodecStream.set_noise_floor) and callable(StreamSlots.set_noise_floor)


# ---- refusals on the host ------------------------------------------------------------------------------------------------------------
def test_host_refusals_name_their_key():
    for bad in (NAN, None, "3", True):
        with pytest.raises(EngineError, match="noise_floor_db"):
            floor_value(ARCH, bad)
    with pytest.raises(EngineError, match="row 1: noise_floor_db is a number of dB \\(not NaN\\)"):
        floor_values(ARCH, [-20.0, NAN, -30.0], 3)
    with pytest.raises(EngineError, match="one entry per row \\(3\\), got 2"):
        floor_values(ARCH, [-20.0, -30.0], 3)
    with pytest.raises(EngineError, match="min_n_q = 3 lies above the cap of row 2"):
        rate_min_nq(ARCH, 3, 6, [6, 4, 2])
    with pytest.raises(EngineError, match="min_n_q"):
        rate_min_nq(ARCH, 0, 6)
    with pytest.raises(EngineError, match="min_n_q"):
        rate_min_nq(ARCH, 7, 6)
    q0 = type("A", (), dict(ARCH_KW, q0_ds_ratio=2))()
    assert "quantizer_conf.q0_ds_ratio > 1" in floor_refusal(q0) and floor_refusal(ARCH) is None
    with pytest.raises(EngineError, match="noise_floor_db is not available for quantizer_conf.q0_ds_ratio > 1"):
        floor_values(q0, -20.0, 1)
    seg = type("A", (), dict(ARCH_KW, segment_length=320))()
    with pytest.raises(EngineError, match="model_conf.segment_dur"):
        floor_values(seg, -20.0, 1)
