"""CPU tests of the stage count per frame chosen by a target SNR (fc_engine_set_rate_frames, fc_engine_set_frame_nq, ``per_frame=``):
the host statement of the rule (``rate_pick_frames``), the floor's checker, the C-ABI surface, and every refusal that must come before
anything reaches the device.  No GPU is needed."""
import inspect
import os
import re

import numpy as np
import pytest

from funcodec_amd import _lib
from funcodec_amd.engine import CodecEngine, EngineError, rate_min_nq, rate_min_nq_frames, rate_pick, rate_pick_frames
from funcodec_amd.model import EncodecMI355X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NEW = {"fc_engine_set_rate_frames": 6, "fc_engine_set_frame_nq": 5}


def _header():
    with open(os.path.join(ROOT, "include", "funcodec_amd.h")) as f:
        return f.read()


def _curves(Tf=9, cap=12, seed=0):
    """err [cap + 1, Tf] float32, falling by about 2 dB a stage from very different input energies, and its float64 row sums"""
    rng = np.random.default_rng(seed)
    e0 = 10.0 ** rng.uniform(-3, 1, Tf)
    err = (e0[None, :] * 10.0 ** (-0.2 * np.arange(cap + 1)[:, None]) * rng.uniform(0.9, 1.1, (cap + 1, Tf))).astype(np.float32)
    return err, err.astype(np.float64).sum(1)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def test_when_every_frame_qualifies_the_sum_meets_the_row_threshold():
    for seed in range(5):
        err, E = _curves(seed=seed)
        rho = 10.0 ** -1.2
        k = rate_pick_frames(err, E, rho, 0, 12)
        assert k.dtype == np.int32 and k.shape == (9,)
        thr = E[0] * rho
        got = err[k, np.arange(9)].astype(np.float64)
        assert np.all(got * 9.0 <= thr), "every frame reaches the target inside 12 stages of 2 dB"
        assert got.sum() <= thr * (1 + 1e-12)                          # a constant noise floor per row: sum <= F * thr / F
        for t in range(9):                                             # and no smaller count does
            assert k[t] == 0 or np.float64(err[k[t] - 1, t]) * 9.0 > thr
        assert len(set(k.tolist())) > 2, "loud frames take more stages than quiet ones"


def test_silence_nonfinite_rows_misses_and_the_floor():
    err, E = _curves()
    # silence: every frame takes the floor
    z = np.zeros_like(err)
    assert rate_pick_frames(z, z.sum(1), 0.1, 0, 12).tolist() == [0] * 9 and rate_pick_frames(z, z.sum(1), 0.1, 3, 12).tolist() == [3] * 9
    # a row whose sums are not all finite: every frame takes the cap; a NaN behind the cap is not looked at
    for bad in (NAN, INF):
        e = err.copy()
        e[4, 2] = bad
        Eb = e.astype(np.float64).sum(1)
        assert rate_pick_frames(e, Eb, 0.1, 0, 12).tolist() == [12] * 9
        assert np.array_equal(rate_pick_frames(e, Eb, 0.1, 0, 3), rate_pick_frames(err, E, 0.1, 0, 3))
    # a miss takes the arg-min, first on ties
    e = np.array([[8.0], [4.0], [2.0], [2.0], [3.0]], np.float32)
    assert rate_pick_frames(e, e[:, 0].astype(np.float64), 1e-9, 0, 4).tolist() == [2]
    assert rate_pick_frames(e, e[:, 0].astype(np.float64), 1e-9, 3, 4).tolist() == [3]
    assert rate_pick_frames(e, e[:, 0].astype(np.float64), 0.0, 0, 4).tolist() == [2]       # a target of +inf: the best count
    assert rate_pick_frames(e, e[:, 0].astype(np.float64), INF, 0, 4).tolist() == [0]       # -inf: the floor
    # floor 0: a frame below the noise floor takes no stage; the floor holds a frame up; the cap holds it down
    assert rate_pick_frames(err, E, 10.0, 0, 12).tolist() == [0] * 9 or rate_pick_frames(err, E, 10.0, 0, 12).min() == 0
    assert rate_pick_frames(err, E, 10.0, 2, 12).min() == 2
    assert rate_pick_frames(err, E, 1e-6, 0, 5).max() <= 5 and rate_pick_frames(err, E, 0.1, 7, 5).tolist() == [5] * 9
    # frames behind the row's own frames take 0 and are not read
    e = err.copy()
    e[:, 6:] = NAN
    Ef = e[:, :6].astype(np.float64).sum(1)
    k = rate_pick_frames(e, Ef, 0.05, 0, 12, frames=6)
    assert k[6:].tolist() == [0, 0, 0] and np.array_equal(k[:6], rate_pick_frames(err[:, :6], Ef, 0.05, 0, 12))


def test_one_frame_with_a_floor_is_the_row_rule():
    """F = 1: err * 1 <= thr is E[k] <= E[0] * rho"""
    rng = np.random.default_rng(3)
    for trial in range(200):
        cap = int(rng.integers(1, 13))
        e = (10.0 ** rng.uniform(-2, 1, (cap + 1, 1))).astype(np.float32)
        if trial % 7 == 0:
            e[:] = 0
        if trial % 11 == 0:
            e[int(rng.integers(0, cap + 1))] = NAN
        E = e[:, 0].astype(np.float64)
        rho = float(10.0 ** rng.uniform(-2, 0.5))
        floor = int(rng.integers(1, cap + 1))
        assert rate_pick_frames(e, E, rho, floor, cap).tolist() == [rate_pick(E, rho, floor, cap)], trial


def test_the_floor_checker():
    arch = type("A", (), dict(num_quantizers=6))()
    assert [rate_min_nq_frames(arch, v) for v in (0, 1, 6)] == [0, 1, 6] and rate_min_nq_frames(arch, 0, 3, [3, 1]) == 0
    for bad in (-1, 7, 1.5, True, None, "2"):
        with pytest.raises(EngineError, match="min_n_q"):
            rate_min_nq_frames(arch, bad)
    with pytest.raises(EngineError, match="min_n_q"):
        rate_min_nq_frames(arch, 4, 3)
    with pytest.raises(EngineError, match="min_n_q = 2 lies above the cap of row 1"):
        rate_min_nq_frames(arch, 2, 6, [3, 1])
    with pytest.raises(EngineError, match="min_n_q"):                  # the row rule's checker stays as it is
        rate_min_nq(arch, 0)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    text = _header()
    for name, nargs in NEW.items():
        assert hasattr(lib, name) and name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", text, re.S)
        assert m and "csrc/rvq_rate_kernels.h" in m.group(1), name       # each entry states the rule by reference to the kernel header
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", text) and _lib.FC_ABI_VERSION == 7 and lib.fc_abi_version() == 7
    with open(os.path.join(ROOT, "funcodec_amd", "csrc", "rvq_rate_kernels.h")) as f:
        rule = f.read()
    for word in ("thr_b = E_b[0] * rho_b", "no division", "first on ties", "reverse water-filling", "clamped to [0, nq]"):
        assert word in rule, word
    from funcodec_amd import build
    assert "rvq_rate_kernels.hip" in build.sources() and "rvq_rate_kernels.h" in build.HEADERS
    # a null engine is refused by name, nothing is touched
    assert lib.fc_engine_set_rate_frames(None, 0, None, None, None, None) != 0 and "engine" in _lib.last_error()
    assert lib.fc_engine_set_frame_nq(None, None, 1, 1, None) != 0 and "engine" in _lib.last_error()


def test_the_new_keywords_default_to_off():
    from funcodec_amd.bin.codec_inference import Speech2Token, get_parser
    for fn in (CodecEngine.encode, CodecEngine.encode_decode, CodecEngine.rvq_encode, EncodecMI355X.inference, EncodecMI355X.inference_encoding,
               Speech2Token.__call__):
        assert inspect.signature(fn).parameters["per_frame"].default is False, fn
    for fn in (CodecEngine.decode_codes, EncodecMI355X.inference_decoding, Speech2Token.__call__, CodecEngine.pack_codes):
        assert inspect.signature(fn).parameters["n_q_frames"].default is None, fn
    a = get_parser().parse_args([])
    assert a.per_frame is False and a.min_n_q == 1
    assert get_parser().parse_args(["--per_frame", "true", "--min_n_q", "0"]).per_frame is True


# ---- refusals before anything reaches the device -----------------------------------------------------------------------------------------
class _NoEngineCall:
    """stands in for the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the refusal came too late")


def _model(name):
    """a model of recipe `name` whose library is replaced: the refusals under test need no engine call"""
    from funcodec_amd.config import arch_from_config, recipe_config
    m = EncodecMI355X(arch_from_config(recipe_config(name)), "cuda:0")
    m.engine.lib = _NoEngineCall()
    return m


def test_per_frame_is_refused_by_name_before_anything_reaches_the_device():
    import torch
    wav = torch.zeros(3, 400)
    m = _model("tiny")
    for call in (m.inference, m.inference_encoding):
        with pytest.raises(EngineError, match="target"):                # without a target
            call(wav, per_frame=True)
        for bad in (-1, 7, 1.5):
            with pytest.raises(EngineError, match="min_n_q"):
                call(wav, target_snr_db=12.0, per_frame=True, min_n_q=bad)
        with pytest.raises(EngineError, match="min_n_q = 3 lies above the cap of row 1"):
            call(wav, target_snr_db=12.0, per_frame=True, min_n_q=3, bit_width=[6 * 12000.0, 2 * 12000.0, 4 * 12000.0])
    for name, word in (("tinybypassseg", "segment_dur"), ("tinybypass", "bypass_quantizer"), ("tinyq0", "q0_ds_ratio")):
        with pytest.raises(EngineError, match=word):
            _model(name).inference(wav, target_snr_db=12.0, per_frame=True, min_n_q=0)
    with pytest.raises(EngineError, match="target"):
        m.engine.rvq_encode(torch.zeros(6, 16), 6, per_frame=True)
    with pytest.raises(EngineError, match="give one of them"):
        m.engine.decode_codes(torch.zeros(3, 5, 6, dtype=torch.int64), n_q_rows=[1, 2, 3], n_q_frames=torch.zeros(3, 5))
