"""CPU tests of the stage count per row chosen by a target SNR (fc_engine_set_rate, fc_rvq_encode_rate, ``target_snr_db=``): the C-ABI
surface, the defaults, the refusals (all before any engine call: there is no GPU here) and the pick itself, ``rate_pick``, on hand-made
curves -- tests/test_rvq_rate_gpu.py holds the device's pick against it."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from funcodec_amd import _lib
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.engine import CodecEngine, EngineError, rate_pick, rate_refusal, rate_targets
from funcodec_amd.model import EncodecMI355X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fc_engine_set_rate": 8, "fc_rvq_encode_rate": 8}
INF = float("inf")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "funcodec_amd.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(NEW))
def test_entry_points_are_declared_bound_and_exported(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/funcodec_amd.h"
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    res, args = _lib.SYMBOLS[name]
    assert res is ctypes.c_int and len(args) == len(params) == NEW[name], (params, args)
    assert hasattr(ctypes.CDLL(_lib.lib_path()), name)


def test_argtypes_of_set_rate():
    res, args = _lib.SYMBOLS["fc_engine_set_rate"]
    assert [a for a in args if a is ctypes.c_int] == [ctypes.c_int, ctypes.c_int] and args[2] is ctypes.c_int and args[3] is ctypes.c_int


def test_abi_version_stays_and_the_header_cites_the_rule():
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", _header())
    assert _lib.FC_ABI_VERSION == 7 and _lib.load().fc_abi_version() == 7
    assert "rate_pick" in _header() and "offline calls only" in _header()


def test_null_engine_is_refused():
    lib = _lib.load()
    ratios = (ctypes.c_double * 2)(0.1, 0.1)
    assert lib.fc_engine_set_rate(None, ratios, 2, 1, None, None, None, None) != 0
    assert b"null engine" in lib.fc_last_error()
    assert lib.fc_rvq_encode_rate(None, None, 1, 1, 1, None, None, None) != 0


def test_the_unit_is_in_the_build():
    from funcodec_amd import build
    assert "rvq_rate_kernels.hip" in build.sources() and "rvq_rate_kernels.h" in build.HEADERS


# ---- defaults -------------------------------------------------------------------------------------------------------------------------
def test_the_new_keywords_default_to_off():
    from funcodec_amd.bin.codec_inference import Speech2Token
    for fn in (CodecEngine.encode, CodecEngine.encode_decode, CodecEngine.rvq_encode, EncodecMI355X.inference, EncodecMI355X.inference_encoding,
               Speech2Token.__call__):
        p = inspect.signature(fn).parameters
        assert p["target_snr_db"].default is None and p["min_n_q"].default == 1, fn


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
class _NoEngineCall:
    """stands in for the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the refusal must come before any engine call")


def _model(cfg_name):
    m = EncodecMI355X(arch_from_config(recipe_config(cfg_name)), "cuda:0")
    real = m.engine.lib
    m.engine.lib = _NoEngineCall()
    return m, real


@pytest.mark.parametrize("cfg_name,key", [("tinyq0", "quantizer_conf.q0_ds_ratio"), ("tinybypass", "model_conf.bypass_quantizer"),
                                          ("tinybypassseg", "model_conf.segment_dur")])
def test_configurations_are_refused_by_name_before_any_engine_call(cfg_name, key):
    arch = arch_from_config(recipe_config(cfg_name))
    assert key in rate_refusal(arch) and "target_snr_db" in rate_refusal(arch)
    with pytest.raises(EngineError, match=key):
        rate_targets(arch, 12.0, 2)
    m, real = _model(cfg_name)
    try:
        wav = torch.zeros(2, 64)
        for call in (m.inference, m.inference_encoding):
            with pytest.raises(EngineError, match=key):
                call(wav, target_snr_db=12.0)
        for call in (m.engine.encode, m.engine.encode_decode):
            with pytest.raises(EngineError, match=key):
                call(wav, 1, target_snr_db=[12.0, 6.0])
        with pytest.raises(EngineError, match=key):
            m.engine.rvq_encode(torch.zeros(4, arch.codebook_dim), 1, target_snr_db=[12.0, 6.0])
    finally:
        m.engine.lib = real


def test_wrappers_refuse_bad_targets_and_floors_before_any_engine_call():
    assert rate_refusal(arch_from_config(recipe_config("tiny"))) is None
    m, real = _model("tiny")          # 6 stages
    try:
        wav = torch.zeros(3, 64)
        for call in (m.inference, m.inference_encoding):
            with pytest.raises(EngineError, match="one entry per row"):
                call(wav, target_snr_db=[12.0, 6.0])
            with pytest.raises(EngineError, match="NaN"):
                call(wav, target_snr_db=[12.0, float("nan"), 3.0])
            with pytest.raises(EngineError, match="target_snr_db"):
                call(wav, target_snr_db=["12", 1.0, 2.0])
            for bad in (0, 7, 2.0, True):
                with pytest.raises(EngineError, match="min_n_q"):
                    call(wav, target_snr_db=12.0, min_n_q=bad)
            with pytest.raises(EngineError, match="min_n_q = 3 lies above the cap of row 1"):
                call(wav, target_snr_db=12.0, min_n_q=3, bit_width=[6 * 12000.0, 2 * 12000.0, 4 * 12000.0])
            with pytest.raises(EngineError, match="min_n_q"):
                call(wav, target_snr_db=12.0, min_n_q=3, bit_width=2 * 12000.0)         # above the call's n_q
        with pytest.raises(EngineError, match="min_n_q"):
            m.engine.encode(wav, 2, target_snr_db=1.0, min_n_q=3)
        with pytest.raises(EngineError, match="return_paths"):
            m.engine.rvq_encode(torch.zeros(4, 16), 2, beam=2, return_paths=True, target_snr_db=[1.0, 2.0])
        with pytest.raises(EngineError, match="utterances of equal length"):
            m.engine.rvq_encode(torch.zeros(5, 16), 2, target_snr_db=[1.0, 2.0])
    finally:
        m.engine.lib = real


def test_targets_become_float64_ratios():
    arch = arch_from_config(recipe_config("tiny"))
    assert rate_targets(arch, 10.0, 3) == [0.1] * 3
    r = rate_targets(arch, torch.tensor([0.0, 20.0, INF, -INF]), 4)
    assert r[0] == 1.0 and r[1] == pytest.approx(0.01, rel=1e-15) and r[2] == 0.0 and r[3] == INF
    assert rate_targets(arch, np.float32(3.0), 1) == [10.0 ** -0.3]
    assert all(isinstance(v, float) for v in r)


# ---- the pick -------------------------------------------------------------------------------------------------------------------------
def test_pick_takes_the_first_crossing_of_a_curve_that_is_not_monotone():
    E = [100.0, 30.0, 9.0, 40.0, 0.5, 0.2]            # 0, 5.2, 10.5, 4.0, 23.0, 27.0 dB
    assert rate_pick(E, 10 ** -1.0, 1, 5) == 2         # 10 dB: stage 2 reaches it, though stage 3 falls back below
    assert rate_pick(E, 10 ** -0.5, 1, 5) == 1
    assert rate_pick(E, 10 ** -2.0, 1, 5) == 4
    assert rate_pick(E, 10 ** -1.0, 3, 5) == 4         # the floor skips the first crossing: the next one
    assert rate_pick(E, 0.09, 1, 5) == 2               # E[k] == E[0] * rho reaches the target


def test_pick_of_a_target_out_of_reach_is_the_best_count_first_on_ties():
    E = [100.0, 30.0, 9.0, 40.0, 9.0, 12.0]
    assert rate_pick(E, 1e-6, 1, 5) == 2               # argmin, the first of the two
    assert rate_pick(E, 1e-6, 3, 5) == 4               # ... within the floor
    assert rate_pick(E, 1e-6, 1, 1) == 1
    assert rate_pick(E, 1e-6, 4, 5) == 4
    assert rate_pick(E, 0.0, 1, 5) == 2                # +inf dB: the best k
    assert rate_pick([4.0, 2.0, 0.0, 1.0], 0.0, 1, 3) == 2     # an exact zero reaches even rho = 0, and is the first
    # never more bits for a worse result: 2 stages give 36 dB, 32 would give 7
    curve = [1.0, 0.3, 10 ** -3.6] + [0.26] * 2 + [0.19] * 28
    assert rate_pick(curve, 10 ** -4.0, 1, 32) == 2


def test_pick_honours_floor_and_cap():
    E = [100.0, 50.0, 20.0, 5.0, 1.0, 0.1]
    assert rate_pick(E, 0.5, 1, 5) == 1 and rate_pick(E, 0.5, 3, 5) == 3 and rate_pick(E, 0.5, 5, 5) == 5
    assert rate_pick(E, 1e-3, 1, 3) == 3               # the crossing at 5 lies behind the cap: the best below it
    assert rate_pick(E, 1e-3, 1, 5) == 5
    assert rate_pick(E + [float("nan")], 1e-3, 1, 5) == 5      # what lies behind the cap is not looked at
    assert rate_pick(E, INF, 2, 5) == 2                # -inf dB: the floor


def test_pick_of_a_silent_row_is_the_floor_and_of_a_row_that_is_not_finite_the_cap():
    assert rate_pick([0.0, 0.3, 0.2, 0.1], 0.1, 1, 3) == 1 and rate_pick([0.0, 0.3, 0.2, 0.1], 0.0, 2, 3) == 2
    nan = float("nan")
    assert rate_pick([nan, nan, nan, nan], 0.1, 1, 3) == 3
    assert rate_pick([1.0, 0.01, nan, 0.5], 0.1, 1, 3) == 3    # even where an earlier stage reaches the target
    assert rate_pick([INF, 1.0, 0.5, 0.1], 0.1, 1, 3) == 3
    assert rate_pick([1.0, 0.01, nan, 0.5], 0.1, 1, 1) == 1    # ... but only up to the cap
    assert rate_pick(np.array([1.0, 0.5, 0.05]), 0.1, 1, 2) == 2 and isinstance(rate_pick(torch.tensor([1.0, 0.5, 0.05], dtype=torch.float64), 0.1, 1, 2), int)


def test_pick_multiplies_in_float64():
    E0, rho = 3.0000000000000004, 10.0 ** -1.3
    thr = float(np.float64(E0) * np.float64(rho))
    assert rate_pick([E0, thr], rho, 1, 1) == 1 and rate_pick([E0, math.nextafter(thr, INF), thr], rho, 1, 2) == 2


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_flags():
    from funcodec_amd.bin.codec_inference import get_parser
    p = get_parser()
    a = p.parse_args([])
    assert a.target_snr_db is None and a.min_n_q == 1
    a = p.parse_args(["--target_snr_db", "12.5", "--min_n_q", "2"])
    assert a.target_snr_db == 12.5 and a.min_n_q == 2
    with pytest.raises(SystemExit):
        p.parse_args(["--target_snr_db", "loud"])


class _StandIn:
    """Speech2Token's call contract with a count per utterance that is a function of its length (there is no GPU here); everything
    around it -- the parser, the loader, the writers -- is the product's"""
    HOP, NQ = 320, 4

    class _Model:
        class quantizer:
            encoder_hop_length, sampling_rate, codebook_size = 320, 16000, 1024

        class engine:
            @staticmethod
            def check_status(sync=False):
                return None

    def __init__(self):
        self.model, self.already_stat_flops, self.calls = self._Model(), False, []

    def __call__(self, speech, need_recon=True, bit_width=None, use_scale=True, run_mod="inference", target_snr_db=None, min_n_q=1, **kw):
        self.calls.append((target_snr_db, min_n_q))
        B, T = speech.shape
        Tf = -(-T // self.HOP)
        ks = torch.tensor([max(min_n_q, 1 + (int(speech[b].abs().gt(0).sum()) // self.HOP) % self.NQ) for b in range(B)], dtype=torch.int32)
        codes = torch.full((self.NQ, B, Tf), 7, dtype=torch.long)
        for b, k in enumerate(ks.tolist()):
            codes[k:, b] = 0
        self.last_n_q_rows, self.last_row_snr_db = ks, ks.double() * 1.5
        return [codes], None, None, None


def test_cli_writes_the_counts_next_to_the_indices(tmp_path, monkeypatch):
    import json
    from funcodec_amd import io as fio
    from funcodec_amd.bin import codec_inference as ci
    rng = np.random.default_rng(3)
    lines = []
    for i in range(5):
        p = str(tmp_path / f"utt{i}.wav")
        fio.save_audio((0.1 * rng.standard_normal(320 * (9 + i)) + 0.01).astype(np.float32)[None], p, 16000, False)
        lines.append(f"utt{i} {p}\n")
    scp = str(tmp_path / "wav.scp")
    with open(scp, "w") as f:
        f.writelines(lines)
    stand = _StandIn()
    monkeypatch.setattr(ci.Speech2Token, "from_pretrained", staticmethod(lambda **kw: stand))
    out = str(tmp_path / "out.1")
    argv = ["--batch_size", "2", "--ngpu", "1", "--data_path_and_name_and_type", f"{scp},speech,sound", "--config_file", "unused.yaml",
            "--model_file", "unused.pth", "--output_dir", out, "--sampling_rate", "16000", "--bit_width", "16000", "--need_indices", "true",
            "--run_mod", "encode"]
    ci.main(argv + ["--target_snr_db", "12.5", "--min_n_q", "2"])
    assert stand.calls and all(c == (12.5, 2) for c in stand.calls)
    rows = [ln.split() for ln in open(os.path.join(out, "codec_n_q.txt")).read().splitlines()]
    assert [r[0] for r in rows] == [f"utt{i}" for i in range(5)] and all(len(r) == 3 for r in rows)
    for (key, k, snr), ln in zip(rows, open(os.path.join(out, "codecs.txt")).read().splitlines()):
        arr = np.array(json.loads(ln.split(" ", 1)[1]))[0]                  # [n_q, frames]: the indices keep their shape, zeros behind k
        assert ln.startswith(key + " ") and arr.shape[0] == _StandIn.NQ and 2 <= int(k) <= _StandIn.NQ
        assert (arr[:int(k)] == 7).all() and (arr[int(k):] == 0).all() and float(snr) == pytest.approx(1.5 * int(k))
    # without the flag nothing is asked for and no file is written
    stand.calls.clear()
    plain = str(tmp_path / "out.2")
    ci.main(argv[:argv.index(out)] + [plain] + argv[argv.index(out) + 1:])
    assert all(c == (None, 1) for c in stand.calls) and not os.path.exists(os.path.join(plain, "codec_n_q.txt"))
