"""CPU tests of the stage count per FRAME of a session push chosen by a noise floor (fc_engine_set_floor_frames, ``per_frame=True`` on
``open_stream`` / ``open_slots``): the host statement of the push frame rule (``floor_pick_frames``), the C-ABI surface, and mode-1 packets
of such counts on the host.  No GPU is needed."""
import inspect
import os
import re

import numpy as np
import pytest

from funcodec_amd import _lib, io as fio
from funcodec_amd.engine import CodecEngine, EngineError, floor_pick, floor_pick_frames, floor_value, rate_min_nq
from funcodec_amd.model import EncodecMI355X
from funcodec_amd.stream import CodecStream, StreamSlots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
ARCH = type("A", (), dict(num_quantizers=6, codebook_dim=16, segment_length=None, bypass_quantizer=False, q0_ds_ratio=1))()
#          k =   0     1    2    3    4    5    6
CURVE = [100.0, 40.0, 9.0, 4.0, 4.0, 1.0, 2.0]


def _header():
    with open(os.path.join(ROOT, "include", "funcodec_amd.h")) as f:
        return f.read()


def frames_of(*curves):
    """stage errors [n_q + 1, 1, F] of one row whose frames have the given curves"""
    return np.asarray(curves, dtype=np.float32).T[:, None, :]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def test_every_frame_takes_the_first_count_that_meets_the_floor():
    quiet = [v * 0.01 for v in CURVE]
    err = frames_of(CURVE, quiet, CURVE)
    out = floor_pick_frames(err, 3, 5.0, 1, 6)
    assert out.dtype == np.int32 and out.shape == (1, 3)
    assert out.tolist() == [[3, 1, 3]]              # 4 <= 5 at k = 3; the quiet frame's input (1.0) already lies below the floor
    assert floor_pick_frames(err, 3, 9.0, 1, 6).tolist() == [[2, 1, 2]]         # 9 <= 9: the comparison is <=
    assert floor_pick_frames(err, 3, 5.0, 4, 6).tolist() == [[4, 4, 4]]         # min_n_q holds a frame up
    # no product with the frame count: a row of 3 frames and a row of 1 frame pick alike
    assert floor_pick_frames(frames_of(CURVE), 1, 5.0, 1, 6).tolist() == [[3]]


def test_a_missed_floor_takes_the_best_count_first_on_ties():
    err = frames_of(CURVE)
    assert floor_pick_frames(err, 1, 0.5, 1, 6).tolist() == [[5]]       # nothing reaches 0.5: the smallest error, not the cap
    assert floor_pick_frames(err, 1, 0.5, 1, 4).tolist() == [[3]]       # err[3] == err[4]: the first
    assert floor_pick_frames(err, 1, 0.5, 0, 6).tolist() == [[5]]       # lo = 0: err[0] is in the scan and is the worst
    assert floor_pick_frames(err, 1, 0.5, 4, 4).tolist() == [[4]]
    up = frames_of([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])                 # every stage makes it worse
    assert floor_pick_frames(up, 1, 0.5, 0, 6).tolist() == [[0]] and floor_pick_frames(up, 1, 0.5, 2, 6).tolist() == [[2]]


def test_floors_of_minus_inf_plus_inf_and_zero():
    err = frames_of(CURVE, [0.0] * 7)
    assert floor_value(ARCH, -INF) == 0.0 and floor_value(ARCH, INF) == INF
    assert floor_pick_frames(err, 2, floor_value(ARCH, -INF), 1, 6).tolist() == [[5, 1]]       # -inf dB: the best k; digital silence: lo
    assert floor_pick_frames(err, 2, floor_value(ARCH, -INF), 0, 6).tolist() == [[5, 0]]       # lo = 0: a silent frame costs no stage
    assert floor_pick_frames(err, 2, floor_value(ARCH, INF), 2, 6).tolist() == [[2, 2]]        # +inf dB: always lo
    assert floor_pick_frames(err, 2, floor_value(ARCH, INF), 0, 6).tolist() == [[0, 0]]
    assert floor_pick_frames(frames_of([3.0, 2.0, 0.0, 0.0]), 1, 0.0, 1, 3).tolist() == [[2]]  # an exact residual of 0 meets a floor of 0


def test_one_nan_frame_takes_the_cap_and_its_neighbours_do_not():
    bad = list(CURVE)
    bad[4] = NAN
    err = frames_of(CURVE, bad, CURVE)
    assert floor_pick_frames(err, 3, 5.0, 1, 6).tolist() == [[3, 6, 3]]
    assert floor_pick_frames(err, 3, 5.0, 1, 3).tolist() == [[3, 3, 3]]         # the NaN lies behind the cap: it is not looked at
    bad[4] = INF
    assert floor_pick_frames(frames_of(bad), 1, 5.0, 0, 5).tolist() == [[5]]


def test_a_row_switched_off_frames_behind_the_rows_frames_and_an_idle_row():
    err = np.concatenate([frames_of(CURVE, CURVE, CURVE)] * 3, axis=1)          # [7, 3, 3]
    out = floor_pick_frames(err, [3, 2, 0], [None, 5.0, 5.0], 0, [6, 4, 6])
    assert out.tolist() == [[6, 6, 6],          # switched off: the cap in every frame
                            [3, 3, 0],          # two frames in the push: the third takes 0
                            [-1, -1, -1]]       # no frame in the push: the device leaves the row alone
    assert floor_pick_frames(err, 3, [-1.0, 5.0, 5.0], 0, 6).tolist()[0] == [6, 6, 6]      # on the device a floor of -1 says the same
    assert floor_pick_frames(err, 3, 5.0, 5, [6, 2, 6]).tolist() == [[5] * 3, [2] * 3, [5] * 3]       # lo is clamped to a row's cap


@pytest.mark.parametrize("min_n_q", [1, 2, 4])
def test_one_frame_rows_pick_as_the_push_rule(min_n_q):
    """F_b = 1 and min_n_q >= 1: floor * 1.0 is floor and the one-term float64 sum is the float32 error itself"""
    rng = np.random.default_rng(7)
    # falling curves with a jitter (not monotone), inputs of 10 .. 1000 against floors of 0.01 .. 10
    err = (10.0 ** rng.uniform(1, 3, (1, 40, 1)) * 0.4 ** np.arange(7)[:, None, None] * rng.uniform(0.5, 2.0, (7, 40, 1))).astype(np.float32)
    err[3, 5, 0] = NAN
    caps = rng.integers(min_n_q, 7, 40).tolist()
    floors = (10.0 ** rng.uniform(-2, 1, 40)).tolist()
    floors[7] = None
    rows = floor_pick(err[:, :, 0].T.astype(np.float64), 1, floors, min_n_q, caps)
    frames = floor_pick_frames(err, 1, floors, min_n_q, caps)
    assert frames[:, 0].tolist() == rows.tolist()
    assert len(set(rows.tolist())) >= 3


# ---- the C ABI and the Python surface ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_the_abi_version_stays():
    h = _header()
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", h)
    for name in ("fc_engine_set_floor_frames", "fc_engine_set_push_frame_nq"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
        assert name in _lib.SYMBOLS
    assert "THE PUSH FRAME RULE" in h and "floor_pick_frames" in h
    with open(os.path.join(ROOT, "funcodec_amd", "csrc", "rvq_rate_kernels.h")) as f:
        rule = f.read()
    assert rule.count("THE PUSH FRAME RULE,") == 1 and "this rule IS the push rule" in rule
    assert "offline calls only" in h                                    # the sentence the rate's host tests quote stays


def test_keywords_reach_both_session_kinds_and_the_hook():
    for fn in (EncodecMI355X.open_stream, EncodecMI355X.open_slots, CodecStream.__init__, StreamSlots.__init__):
        p = inspect.signature(fn).parameters
        assert p["per_frame"].default is False and p["min_n_q"].default == 1, fn
    from funcodec_amd.bin.codec_inference import Speech2Token
    for fn in (Speech2Token.open_stream, Speech2Token.open_slots):
        assert inspect.signature(fn).parameters["per_frame"].default is False
    assert "fused" in inspect.signature(CodecEngine.rvq_encode).parameters
    assert isinstance(CodecStream.last_n_q_frames, property) and isinstance(StreamSlots.last_n_q_frames, property)
    assert "n_q_frames" in inspect.signature(CodecStream.decode).parameters and "n_q_frames" in inspect.signature(StreamSlots.decode).parameters


def test_min_n_q_of_frame_mode_lies_in_0_to_n_q():
    assert rate_min_nq(ARCH, 0, 6, floor=0) == 0 and rate_min_nq(ARCH, 6, 6, floor=0) == 6
    for bad in (-1, 7, True, 1.5):
        with pytest.raises(EngineError, match=r"min_n_q lies in \[0, 6\]"):
            rate_min_nq(ARCH, bad, 6, floor=0)
    with pytest.raises(EngineError, match="above the cap of row 1"):
        rate_min_nq(ARCH, 3, 6, [6, 2], floor=0)
    with pytest.raises(EngineError, match=r"min_n_q lies in \[1, 6\]"):       # without per_frame a count of 0 stays refused
        rate_min_nq(ARCH, 0, 6)


# ---- mode-1 packets of a session's counts -----------------------------------------------------------------------------------------------
def test_mode_1_packets_of_a_pushs_counts_round_trip():
    rng = np.random.default_rng(11)
    n_q, F = 6, 17
    codes = rng.integers(0, 1024, (n_q, F))
    counts = np.array([0, 6, 3, 0, 0, 1, 2, 6, 6, 0, 4, 5, 0, 0, 0, 3, 1], dtype=np.int32)      # silence costs its count bits alone
    for t, k in enumerate(counts):
        codes[k:, t] = 0
    packet = fio.pack_frame_codes(codes, counts, bits=10)
    assert fio.packet_mode(packet) == 1
    frames, kmax = fio.parse_frame_packet(packet, n_q=n_q, bits=10)[:2]
    assert (frames, kmax) == (F, 6)
    assert len(packet) == fio.frame_packet_bytes(F, 6, int(counts.sum()), 10)
    got_codes, got_counts, _ = fio.unpack_frame_packet(packet)
    assert np.array_equal(got_counts, counts) and np.array_equal(np.asarray(got_codes).T, codes)
    silent = fio.pack_frame_codes(np.zeros((n_q, F), np.int64), np.zeros(F, np.int32), bits=10)
    kmax0 = fio.parse_frame_packet(silent, n_q=n_q, bits=10)[1]
    assert len(silent) == fio.frame_packet_bytes(F, kmax0, 0, 10) < fio.packet_bytes(F, 1, 10)      # below the smallest mode-0 packet
    with pytest.raises(fio.PacketError):
        fio.parse_frame_packet(packet[:-1], n_q=n_q, bits=10)


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------
def test_per_frame_is_refused_for_nets_without_a_per_frame_residual():
    """before anything of the session is opened (the engine is never reached)"""
    import dataclasses
    from funcodec_amd.config import arch_from_config, recipe_config
    arch = arch_from_config(recipe_config("tinyss"))
    for change, words in ((dict(bypass_quantizer=True), "per_frame=True: .*model_conf.bypass_quantizer"),
                          (dict(segment_dur=1.0), "model_conf.segment_dur"),
                          (dict(q0_ds_ratio=2), "quantizer_conf.q0_ds_ratio > 1")):
        model = type("M", (), dict(arch=dataclasses.replace(arch, **change), engine=None))()
        for open_session in (lambda: CodecStream(model, 1, per_frame=True, noise_floor_db=-20.0, min_n_q=0),
                             lambda: StreamSlots(model, 2, per_frame=True, noise_floor_db=-20.0, min_n_q=0)):
            with pytest.raises(EngineError, match=words):
                open_session()
