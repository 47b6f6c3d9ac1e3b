"""The SLSTM bottleneck's two HIP kernels (lstm_kernels.hip) against a float64 torch.nn.LSTM, at every instantiation the engine
builds and at full recurrence length:

- lstm_wave_kernel<NS> (one launch per wavefront step): every NS (1, 2, 4, 8, 16 and the generic NS = 0 loop) and every k-slice
  count KS (4, 2, 1), L = 1 .. 4 layers, batch tiles of 16 rows (B = 1, 15, 16, 17, 33), T from 1 to ~500 steps, inputs that
  saturate the gates, with and without the res_seq skip;
- lstm_persist_kernel<8 | 16> (one launch, grid barrier): H = 512 / 1024 at L = 2 over ~500 steps, one and two batch tiles;
- the two kernels bit for bit against each other at full length, and freqmpgr1rel (the one-layer H = 128 net bench.py times)
  at its timed shape.

A float32 torch LSTM is no yardstick for a fp32 kernel over hundreds of recurrent steps: each case also runs it, and the kernel's
error against float64 may be at most a fixed multiple of torch float32's own error on the same inputs (or an absolute floor for
inputs where torch's error is tiny).  Every case asserts which kernel class actually ran: after a persistent-kernel barrier timeout
the engine silently moves to the per-step path for good."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import record_report
from helpers import audio, freq_engine_for, freq_oracle_for, index_report, rms
from test_gpu_parity import _assert_flips_are_near_ties

from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.synth import make_state_dict

pytestmark = pytest.mark.gpu

# max |gpu - float64| <= max(ABS_FLOOR, ABS_K * max |torch float32 - float64|), and the same with RMS over the whole output.
# Measured over the cases below on an MI355X: worst max |gpu - f64| 1.81e-6 (H 256, L 1, 4 randn; torch float32 1.64e-6); where
# |gpu - f64| > 2e-7 it is at most 1.42 x torch float32's max error, and where it exceeds 2 x torch's it is at most 1.80e-7 (no skip,
# deep stacks: torch float32 is then ~1e-8, the exp2 / rcp gates ~1e-7).  RMS: at most 1.71 x torch float32's where above 3e-8, at
# most 2.96e-8 where above 2 x torch's.
ABS_FLOOR = 4e-7
ABS_K = 2.0
RMS_FLOOR = 6e-8
RMS_K = 2.0

LONG_T = 501                 # freqmpgr1rel's frames per 10 s utterance (bench.py: 32 x 10 s per call)
BMAX = 33                    # every case of a (net, T, input scale) uses the first B rows of one 33-row input
WAVE_WIDTHS = (16, 32, 48, 64, 96, 128, 192, 256)
PERSIST_WIDTHS = (512, 1024)                 # ds320 / ds640: the persistent kernel at L = 2, B <= 32
L_SWEEP = {(48, 1): False, (48, 3): True, (48, 4): False, (128, 1): True, (128, 3): False, (128, 4): True,
           (256, 1): False, (256, 3): True, (256, 4): False}          # (H, L) -> res_seq


def wave_instantiation(H):
    """(KS, NS) that launch_lstm_wave picks for width H: KS k-slices, the largest of 4, 2, 1 that divides H / 16; NS = H / (16 KS)
    16-column steps per slice, where the NS values without an instantiation of their own run the generic NS = 0 loop."""
    ks = 4
    while ks > 1 and H % (16 * ks):
        ks //= 2
    ns = H // (16 * ks)
    return ks, (ns if ns in (1, 2, 4, 8, 16) else 0)


def _wave_cases():
    """(H, L, skip, B, T, input scale) of the per-step kernel."""
    cases = []
    for H in WAVE_WIDTHS:
        cases += [(H, 2, True, B, 17, 1.0) for B in (1, 15, 16, 17, 33)]
        cases += [(H, 2, True, 17, T, 1.0) for T in (1, 2)]                  # T = L - 1 and T = L
        cases.append((H, 2, True, 33, 17, 4.0))
    cases += [(96, 2, False, 17, 17, 1.0)]
    for (H, L), skip in L_SWEEP.items():
        cases += [(H, L, skip, 17, T, 1.0) for T in sorted({1, 2, max(L - 1, 1), L, 17})]
        cases += [(H, L, skip, 1, 17, 1.0), (H, L, skip, 33, 17, 4.0)]
    cases += [(128, 1, True, 32, LONG_T, 1.0), (128, 1, True, 32, LONG_T, 4.0),     # freqmpgr1rel's LSTM shape
              (48, 3, True, 17, LONG_T, 1.0), (96, 2, False, 17, LONG_T, 4.0),      # the NS = 0 loop, KS = 1 and 2
              (256, 4, False, 33, LONG_T, 1.0)]
    for H in PERSIST_WIDTHS:                  # NS = 8 / 16: B = 33 is beyond the persistent kernel
        cases += [(H, 2, True, 33, 17, 1.0), (H, 2, True, 33, LONG_T, 1.0), (H, 2, True, 33, 17, 4.0)]
    return cases


WAVE_CASES = _wave_cases()
PERSIST_CASES = [(H, 2, True, B, LONG_T, 1.0) for H in PERSIST_WIDTHS for B in (1, 16, 17, 32)] + \
                [(H, 2, True, 17, LONG_T, 4.0) for H in PERSIST_WIDTHS]


def _id(c):
    H, L, skip, B, T, scale = c
    return f"H{H}-L{L}-{'skip' if skip else 'noskip'}-B{B}-T{T}" + ("-x4" if scale != 1.0 else "")


# ---- engines, references --------------------------------------------------------------------------------------------------------
def _config(H, L, skip):
    if (H, L, skip) == (512, 2, True):
        return recipe_config("ds320"), 0
    if (H, L, skip) == (1024, 2, True):
        return recipe_config("ds640"), 0
    cfg = recipe_config("tiny")              # ratios (4, 2): the bottleneck is 4 n_filters wide
    for k in ("encoder_conf", "decoder_conf"):
        cfg[k].update(n_filters=H // 4, seq_layer_num=L, res_seq=skip)
    return cfg, 300 + 8 * H + 2 * L + int(skip)


def _torch_lstm(sd, prefix, H, L, dtype):
    lstm = torch.nn.LSTM(H, H, L).to(dtype)
    with torch.no_grad():
        for name, p in lstm.named_parameters():
            p.copy_(torch.from_numpy(sd[f"{prefix}.{name}"]))
    return lstm.eval()


@functools.lru_cache(maxsize=None)
def _state(H, L, skip):
    """(arch, synthetic state dict, encoder LSTM prefix) of the net whose bottleneck LSTM is H wide with L layers."""
    cfg, seed = _config(H, L, skip)
    arch = arch_from_config(cfg)
    assert (arch.bottleneck_channels, arch.lstm_layers, arch.lstm_skip) == (H, L, skip)
    sd = make_state_dict(arch, seed)
    prefix = [k[: -len(".weight_ih_l0")] for k in sd if k.startswith("encoder.") and k.endswith(".weight_ih_l0")][0]
    return arch, sd, prefix


@functools.lru_cache(maxsize=None)
def _net(H, L, skip):
    """(model, encoder LSTM prefix)."""
    from funcodec_amd.model import EncodecMI355X
    arch, sd, prefix = _state(H, L, skip)
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m, prefix


@functools.lru_cache(maxsize=None)
def _data(H, L, skip, T, scale):
    """Input [BMAX, H, T] of a (net, T, scale) and its float64 / float32 torch outputs (SLSTM: y = LSTM(x) + x when skip).
    LSTM rows are independent: a case of B rows uses the first B rows of all three."""
    _, sd, prefix = _state(H, L, skip)
    g = torch.Generator().manual_seed(1000 * H + 100 * L + T + int(scale))
    x = scale * torch.randn(BMAX, H, T, generator=g)

    def run(lstm, dtype):
        xt = x.to(dtype).permute(2, 0, 1)
        with torch.no_grad():
            y, _ = lstm(xt)
        if skip:
            y = y + xt
        return y.permute(1, 2, 0).double().contiguous()
    return x, run(_torch_lstm(sd, prefix, H, L, torch.float64), torch.float64), \
        run(_torch_lstm(sd, prefix, H, L, torch.float32), torch.float32)


def _lstm_classes(prof):
    return {p["kernel"].split("<")[0] for p in prof if p["launches"] > 0 and p["kernel"].startswith("lstm_")}


def _run(m, prefix, x):
    """Engine output for x and the LSTM kernel classes that produced it."""
    eng = m.engine
    eng.read_profile()
    eng.set_profiling(True)
    try:
        y = eng.lstm_forward(prefix, x).cpu()
        prof = eng.read_profile()
    finally:
        eng.set_profiling(False)
    eng.check_status()
    return y, _lstm_classes(prof)


WORST = {}        # (H, L, path) -> worst measured errors over the session's cases


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    if WORST:
        record_report("lstm_kernels_vs_float64", table=[dict(H=H, L=L, path=p, **v) for (H, L, p), v in sorted(WORST.items())])


def _check(case, got, ref64, ref32, path):
    H, L = case[0], case[1]
    assert torch.isfinite(got).all(), case
    d, d32 = got.double() - ref64, ref32 - ref64
    e, e32 = float(d.abs().max()), float(d32.abs().max())
    r, r32 = float(d.pow(2).mean().sqrt()), float(d32.pow(2).mean().sqrt())
    w = WORST.setdefault((H, L, path), dict(max_gpu=0.0, max_t32=0.0, rms_gpu=0.0, rms_t32=0.0, max_ratio=0.0))
    w.update(max_gpu=max(w["max_gpu"], e), max_t32=max(w["max_t32"], e32), rms_gpu=max(w["rms_gpu"], r), rms_t32=max(w["rms_t32"], r32),
             max_ratio=max(w["max_ratio"], e / max(e32, 1e-30)))
    assert e <= max(ABS_FLOOR, ABS_K * e32), f"{_id(case)} {path}: max |gpu - f64| {e:.3e}, torch float32 {e32:.3e}"
    assert r <= max(RMS_FLOOR, RMS_K * r32), f"{_id(case)} {path}: rms |gpu - f64| {r:.3e}, torch float32 {r32:.3e}"


# ---- 1. each kernel against float64 -----------------------------------------------------------------------------------------------
def test_cases_reach_every_instantiation_and_edge():
    """The matrix below covers all six lstm_wave_kernel instantiations and all three k-slice counts, L = 1 .. 4 at three widths,
    the batch-tile edges and the short / long recurrence lengths."""
    inst = {wave_instantiation(c[0]) for c in WAVE_CASES}
    assert {ns for _, ns in inst} == {0, 1, 2, 4, 8, 16}
    assert {ks for ks, _ in inst} == {1, 2, 4}
    assert {ks for ks, ns in inst if ns == 0} == {1, 2, 4}
    assert [wave_instantiation(H) for H in (16, 48, 96, 192, 512, 1024)] == [(1, 1), (1, 0), (2, 0), (4, 0), (4, 8), (4, 16)]
    for H in (48, 128, 256):
        for L in (1, 2, 3, 4):
            Ts = {c[4] for c in WAVE_CASES if c[:2] == (H, L)}
            assert {1, 2, max(L - 1, 1), L, 17} <= Ts, (H, L)
    assert {c[3] for c in WAVE_CASES} >= {1, 15, 16, 17, 33}
    assert {c[2] for c in WAVE_CASES} == {True, False} and {c[5] for c in WAVE_CASES} == {1.0, 4.0}
    long_ = {(c[0], c[1]) for c in WAVE_CASES if c[4] == LONG_T}
    assert (128, 1) in long_ and any(wave_instantiation(H)[1] == 0 for H, _ in long_)
    assert all(c[3] <= 32 for c in PERSIST_CASES) and all(c[3] > 32 for c in WAVE_CASES if c[0] in PERSIST_WIDTHS)


@pytest.mark.parametrize("case", WAVE_CASES, ids=_id)
def test_wave_kernel_against_float64(case):
    H, L, skip, B, T, scale = case
    m, prefix = _net(H, L, skip)
    x, ref64, ref32 = _data(H, L, skip, T, scale)
    got, ran = _run(m, prefix, x[:B])
    assert ran == {"lstm_wave_kernel"}, ran
    _check(case, got, ref64[:B], ref32[:B], "wave")


@pytest.mark.parametrize("case", PERSIST_CASES, ids=_id)
def test_persistent_kernel_against_float64(case):
    """H = 512 with B > 16 runs two batch-tile groups in one launch, H = 1024 with B > 16 two launches."""
    H, L, skip, B, T, scale = case
    m, prefix = _net(H, L, skip)
    x, ref64, ref32 = _data(H, L, skip, T, scale)
    got, ran = _run(m, prefix, x[:B])
    assert ran == {"lstm_persist_kernel"}, ran
    _check(case, got, ref64[:B], ref32[:B], "persist")


# ---- 2. the two kernels bit for bit at full length ----------------------------------------------------------------------------------
_CHILD = (
    "import json, sys, numpy as np, torch\n"
    "sys.path.insert(0, 'tests'); sys.path.insert(0, 'oracle'); sys.path.insert(0, '.')\n"
    "from test_lstm_kernels import _net, _run\n"
    "ran = []\n"
    "for H, B, xin, yout in json.loads(sys.argv[1]):\n"
    "    m, prefix = _net(H, 2, True)\n"
    "    y, cls = _run(m, prefix, torch.from_numpy(np.load(xin)))\n"
    "    np.save(yout, y.numpy())\n"
    "    ran.append(sorted(cls))\n"
    "print(json.dumps(ran))\n")


def test_wave_and_persistent_kernels_are_bit_identical_at_full_length(tmp_path):
    """The persistent kernel promises the per-step kernel's arithmetic order per accumulator: the per-step launch path
    (FC_LSTM_PERSIST=0, read once per process, hence fresh child processes) must give the same bits over ~500 steps, with two batch
    tiles (H = 512: two groups in one launch; H = 1024: two launches), and both must pass the float64 bar."""
    shapes = [(512, 17), (1024, 32)]
    spec = {flag: [] for flag in ("1", "0")}
    for H, B in shapes:
        np.save(tmp_path / f"x{H}.npy", _data(H, 2, True, LONG_T, 1.0)[0][:B].numpy())
        for flag in spec:
            spec[flag].append((H, B, str(tmp_path / f"x{H}.npy"), str(tmp_path / f"y{H}_{flag}.npy")))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ran = {}
    for flag, s in spec.items():
        out = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(s)], check=True, cwd=root, capture_output=True, text=True,
                             env=dict(os.environ, FC_LSTM_PERSIST=flag), timeout=600)
        ran[flag] = json.loads(out.stdout.strip().splitlines()[-1])
    assert ran["1"] == [["lstm_persist_kernel"]] * len(shapes), ran
    assert ran["0"] == [["lstm_wave_kernel"]] * len(shapes), ran
    for H, B in shapes:
        yp, yw = (torch.from_numpy(np.load(tmp_path / f"y{H}_{flag}.npy")) for flag in ("1", "0"))
        assert torch.equal(yp, yw), (H, B, float((yp - yw).abs().max()))
        _, ref64, ref32 = _data(H, 2, True, LONG_T, 1.0)
        _check((H, 2, True, B, LONG_T, 1.0), yp, ref64[:B], ref32[:B], "persist")
        _check((H, 2, True, B, LONG_T, 1.0), yw, ref64[:B], ref32[:B], "wave")


# ---- 3. freqmpgr1rel at the shape bench.py times ---------------------------------------------------------------------------------
def test_freqmpgr1rel_at_the_timed_shape_in_a_32_utterance_call():
    """bench.py's freqcodec_gr1rel side measurement: weight seed 0, 32 x 10 s of synthetic_audio(.., 1234) in one call of 32, so that
    the one-layer H = 128 LSTM runs ~500 per-step launches (no persistent kernel at this width).  Rows 0, 15, 16, 31 equal the
    single-utterance calls bit for bit, rows 0 / 31 match the CPU oracle (pinned to the real reference by freqmpgr1rel_b2_t16000)
    up to proven fp32 ties."""
    m, orc = freq_engine_for("freqmpgr1rel", 0), freq_oracle_for("freqmpgr1rel", 0)
    eng = m.engine
    wav = audio(32, 160000, 1234)
    n_q = m.arch.num_quantizers
    old = eng.micro_batch
    eng.micro_batch = 32
    eng.read_profile()
    eng.set_profiling(True)
    try:
        a = eng.encode_decode(wav.cuda(), n_q, use_scale=True)
        prof = eng.read_profile()
    finally:
        eng.set_profiling(False)
        eng.micro_batch = old
    eng.check_status()
    assert _lstm_classes(prof) == {"lstm_wave_kernel"}, prof
    assert a["codes"].shape == (n_q, 32, 501)
    for i in (0, 15, 16, 31):
        one = eng.encode_decode(wav[i:i + 1].cuda(), n_q, use_scale=True)
        assert torch.equal(one["codes"][:, 0], a["codes"][:, i]), i
        assert torch.equal(one["recon"][0], a["recon"][i]) and torch.equal(one["quantized"][0], a["quantized"][i]), i
    eng.check_status()
    rows = [0, 31]
    o = orc.inference(wav[rows], bit_width=None, use_scale=True)
    got = a["codes"][:, rows].cpu()
    rep = index_report(got, o["code_indices"][0])
    if rep["frames_bad"]:
        _assert_flips_are_near_ties(orc.embed, o["encoder_out"], o["code_indices"][0], got, max_frames=1)
    else:
        ref_rms = float(o["recon_speech"].double().pow(2).mean().sqrt())
        assert rms(a["recon"][rows], o["recon_speech"]) < 1e-3 * ref_rms
        assert rms(a["quantized"][rows], o["code_embeddings"][0][0]) == 0.0
