"""The two ends of the STFT-domain codec (FreqCodec, model_type 1) per element against float64: the STFT front end's feature tensor in both
forms, and the back end -- spectrum from the decoder output, inverse-DFT GEMM, envelope division / trim / scale -- through
`Engine.freq_synthesis` (fc_freq_synthesis), which runs the very function run_decoder_2d calls behind the decoder's last conv.

Synthesis (references: float64 restatement of FreqCodec._decode_frame's arithmetic, oracle/freq_oracle.py's inverse_spectrogram):
  * pointwise: the captured spectrum rows against softplus(m) * (re, im) (mag_phase) and softplus(m) * (cos, sin)(sin(o1) pi) (mag_angle)
    with the pending affine applied in double first.  Planted: m at -100, -20, 0, 19.999, 20, 20.001, 60 and, between the two plausible
    softplus thresholds, 10.001, 10.5, 12, 15 (softplus(m) - m is 4.5e-5 at 10 and 2e-9 at 20: only values just above 10 can tell a
    threshold of 10 from one of 20 in float32); o1 at 0, +-pi/2, +-pi, +-10, +-50; per-row, per-channel affines; the DC and Nyquist rows.
  * the inverse STFT alone: the captured float32 spectrum, as complex128, through inverse_spectrogram, sample by sample; the first n_fft
    samples, the last n_fft samples of the full length and the interior are asserted separately.  Tp in {2, 3, taps, taps + 1, 17, 64},
    out_len in {1, 2, hop - 1, hop, 1023, 1024, 1025, full - 1, full}, with and without a per-row scale at B = 3, large imaginary parts in
    the DC and Nyquist rows (torch.istft ignores them), a single bin at frame 0 and at the last frame.
  * refusals on the host, and bit identity across batch position and calls.

Analysis (references: oracle/freq_oracle.py's spectrogram on float64 audio): the mag_angle form (atan2f) and the mag_phase form, with and
without audio_normalize (the div path of polyphase_in_kernel), B = 3 rows of loudness x1, x0.01, x30, at T = n_fft / 2 + 1, n_fft / 2 + 2,
k hop - 1, k hop, k hop + 1 and 3999; n_fft 512 / hop 160 and n_fft 64 / hop 24 (neither hop divides its n_fft).

Bars.  Analysis: the project's 2e-5 x top on magnitude-weighted errors (tests/test_freq_layers.py), with top the largest magnitude of the
utterance's own row, so a quiet row is not judged by a loud one's scale.  Spectrum and waveform: 12 x the max error of the same operation in
torch float32 on the CPU against float64 (the margin of tests/test_conv_layers.py: the engine's GEMM order and expf / log1pf / sinf / cosf
are not torch's), above a floor, and never above LAYER_ABS_TOL (5e-5) on the spectrum or WAV_RMS_TOL (1e-4) on the waveform.  Spectrum errors are taken relative to
max(1, |reference bin|) per element (the size of the complex bin: where the angle puts one part near zero the other part's size still
sets that part's rounding), waveform errors relative to the row's largest reference sample; torch's error is taken over the same
region as the engine's.  Floors: 1e-6 on the spectrum (16 float32 epsilons of a pointwise result); on the waveform sqrt(K) float32 unit
roundoffs of the row's peak, K = 2 F taps being the inverse-DFT GEMM's reduction length (_wave_floor) -- torch.istft is an FFT, whose float32
error (1.2e-7 of the peak) is an order below what any length-2056 float32 sum can give, so 12 x its error alone is no bar for a GEMM: the
first run on the hardware measured the engine at 1.5e-6 of the peak there.

Measured on an MI355X (max over the cases of each group; engine vs float64 / torch float32 vs float64, in the units above):
  spectrum            tinyfreq 1.8e-7 / 2.2e-7   tinyfreqang 5.5e-7 / 8.6e-7   tinyfreqgr1wnc 1.7e-7 / 2.3e-7   freqmp 1.7e-7 / 2.4e-7
                      fuzz64hop24 1.4e-7 / 1.9e-7
  waveform, Tp x len  tinyfreq 1.5e-6 / 2.2e-7   tinyfreqang 2.2e-6 / 2.5e-7   tinyfreqgr1wnc 1.6e-6 / 2.1e-7   freqmp 2.1e-6 / 2.3e-7
                      fuzz64hop24 5.4e-7 / 1.4e-7
  waveform, edges     tinyfreq 1.5e-6 / 1.8e-7   tinyfreqang 1.8e-6 / 2.3e-7   tinyfreqgr1wnc 1.7e-6 / 1.8e-7   freqmp 1.7e-6 / 1.8e-7
                      fuzz64hop24 6.0e-7 / 1.6e-7
  features (x top)    tinyfreqang log-magnitude 1.0e-6, angle 5.6e-7   tinyfreqangraw 1.1e-6, 5.8e-7
                      fuzz64hop24 log-magnitude 4.4e-7, phase 1.5e-7 / 1.8e-7   fuzz64hop24raw 6.8e-7, 1.7e-7 / 1.5e-7
The waveform sits at 7 - 9 x torch's FFT and under the sqrt(K) floor (2.7e-6, 8.4e-7); every other figure is at or below torch float32's.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_freq_layers import CONFIGS, LAYER_ABS_TOL, NETS, _freq_parts
from test_gpu_parity import WAV_RMS_TOL

pytestmark = pytest.mark.gpu

FEATURE_TOL = 2e-5            # x the row's largest magnitude (test_stft_features_mag_phase_against_float64_stft)
K32 = 12.0                    # x torch float32's own max error (tests/test_conv_layers.py ABS_K)
FLOOR = 1e-6                  # 16 float32 epsilons
SYNTH_NETS = ("tinyfreq", "tinyfreqang", "tinyfreqgr1wnc", "freqmp", "fuzz64hop24")
M_PLANTED = (-100.0, -20.0, 0.0, 19.999, 20.0, 20.001, 60.0, 10.001, 10.5, 12.0, 15.0)
O1_PLANTED = (0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, 10.0, -10.0, 50.0, -50.0)


def _no_normalize(name):
    from funcodec_amd.config import freq_recipe_config
    cfg = CONFIGS[name]() if name in CONFIGS else freq_recipe_config(name)
    cfg["model_conf"] = dict(cfg["model_conf"], audio_normalize=False)
    return cfg


# nets of this file only: the analysis nets without the volume normalisation
LOCAL = {"tinyfreqangraw": ("tinyfreqang", 10), "fuzz64hop24raw": ("fuzz64hop24", 16)}


@functools.lru_cache(maxsize=2)
def _local_parts(name):
    from freq_oracle import FreqOracle
    from funcodec_amd.config import arch_from_config
    from funcodec_amd.model import EncodecMI355X
    from funcodec_amd.synth import make_freq_state_dict
    base, seed = LOCAL[name]
    cfg = _no_normalize(base)
    sd = {k: torch.from_numpy(v) for k, v in make_freq_state_dict(cfg, seed).items()}
    m = EncodecMI355X(arch_from_config(cfg), "cuda:0")
    m.load_state_dict(sd)
    return m, FreqOracle(cfg, sd)


def _parts(net):
    if net in LOCAL:
        return _local_parts(net)
    return _freq_parts(net, NETS[net][0] if net in NETS else 16)


def _worst(d):
    """(largest element, its index) of an error tensor."""
    i = int(d.argmax())
    return float(d.flatten()[i]), tuple(int(v) for v in np.unravel_index(i, tuple(d.shape)))


def _report(case, **facts):
    from conftest import record_report
    record_report(case, **{k: (float(f"{v:.3g}") if isinstance(v, float) else v) for k, v in facts.items()})
    print(case, {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in facts.items()})


# ---- synthesis: references ----------------------------------------------------------------------------------------------------------
def _affine(B, C):
    """[B, C, 2] (scale, shift), every row and channel clearly its own."""
    sc = torch.tensor([[0.7 + 0.45 * b, 1.9 - 0.4 * b, -1.3 + 0.25 * b][:C] for b in range(B)])
    sh = torch.tensor([[0.3 - 0.5 * b, -0.8 + 0.3 * b, 0.9 * b - 0.4][:C] for b in range(B)])
    return torch.stack([sc, sh], -1).float()


def _planted_dec(orc, B, Tp, gen, aff):
    """Unit-scale random decoder output [B, C, F, Tp] with the planted magnitudes (and angles) at scattered positions, the DC and Nyquist
    rows included, such that the affine maps the stored value onto the planted one (to float32 rounding)."""
    C, Fq = orc.in_ch, orc.n_fft // 2 + 1
    dec = torch.randn(B, C, Fq, Tp, generator=gen, dtype=torch.float64)
    rows = [0, Fq - 1, 1, Fq // 2, Fq - 2, 7 % Fq]

    def raw(b, c, v):
        return v if aff is None else (v - float(aff[b, c, 1])) / float(aff[b, c, 0])
    n = 0
    for b in range(B):
        for i, mv in enumerate(M_PLANTED):
            for j, o1 in enumerate(O1_PLANTED if C == 2 else (None,)):
                f, t = rows[n % len(rows)], (3 * n + b) % Tp
                n += 1
                dec[b, 0, f, t] = raw(b, 0, mv)
                if o1 is not None:
                    dec[b, 1, f, t] = raw(b, 1, o1)
                else:                                   # a phase of unit size, so the magnitude's error shows in both parts
                    dec[b, 1, f, t], dec[b, 2, f, t] = raw(b, 1, 0.9), raw(b, 2, -1.1)
    return dec.float()


def _spectrum_ref(orc, dec, aff, dtype):
    """[B, 2F, Tp]: FreqCodec._decode_frame's spectrum (codec_freq.py:419-434) of aff(dec) in `dtype`, real rows then imaginary rows."""
    v = dec.to(dtype)
    if aff is not None:
        a = aff.to(dtype)
        v = v * a[:, :, 0, None, None] + a[:, :, 1, None, None]
    m = v[:, 0]
    sp = F.softplus(m) if dtype == torch.float32 else torch.logaddexp(m, torch.zeros_like(m))
    if orc.in_ch == 2:
        ang = torch.sin(v[:, 1]) * torch.pi
        return torch.cat([torch.cos(ang) * sp, torch.sin(ang) * sp], 1)
    return torch.cat([sp * v[:, 1], sp * v[:, 2]], 1)


def _check_spectrum(orc, dec, aff, spec, tag):
    """Per element, relative to max(1, |reference bin|) (the complex bin's size).  mag_angle elements whose angle input exceeds 4 in size (the planted +-10, +-50) are
    judged apart from the others: float32 resolves such an input, and so the angle, only to 4e-6, and torch float32's error there would
    otherwise set the bar for every element.  Returns (engine, torch float32) max errors over the ordinary elements."""
    ref = _spectrum_ref(orc, dec, aff, torch.float64)
    t32 = _spectrum_ref(orc, dec, aff, torch.float32)
    Fq = orc.n_fft // 2 + 1
    den = torch.hypot(ref[:, :Fq], ref[:, Fq:]).clamp(min=1.0).repeat(1, 2, 1)       # max(1, |re + i im|): both parts carry the magnitude's error
    d, d32 = (spec.double() - ref).abs() / den, (t32.double() - ref).abs() / den
    big = torch.zeros_like(ref, dtype=torch.bool)
    if orc.in_ch == 2:
        o1 = dec[:, 1].double() if aff is None else dec[:, 1].double() * aff[:, 1, 0, None, None].double() + aff[:, 1, 1, None, None].double()
        big = (o1.abs() > 4.0).repeat(1, 2, 1)
    out = None
    for name, sel in (("", ~big), (" (large angle inputs)", big)):
        if not bool(sel.any()):
            continue
        e, at = _worst(torch.where(sel, d, torch.zeros_like(d)))
        e32, _ = _worst(torch.where(sel, d32, torch.zeros_like(d32)))
        bar = min(max(FLOOR, K32 * e32), LAYER_ABS_TOL)
        where = f"(b, row, t) = {at} ({'im' if at[1] >= Fq else 're'} of bin {at[1] % Fq}), engine {float(spec[at]):.9g}, float64 {float(ref[at]):.9g}"
        assert e <= bar, f"{tag}{name}: spectrum error {e:.3e} above {bar:.3e} (torch float32 {e32:.3e}) at {where}"
        out = out or (e, e32)
    return out


def _istft_refs(orc, spec, scale):
    """The waveform of the captured float32 spectrum [B, 2F, Tp] in float64 and in torch float32: [B, hop (Tp - 1)] each."""
    from freq_oracle import inverse_spectrogram
    Fq = orc.n_fft // 2 + 1
    sc = torch.complex(spec[:, :Fq].double(), spec[:, Fq:].double())
    ref = inverse_spectrogram(sc, orc.n_fft, orc.stft_hop)
    t32 = inverse_spectrogram(sc.to(torch.complex64), orc.n_fft, orc.stft_hop)
    if scale is not None:
        ref = ref * scale.double()[:, None]
        t32 = t32 * scale[:, None]
    return ref, t32


def _check_wave(orc, wav, ref, t32, tag):
    """wav [B, out_len] against the first out_len samples of ref, t32 [B, full], per sample relative to the row's largest reference sample;
    the first n_fft samples, the last n_fft samples of the full length and the interior separately.  Returns (engine, torch float32)."""
    out_len, full, N = wav.shape[1], ref.shape[1], orc.n_fft
    assert ref.shape[0] == wav.shape[0] and out_len <= full
    top = ref.abs().amax(dim=1, keepdim=True).clamp(min=1e-30)
    d = (wav.double() - ref[:, :out_len]).abs() / top
    d32 = (t32.double() - ref).abs()[:, :out_len] / top
    assert torch.isfinite(wav).all(), f"{tag}: non-finite samples"
    idx = torch.arange(out_len)
    head, tail = idx < N, idx >= full - N
    worst = (0.0, 0.0)
    for name, sel in (("first n_fft samples", head), ("last n_fft samples", tail & ~head), ("interior", ~head & ~tail)):
        if not bool(sel.any()):
            continue
        pos = idx[sel]
        e, at = _worst(d[:, sel])
        e32, _ = _worst(d32[:, sel])
        bar = min(max(_wave_floor(orc), K32 * e32), WAV_RMS_TOL)
        b, i = at[0], int(pos[at[1]])
        assert e <= bar, (f"{tag}, {name}: error {e:.3e} of the row's peak above {bar:.3e} (torch float32 {e32:.3e}) at (b, sample) = ({b}, {i}) "
                          f"of out_len {out_len}, full {full}: engine {float(wav[b, i]):.9g}, float64 {float(ref[b, i]):.9g}")
        worst = (max(worst[0], e), max(worst[1], e32))
    return worst


def _wave_floor(orc):
    """sqrt(K) float32 unit roundoffs of the row's peak, K = 2 F taps the inverse-DFT GEMM's reduction length: the usual estimate of the
    rounding error of a length-K float32 sum whose partial sums are of the size of the result (2.7e-6 at n_fft 512 / hop 160, 8.4e-7 at
    64 / 24).  torch.istft's float32 FFT sums in log2(n_fft) stages and stays below it."""
    return math.sqrt(2 * (orc.n_fft // 2 + 1) * _taps(orc)) * 2.0 ** -24


def _out_lens(hop, full):
    return sorted({n for n in (1, 2, hop - 1, hop, 1023, 1024, 1025, full - 1, full) if 1 <= n <= full})


def _taps(orc):
    return -(-orc.n_fft // orc.stft_hop)


# ---- synthesis: tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", SYNTH_NETS)
def test_spectrum_from_decoder_output_against_float64(net):
    """spec_from_dec_kernel<2 | 3> per element: planted magnitudes around both softplus branches and far out, planted angles, B = 3 rows
    with their own affines (every channel its own), the same call without an affine, and the net's own form (weight_norm: none)."""
    m, orc = _parts(net)
    gen = torch.Generator().manual_seed(100 + len(net))
    B = 3
    worst = (0.0, 0.0)
    for Tp in (23, 64):
        for aff in (_affine(B, orc.in_ch), None):
            dec = _planted_dec(orc, B, Tp, gen, aff)
            wav, spec = m.engine.freq_synthesis(dec.cuda(), None if aff is None else aff.cuda(), want_spec=True)
            assert spec.shape == (B, 2 * (orc.n_fft // 2 + 1), Tp) and wav.shape == (B, orc.stft_hop * (Tp - 1))
            e = _check_spectrum(orc, dec, aff, spec.cpu(), f"{net} Tp={Tp} {'affine' if aff is not None else 'no affine'}")
            worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    m.engine.check_status()
    _report("freq_stft_spectrum_" + net, engine=worst[0], torch32=worst[1])


@pytest.mark.parametrize("net", SYNTH_NETS)
def test_inverse_stft_against_float64_per_sample(net):
    """The inverse-DFT GEMM and istft_finish_kernel on the captured spectrum: every Tp x out_len, with and without a per-row scale, B = 3."""
    m, orc = _parts(net)
    hop = orc.stft_hop
    gen = torch.Generator().manual_seed(200 + len(net))
    B = 3
    taps = _taps(orc)
    scale = torch.tensor([0.37, 1.0, 23.0])
    worst = (0.0, 0.0)
    for Tp in sorted({2, 3, taps, taps + 1, 17, 64}):
        full = hop * (Tp - 1)
        dec = torch.randn(B, orc.in_ch, orc.n_fft // 2 + 1, Tp, generator=gen)
        for sc in (None, scale):
            refs, spec0 = None, None
            for out_len in _out_lens(hop, full):
                wav, spec = m.engine.freq_synthesis(dec.cuda(), None, None if sc is None else sc.cuda(), out_len=out_len, want_spec=True)
                assert wav.shape == (B, out_len)
                wav, spec = wav.cpu(), spec.cpu()
                if refs is None:
                    refs, spec0 = _istft_refs(orc, spec, sc), spec
                assert torch.equal(spec, spec0), "the spectrum does not depend on out_len"
                e = _check_wave(orc, wav, refs[0], refs[1], f"{net} Tp={Tp} out_len={out_len} {'scale' if sc is not None else 'no scale'}")
                worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    m.engine.check_status()
    _report("freq_stft_istft_" + net, engine=worst[0], torch32=worst[1])


@pytest.mark.parametrize("net", SYNTH_NETS)
def test_inverse_stft_ignores_dc_and_nyquist_imaginary_parts_and_places_single_bins(net):
    """Large imaginary parts in the DC and Nyquist rows (torch.istft drops them), and a spectrum that is one bin at frame 0 / at the last
    frame (every other magnitude is softplus(-100) = 4e-44): the samples next to both ends, where the frame range is clamped."""
    m, orc = _parts(net)
    hop, Fq, C = orc.stft_hop, orc.n_fft // 2 + 1, orc.in_ch
    gen = torch.Generator().manual_seed(300 + len(net))
    Tp, B = 17, 3
    dec = torch.randn(B, C, Fq, Tp, generator=gen)
    for f in (0, Fq - 1):
        if C == 3:
            dec[:, 2, f] *= 50.0                       # imaginary part ~ 50 x the real part
        else:
            dec[:, 0, f] = 30.0 + dec[:, 0, f]         # mag_angle: |spectrum| = 30, the angle sets both parts
    wav, spec = m.engine.freq_synthesis(dec.cuda(), None, None, want_spec=True)
    spec = spec.cpu()
    assert float(spec[:, Fq].abs().max()) > 25.0 and float(spec[:, 2 * Fq - 1].abs().max()) > 25.0
    _check_spectrum(orc, dec, None, spec, f"{net} dc/nyquist")
    ref, t32 = _istft_refs(orc, spec, None)
    worst = _check_wave(orc, wav.cpu(), ref, t32, f"{net} dc/nyquist imaginary parts")
    for Tp in (2, 17):
        for frame in (0, Tp - 1):
            for f in (0, 5 % Fq, Fq - 1):
                dec = torch.zeros(1, C, Fq, Tp)
                dec[:, 0] = -100.0
                dec[0, 0, f, frame] = 5.0
                dec[0, 1] = 0.6
                if C == 3:
                    dec[0, 2] = 0.8
                full = hop * (Tp - 1)
                for out_len in sorted({1, min(hop, full), full - 1, full} - {0}):
                    wav, spec = m.engine.freq_synthesis(dec.cuda(), None, None, out_len=out_len, want_spec=True)
                    spec = spec.cpu()
                    assert int((spec.abs() > 1e-30).sum()) in (1, 2), "one bin (its real and / or imaginary part)"
                    ref, t32 = _istft_refs(orc, spec, None)
                    assert float(ref.abs().max()) > 1e-4
                    e = _check_wave(orc, wav.cpu(), ref, t32, f"{net} single bin {f} at frame {frame} of {Tp}, out_len={out_len}")
                    worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    m.engine.check_status()
    _report("freq_stft_istft_edges_" + net, engine=worst[0], torch32=worst[1])


def test_freq_synthesis_refusals_leave_the_engine_working():
    from funcodec_amd.engine import EngineError
    from helpers import engine_for
    m, orc = _parts("tinyfreq")
    eng, hop, Fq = m.engine, orc.stft_hop, orc.n_fft // 2 + 1
    gen = torch.Generator().manual_seed(4)
    dec = torch.randn(2, 3, Fq, 5, generator=gen).cuda()
    before = eng.freq_synthesis(dec)
    with pytest.raises(EngineError, match="not an STFT-domain codec"):
        engine_for("tiny", 7).engine.freq_synthesis(dec)
    with pytest.raises(EngineError, match="dec has 2 channels, the decoder's output has 3"):
        eng.freq_synthesis(dec[:, :2])
    with pytest.raises(EngineError, match=f"dec has {Fq - 1} frequency rows, n_fft / 2 \\+ 1 is {Fq}"):
        eng.freq_synthesis(dec[:, :, :-1])
    with pytest.raises(EngineError, match="at least 2 frames, got 1"):
        eng.freq_synthesis(dec[..., :1])
    for bad in (0, -1, hop * 4 + 1):
        with pytest.raises(EngineError, match=f"out_len {bad} is outside \\[1, stft_hop \\* \\(frames - 1\\)\\] = \\[1, {hop * 4}\\]"):
            eng.freq_synthesis(dec, out_len=bad)
    with pytest.raises(EngineError, match="dec must be"):
        eng.freq_synthesis(dec[0])
    with pytest.raises(EngineError, match="one value per utterance"):
        eng.freq_synthesis(dec, scale=torch.ones(3))
    with pytest.raises(EngineError, match="the affine must be"):
        eng.freq_synthesis(dec, aff=torch.ones(2, 2, 2))
    assert torch.equal(eng.freq_synthesis(dec), before)
    eng.check_status()


@pytest.mark.parametrize("net", ("tinyfreq", "tinyfreqang", "fuzz64hop24"))
def test_freq_synthesis_rows_do_not_depend_on_the_batch(net):
    """The same decoder row gives the same bits as row 0 of B = 1 and as row 2 of B = 4, and a repeated call returns the same bits."""
    m, orc = _parts(net)
    gen = torch.Generator().manual_seed(500)
    Tp, C, Fq = 33, orc.in_ch, orc.n_fft // 2 + 1
    dec = torch.randn(4, C, Fq, Tp, generator=gen).cuda()
    aff = _affine(4, C).cuda()
    scale = torch.tensor([3.0, 0.2, 1.7, 11.0]).cuda()
    w4, s4 = m.engine.freq_synthesis(dec, aff, scale, want_spec=True)
    w4b, s4b = m.engine.freq_synthesis(dec, aff, scale, want_spec=True)
    assert torch.equal(w4, w4b) and torch.equal(s4, s4b)
    w1, s1 = m.engine.freq_synthesis(dec[2:3], aff[2:3], scale[2:3], want_spec=True)
    assert torch.equal(s1[0], s4[2]), _worst((s1[0] - s4[2]).abs().cpu())
    assert torch.equal(w1[0], w4[2]), _worst((w1[0] - w4[2]).abs().cpu())
    m.engine.check_status()


# ---- analysis ------------------------------------------------------------------------------------------------------------------------
def _lengths(orc):
    N, hop = orc.n_fft, orc.stft_hop
    k = -(-(N // 2 + 2) // hop)                          # the smallest k with k hop - 1 > n_fft / 2
    return [N // 2 + 1, N // 2 + 2, k * hop - 1, k * hop, k * hop + 1, 3999]


def _wrap(a):
    return torch.remainder(a + math.pi, 2 * math.pi) - math.pi


@pytest.mark.parametrize("net", ("tinyfreqang", "tinyfreqangraw", "fuzz64hop24", "fuzz64hop24raw"))
def test_stft_features_both_forms_against_float64_stft(net):
    """stft_feats_kernel<2> (log-magnitude, atan2f angle; compared modulo 2 pi, weighted by the magnitude) and <3> behind
    polyphase_in_kernel with and without its divisor, B = 3 rows of loudness x1, x0.01, x30, at the lengths where the frame count
    1 + T // hop and the right-hand reflection change."""
    from freq_oracle import spectrogram
    from helpers import audio
    m, orc = _parts(net)
    Fq, B = orc.n_fft // 2 + 1, 3
    assert orc.audio_normalize == (not net.endswith("raw")) and orc.in_ch == (2 if "ang" in net else 3)
    worst = {}
    for T in _lengths(orc):
        wav = audio(B, T, 7000 + T, "tones") * torch.tensor([1.0, 0.01, 30.0])[:, None]
        x = wav.double()
        if orc.audio_normalize:
            x = x / (1e-8 + x.pow(2).mean(dim=1, keepdim=True).sqrt())
        xc = spectrogram(x, orc.n_fft, orc.stft_hop)
        mag = xc.abs()
        Tp = 1 + T // orc.stft_hop
        assert xc.shape == (B, Fq, Tp)
        cap = torch.full((B, orc.in_ch, Fq, Tp), float("nan"), dtype=torch.float32, device="cuda")
        m.engine.debug_freq_features(cap, 1)
        m.engine.encode(wav.cuda(), 1)
        torch.cuda.synchronize()
        got = cap.cpu().double()
        assert torch.isfinite(got).all(), (net, T, "the feature tensor has [B, C, n_fft / 2 + 1, 1 + T // hop] elements")
        top = mag.amax(dim=(1, 2), keepdim=True)
        errs = {"log-magnitude": (got[:, 0].exp() - mag.clamp(min=1e-6)).abs() / top}
        if orc.in_ch == 2:
            errs["angle"] = _wrap(got[:, 1] - torch.angle(xc)).abs() * mag / top
        else:
            ph = xc / mag.clamp(min=1e-6)
            errs["phase re"] = (got[:, 1] - ph.real).abs() * mag / top
            errs["phase im"] = (got[:, 2] - ph.imag).abs() * mag / top
        for what, d in errs.items():
            e, at = _worst(d)
            worst[what] = max(worst.get(what, 0.0), e)
            assert e < FEATURE_TOL, f"{net} T={T} {what}: {e:.3e} of the row's largest magnitude at (b, bin, frame) = {at} of {Tp} frames"
    m.engine.check_status()
    _report("freq_stft_features_" + net, **worst)
