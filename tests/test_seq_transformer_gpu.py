"""The transformer bottleneck (encoder_conf / decoder_conf ``seq_model: transformer``) on the MI355X: the block against a float64
restatement of the reference's semantics, the whole codec against the real reference's fixtures (tests/golden/MANIFEST_seqtf.json,
tools/make_golden_seqtf.py), causality, determinism / batch independence and the drop-in Speech2Token."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from helpers import audio, golden, index_report, rms
from test_gpu_parity import WAV_RMS_TOL, _assert_flips_are_near_ties, _prefix_before

from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.plan import encoder_plan
from funcodec_amd.synth import make_freq_state_dict, make_state_dict

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAN = json.load(open(os.path.join(GOLD, "MANIFEST_seqtf.json")))
BLOCK_ABS_TOL = 1e-5        # max |engine - float64| over a whole 2-block stack (the LSTM block bar); measured <= 2.9e-6
BLOCK_RMS_TOL = 1e-6        # measured <= 4.6e-7


def _state(cfg, seed):
    arch = arch_from_config(cfg)
    return arch, (make_freq_state_dict(cfg, seed) if arch.model_type == "freq_codec" else make_state_dict(arch, seed))


@functools.lru_cache(maxsize=4)
def _engine(cfg_name, seed):
    from funcodec_amd.model import EncodecMI355X
    arch, sd = _state(recipe_config(cfg_name), seed)
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m, sd


# ---- 1. the block against float64 ---------------------------------------------------------------------------------------------
def _ln(x, sd, key):
    return torch.nn.functional.layer_norm(x, x.shape[-1:], sd[key + ".weight"], sd[key + ".bias"], eps=1e-12)


def transformer_f64(x, sd, prefix, blocks, causal, skip, heads=4):
    """TransformerEncoder.forward (normed_modules/transformer.py:150-208) with input_layer None, no length mask, dropout 0:
    EncoderLayer (transformer_encoder.py:92-150, normalize_before) x blocks, after_norm, + x if skip.  x [B, C, T] float64."""
    sd = {k: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith(prefix + ".")}
    xs = x.double().permute(0, 2, 1)
    res = xs
    B, T, C = xs.shape
    dk = C // heads
    lin = lambda h, k: h @ sd[k + ".weight"].T + sd[k + ".bias"]
    for l in range(blocks):
        p = f"{prefix}.encoders.{l}"
        h = _ln(xs, sd, p + ".norm1")
        q, k, v = (lin(h, f"{p}.self_attn.linear_{n}").view(B, T, heads, dk).transpose(1, 2) for n in "qkv")
        s = q @ k.transpose(-2, -1) / np.sqrt(dk)
        if causal:
            s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
        ctx = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, C)
        xs = xs + lin(ctx, f"{p}.self_attn.linear_out")
        h = _ln(xs, sd, p + ".norm2")
        xs = xs + lin(torch.relu(lin(h, f"{p}.feed_forward.w_1")), f"{p}.feed_forward.w_2")
    xs = _ln(xs, sd, prefix + ".after_norm")
    if skip:
        xs = xs + res
    return xs.permute(0, 2, 1)


@functools.lru_cache(maxsize=2)
def _block_engine(C, causal):
    """A small codec whose bottleneck is C wide (ratios [4, 2]: C = 4 n_filters) with a 2-block transformer; causal attention comes
    with the causal weight_norm nets (the reference ties TransformerEncoder's causal_mode to the convs' `causal`)."""
    from funcodec_amd.model import EncodecMI355X
    cfg = recipe_config("tinytf")
    for k in ("encoder_conf", "decoder_conf"):
        cfg[k]["n_filters"] = C // 4
        if causal:
            cfg[k].update(norm="weight_norm", causal=True)
            cfg[k].pop("norm_params", None)
    arch, sd = _state(cfg, 100 + C)
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    prefix = [op.key for op in encoder_plan(arch) if op.kind == "transformer"][0]
    return m, sd, prefix, arch


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("C", [64, 128, 256, 512, 1024])
def test_block_against_float64(C, causal):
    m, sd, prefix, arch = _block_engine(C, causal)
    worst = []
    for B in (1, 3):
        for T in (1, 5, 250, 3001):            # 3001: far past what a kernel holding a whole score row in LDS could take
            g = torch.Generator().manual_seed(C * 7919 + B * 31 + T)
            x = torch.randn(B, C, T, generator=g)
            y = m.engine.seq_forward(prefix, x.cuda()).cpu().double()
            ref = transformer_f64(x, sd, prefix, arch.lstm_layers, causal, arch.lstm_skip)
            e_max, e_rms = float((y - ref).abs().max()), float((y - ref).pow(2).mean().sqrt())
            worst.append((B, T, e_max, e_rms))
            assert bool(torch.isfinite(y).all())
            assert e_max < BLOCK_ABS_TOL and e_rms < BLOCK_RMS_TOL, (B, T, e_max, e_rms)
    print(f"C={C} causal={causal}: (B, T, max abs, rms) {worst}")


def test_causal_attention_does_not_see_later_frames():
    """A frame's block output is bitwise independent of later frames (masked keys add exactly nothing)."""
    m, sd, prefix, arch = _block_engine(256, True)
    x = torch.randn(2, 256, 777, generator=torch.Generator().manual_seed(5))
    x2 = x.clone()
    x2[:, :, 400:] = torch.randn(2, 256, 377, generator=torch.Generator().manual_seed(6)) * 3
    y, y2 = m.engine.seq_forward(prefix, x.cuda()).cpu(), m.engine.seq_forward(prefix, x2.cuda()).cpu()
    assert torch.equal(y[:, :, :400], y2[:, :, :400]) and not torch.equal(y[:, :, 400:], y2[:, :, 400:])
    # the work accounting of this engine = the kernel dispatches of one fc_encode_decode(B 2, T 4000) in a rocprofv3 kernel trace (per
    # transformer block: two LayerNorms, the attention, the ReLU and four GEMMs)
    w = m.engine.work(2, 4000, arch.num_quantizers)
    assert (w["total_launches"], w["conv_launches"]) == (60, 34), w


# ---- 2. end to end against the real reference ----------------------------------------------------------------------------------
E2E = sorted(n for n, c in MAN["cases"].items() if c["kind"] in ("e2e", "freq"))
SEG = sorted(n for n, c in MAN["cases"].items() if c["kind"] == "segmented")


def _ref_quantized(g, sd):
    """The reference's quantised embedding [B, Tf, D]: stored, or (slim fixtures) re-created exactly as the reference forms it -- the
    codebook rows of the stored indices summed in stage order in fp32, from 0 (ddp_core_vq.py:407-408)."""
    if "quantized" in g:
        return g["quantized"]
    E, idx = sd["quantizer.rq.model.embed"], g["indices"].astype(np.int64)
    acc = np.zeros((idx.shape[1], idx.shape[2], E.shape[2]), np.float32)
    for i in range(idx.shape[0]):
        acc = acc + E[i][idx[i]]
    return acc


def _ref_recon(g, c):
    """The reference's reconstruction [B, C, n] and the sample its first column is: all of it, or (slim fixtures) the window
    `recon_window` of every utterance."""
    if "recon" in g:
        return g["recon"], 0
    return g["recon_excerpt"], c["recon_window"][0]


@pytest.mark.parametrize("name", E2E)
def test_e2e_against_reference_golden(name):
    """The bars of tests/test_gpu_parity.py::test_e2e_against_reference_golden: codes equal on every frame or each differing frame a
    proven fp32 tie, encoder output 2e-5 rms, waveform 1e-4 rms, the decode of the reference's own codes."""
    c = MAN["cases"][name]
    m, sd = _engine(c["config"], c["weight_seed"])
    wav = audio(c["batch"], c["samples"], c["audio_seed"], c["audio_kind"])
    g = golden(name)
    r = m.engine.encode(wav, c["n_q"], want_enc_out=True)
    e_enc = rms(r["enc_out"], g["encoder_out"])
    assert e_enc < 2e-5, e_enc
    assert float(((r["scale"].cpu() - torch.from_numpy(g["scale"])).abs() / torch.from_numpy(g["scale"])).max()) < 1e-5
    rep = index_report(r["codes"], g["indices"].astype(np.int64))
    r2 = m.engine.encode_decode(wav, c["n_q"], use_scale=True)
    assert torch.equal(r2["codes"], r["codes"])
    qref = _ref_quantized(g, sd)
    rref, lo = _ref_recon(g, c)
    hi = lo + rref.shape[-1]
    proofs = []
    if rep["mismatched_indices"]:
        proofs = _assert_flips_are_near_ties(sd["quantizer.rq.model.embed"], torch.from_numpy(g["encoder_out"]), g["indices"].astype(np.int64),
                                             r["codes"], got_enc=r["enc_out"].cpu(), max_frames=max(1, rep["frames"] // 250))
        Tf, hop = g["indices"].shape[2], m.engine.hop_length
        for b in range(c["batch"]):
            # the waveform of an utterance without a tie matches whole; with one, a causal net still matches up to the tied frame's
            # neighbourhood, while through non-causal attention every frame of the decoded utterance sees the flipped code
            cut = _prefix_before([p[1] for p in proofs], Tf, hop, b)
            n = min(hi, c["samples"] if cut is None else (min(cut, c["samples"]) if m.arch.causal else 0))
            if n > lo:
                assert rms(r2["recon"][b, :, lo:n], rref[b, :, :n - lo]) < WAV_RMS_TOL, (b, lo, n)
    else:
        assert rms(r["quantized"], qref) == 0.0
        e_wav = rms(r2["recon"][..., lo:hi], rref)
        assert e_wav < WAV_RMS_TOL, e_wav
    tok = torch.from_numpy(g["indices"].astype(np.int64)).permute(1, 2, 0).contiguous()
    w2, emb = m.engine.decode_codes(tok)
    assert rms(emb, qref) == 0.0
    if "recon_from_codes" in g:
        n = g["recon_from_codes"].shape[-1]
        assert w2.shape[-1] >= n and rms(w2[..., :n], g["recon_from_codes"]) < WAV_RMS_TOL
    else:                                          # un-scaled decode x the reference's scale == its scaled reconstruction
        sc = torch.from_numpy(g["scale"]).view(-1, 1, 1)
        assert rms(w2.cpu()[..., lo:hi] * sc, rref) < WAV_RMS_TOL
    print(f"{name}: encoder_out rms {e_enc:.2e}, {rep['mismatched_indices']} differing indices, tie proofs {proofs}")


@pytest.mark.parametrize("name", SEG)
def test_segmented_against_reference_golden(name):
    c = MAN["cases"][name]
    m, sd = _engine(c["config"], c["weight_seed"])
    wav = audio(c["batch"], c["samples"], c["audio_seed"], c["audio_kind"])
    g = golden(name)
    r = m.inference(wav.unsqueeze(1), bit_width=c["bit_width"], use_scale=True)
    assert len(r["code_indices"]) == len(c["frames"])
    for f, idx in enumerate(r["code_indices"]):
        assert torch.equal(idx.cpu(), torch.from_numpy(g[f"indices_{f}"].astype(np.int64))), f
        assert np.allclose(r["code_embeddings"][f][1].cpu().numpy(), g[f"scale_{f}"], rtol=1e-5)
    assert rms(r["recon_speech"], g["recon"]) < WAV_RMS_TOL


# ---- 3. causality of the whole causal codec ------------------------------------------------------------------------------------
def test_causal_codec_frames_before_a_change_are_bitwise_equal():
    """ss320tfc: causal convs + causal attention.  Two inputs differ only after sample S (the tail is negated, so the volume scale --
    a sum of squares -- is bitwise the same); every frame whose receptive field ends before S has the same encoder output and codes."""
    m, sd = _engine("ss320tfc", 0)
    wav = audio(2, 32000, 17, "tones")
    S = 16000
    wav2 = wav.clone()
    wav2[:, S:] = -wav2[:, S:]
    a = m.engine.encode(wav, 32, want_enc_out=True)
    b = m.engine.encode(wav2, 32, want_enc_out=True)
    assert torch.equal(a["scale"], b["scale"])
    hop = m.engine.hop_length
    n = S // hop                                   # frame t reads samples < (t + 1) * hop
    assert torch.equal(a["enc_out"][:, :n], b["enc_out"][:, :n]) and torch.equal(a["codes"][:, :, :n], b["codes"][:, :, :n])
    assert not torch.equal(a["enc_out"][:, n + 2:], b["enc_out"][:, n + 2:])


# ---- 4. determinism and batch independence at the benchmark shape ---------------------------------------------------------------
def test_full_size_determinism_and_batch_independence():
    m, sd = _engine("ds640tf", 0)
    wav = audio(16, 160000, 1234, "noise")
    r = m.engine.encode_decode(wav, 32, use_scale=True)
    r2 = m.engine.encode_decode(wav, 32, use_scale=True)
    assert torch.equal(r2["codes"], r["codes"]) and torch.equal(r2["recon"], r["recon"])
    sub = m.engine.encode_decode(wav[5:8], 32, use_scale=True)
    assert torch.equal(sub["codes"], r["codes"][:, 5:8]) and torch.equal(sub["recon"], r["recon"][5:8])
    assert bool(torch.isfinite(r["recon"]).all())


# ---- 5. the drop-in surface ----------------------------------------------------------------------------------------------------
def test_speech2token_dropin(tmp_path):
    from funcodec_amd.bin.codec_inference import Speech2Token
    from funcodec_amd.synth import write_checkpoint
    name = "ds320tf_b2_t16000"
    c = MAN["cases"][name]
    arch, sd = _state(recipe_config(c["config"]), c["weight_seed"])
    cfg_path, pth_path = write_checkpoint(str(tmp_path), recipe_config(c["config"]), sd)
    s2t = Speech2Token(cfg_path, pth_path, device="cuda")
    g = golden(name)
    wav = audio(c["batch"], c["samples"], c["audio_seed"], c["audio_kind"])
    idx, embs, recon, subs = s2t(wav.unsqueeze(1), run_mod="inference")
    assert isinstance(idx, list) and idx[0].shape == g["indices"].shape
    rep = index_report(idx[0], g["indices"].astype(np.int64))
    if rep["mismatched_indices"]:
        m, _ = _engine(c["config"], c["weight_seed"])
        enc = m.engine.encode(wav, c["n_q"], want_enc_out=True)["enc_out"]
        _assert_flips_are_near_ties(sd["quantizer.rq.model.embed"], torch.from_numpy(g["encoder_out"]), g["indices"].astype(np.int64), idx[0],
                                    got_enc=enc.cpu(), max_frames=1)
    else:
        assert rms(embs[0][0], g["quantized"]) == 0.0 and rms(recon, g["recon"]) < WAV_RMS_TOL
    assert float(((embs[0][1].cpu() - torch.from_numpy(g["scale"])).abs() / torch.from_numpy(g["scale"])).max()) < 1e-5
