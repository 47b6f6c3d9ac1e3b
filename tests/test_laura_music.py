"""LauraTTS text-to-music recipe (egs/jamendo/text2music_laura, config ``lauramusic``): d_model 1024, 16 heads, feed-forward 4096 in
all three stacks, T5-base input width 768.

CPU tests: the recipe config, the feed-forward rule of the decoding step, the checkpoint contract and oracle/laura_oracle.py against the
goldens the REAL reference produced (tools/make_golden_laura_music.py).  GPU tests (`-m gpu`): the HIP engine against the same goldens
with the bars of tests/test_laura.py, the decoding step's GEMV at K = 4096 (x staged in LDS windows), the persistent step at d = 1024
(B <= 2; larger batches on the kernel chain) and the Text2Audio drop-in with a stand-in text embedder.  The e2e fixture's codec is the
FreqCodec ds640 recipe, a stand-in: the released model pairs with the universal nq32ds640 FreqCodec, whose config.yaml is not in the
reference tree.
"""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLD, golden, rms

from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
from funcodec_amd.synth import laura_plan, make_laura_state_dict, synthetic_audio, synthetic_text, synthetic_text_embedder

with open(os.path.join(GOLD, "MANIFEST_laura_music.json")) as f:
    MAN = json.load(f)
CASES = sorted(MAN["cases"])
SAME_BUILD = torch.__version__ == MAN["torch"] and torch.get_num_threads() == MAN["threads"]
LOGP_TOL = 2e-4


def case_inputs(name):
    c = MAN["cases"][name]
    cfg = laura_recipe_config(c["config"])
    sd = make_laura_state_dict(cfg, c["weight_seed"])
    text = synthetic_text(cfg, len(c["text_lengths"]), c["text_lengths"], c["text_seed"])
    spec = laura_spec_from_config(cfg)
    continual = None
    if c["continual_lengths"] is not None:
        rng = np.random.Generator(np.random.PCG64(c["text_seed"] + 1000))
        continual = [rng.integers(0, spec.codebook_size, size=(n, spec.predict_nq)).astype(np.int64) for n in c["continual_lengths"]]
    return c, cfg, spec, sd, text, continual


# ================================================================ CPU ================================================================
def test_music_recipe_config():
    spec = laura_spec_from_config(laura_recipe_config("lauramusic"))
    for s in (spec.codec_lm, spec.text_encoder, spec.codec_encoder):
        assert (s.d_model, s.heads, s.ff) == (1024, 16, 4096)
    assert spec.codec_lm.layers == 12 and spec.text_encoder.layers == 6 == spec.codec_encoder.layers
    assert spec.input_size == 768 and spec.vocab_size == 0 and spec.predict_nq == 2 and spec.lm_vocab == 2050
    assert laura_recipe_config("lauramusic")["audio_max_duration"] == 30


@pytest.mark.parametrize("att,unit,ok", [(1024, 4096, True), (512, 2048, True), (512, 2112, True), (256, 2112, True),
                                         (768, 3072, True), (512, 4096, False), (512, 2176, False), (1024, 4160, False)])
def test_feed_forward_rule_of_the_decoding_step(att, unit, ok):
    """ff <= 2112 (one LDS stage of the step GEMV) or ff <= 4 * d_model (windows of <= 1024 columns); beyond both: refused."""
    cfg = laura_recipe_config("laura")
    cfg["model_conf"]["codec_lm_conf"].update(att_unit=att, head=att // 64, unit=unit)
    if ok:
        assert laura_spec_from_config(cfg).codec_lm.ff == unit
    else:
        with pytest.raises(NotImplementedError, match="unit"):
            laura_spec_from_config(cfg)


def test_music_checkpoint_plan_matches_the_real_models_state_dict_keys():
    real = {k: tuple(v) for k, v in json.load(open(os.path.join(GOLD, "state_dict_keys_lauramusic.json"))).items()}
    plan = dict(laura_plan(laura_recipe_config("lauramusic")))
    for k, shape in plan.items():
        assert k in real and real[k] == tuple(shape), k
    left = [k for k in real if k not in plan]
    assert all(k.startswith("quantizer.rq.model.") or k == "quantizer_codebook.codec_index_shift" for k in left), left
    assert real["codec_lm.encoder.encoders.11.feed_forward.w_2.weight"] == (1024, 4096)
    assert real["text_encoder.embed.0.weight"] == (1024, 768)


def test_synthetic_text_embedder_is_a_function_of_the_text():
    cfg = laura_recipe_config("lauramusic")
    f = synthetic_text_embedder(cfg, 5)
    e, n = f("slow ambient synth pads")
    assert e.shape == (1, 4, 768) and e.dtype == torch.float32 and n.tolist() == [4]
    assert torch.equal(e, synthetic_text_embedder(cfg, 5)("slow ambient synth pads")[0])
    assert not torch.equal(e, f("fast ambient synth pads")[0])


def test_music_oracle_matches_reference_golden():
    from laura_oracle import LauraOracle
    name = "laura_music_b2"
    c, cfg, spec, sd, text, _ = case_inputs(name)
    g = golden(name)
    orc = LauraOracle(cfg, sd)
    lens = c["text_lengths"]
    with torch.no_grad():
        outs = orc.encode(torch.from_numpy(text), lens)
        assert rms(outs, g["text_outs"]) < 1e-6
        codecs = []
        for b in range(len(lens)):
            toks, logp = orc.decode_codec(outs[b, : lens[b]], c["max_length"], sampling=False, return_logp=True)
            assert float((logp - torch.from_numpy(g[f"logp_{b}"])).abs().max()) < 1e-4
            assert np.array_equal(toks.numpy(), g[f"tokens_{b}"].astype(np.int64))
            if SAME_BUILD:
                assert np.array_equal(logp.numpy(), g[f"logp_{b}"])
            codecs.append(toks)
        embs = orc.cal_codec_emb([outs[b, : lens[b]] for b in range(len(lens))], codecs)
        for b in range(len(lens)):
            assert rms(embs[b], g[f"codec_emb_{b}"]) < 1e-5


# ================================================================ GPU ================================================================
_engine = {}


def music_engine(seed, max_positions=256):
    """One music engine at a time (about 1.3 GB of weights, twice: full-sequence and step layouts)."""
    from funcodec_amd.laura import LauraGenMI355X
    key = (seed, max_positions)
    if key not in _engine:
        _engine.clear()
        cfg = laura_recipe_config("lauramusic")
        m = LauraGenMI355X(laura_spec_from_config(cfg), "cuda:0", max_positions=max_positions)
        m.load_state_dict(make_laura_state_dict(cfg, seed))
        _engine[key] = m
    return _engine[key]


def _pad_tokens(toks, nq):
    n = max(t.shape[0] for t in toks)
    out = np.zeros((len(toks), max(n, 1), nq), np.int64)
    for i, t in enumerate(toks):
        out[i, : t.shape[0]] = t
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_music_engine_against_reference_golden(name):
    c, cfg, spec, sd, text, continual = case_inputs(name)
    g = golden(name)
    m = music_engine(c["weight_seed"])
    lens, B, nq = c["text_lengths"], len(c["text_lengths"]), spec.predict_nq
    outs, _ = m.encode(torch.from_numpy(text), torch.tensor(lens))
    ref_outs = torch.from_numpy(g["text_outs"])
    for b in range(B):
        r = ref_outs[b, : lens[b]]
        assert rms(outs[b, : lens[b]], r) < 1e-4 * max(1.0, float(r.pow(2).mean().sqrt())), (name, b)
    toks_ref = [g[f"tokens_{b}"].astype(np.int64) for b in range(B)]
    cl = c["continual_lengths"] or [0] * B
    codec = torch.from_numpy(_pad_tokens(toks_ref, nq))
    clen = [t.shape[0] for t in toks_ref]
    # teacher forcing, full-sequence form
    lp = m.engine.lm_logprobs(ref_outs, lens, codec, clen).cpu()
    for b in range(B):
        ref_lp = torch.from_numpy(g[f"logp_{b}"])
        p0 = lens[b] + 1 + cl[b]
        n = min(ref_lp.shape[0], lp.shape[1] - p0)
        assert float((lp[b, p0: p0 + n] - ref_lp[:n]).abs().max()) < LOGP_TOL, (name, b, "full-sequence")
    # greedy decode with the KV cache (step form): tokens identical, per-step log-probabilities within the bar
    cont = None if continual is None else torch.from_numpy(_pad_tokens(continual, nq))
    tokens, out_lens, slp = m.engine.decode_codec(ref_outs, lens, c["max_length"], sampling=False, continual=cont,
                                                  continual_lengths=c["continual_lengths"], return_logp=True)
    tokens, slp = tokens.cpu().numpy(), slp.cpu()
    for b in range(B):
        ref_lp = torch.from_numpy(g[f"logp_{b}"])
        assert np.array_equal(tokens[b, : out_lens[b]], toks_ref[b]), (name, b, "greedy tokens")
        assert float((slp[b, : ref_lp.shape[0]] - ref_lp).abs().max()) < LOGP_TOL, (name, b, "step form")
    # teacher forcing through the step form
    forced = np.zeros((B, c["max_length"], nq), np.int64)
    for b in range(B):
        t = toks_ref[b][cl[b]:]
        forced[b, : t.shape[0]] = t
    _, _, flp = m.engine.decode_codec(ref_outs, lens, c["max_length"], sampling=False, continual=cont,
                                      continual_lengths=c["continual_lengths"], forced=torch.from_numpy(forced), return_logp=True)
    for b in range(B):
        ref_lp = torch.from_numpy(g[f"logp_{b}"])
        assert float((flp.cpu()[b, : ref_lp.shape[0]] - ref_lp).abs().max()) < LOGP_TOL, (name, b, "forced step form")
    emb = m.engine.codec_emb(ref_outs, lens, codec, clen).cpu()
    for b in range(B):
        r = torch.from_numpy(g[f"codec_emb_{b}"])
        assert rms(emb[b, : clen[b]], r) < 1e-4 * max(1.0, float(r.pow(2).mean().sqrt())), (name, b)


LM_LINEARS = ["codec_lm.encoder.encoders.0.self_attn.linear_out", "codec_lm.encoder.encoders.0.feed_forward.w_1",
              "codec_lm.encoder.encoders.0.feed_forward.w_2", "codec_lm.encoder.encoders.11.feed_forward.w_2", "codec_lm.decoder",
              "codec_lm.encoder.encoders.5.self_attn.linear_qkv"]


def _weights(sd, n):
    if n.endswith("linear_qkv"):
        p = n[: -len(".linear_qkv")]
        return (torch.cat([torch.from_numpy(sd[f"{p}.linear_{k}.weight"]) for k in "qkv"]),
                torch.cat([torch.from_numpy(sd[f"{p}.linear_{k}.bias"]) for k in "qkv"]))
    return torch.from_numpy(sd[n + ".weight"]), torch.from_numpy(sd[n + ".bias"])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 7, 16])
def test_music_step_form_linears_against_torch(B):
    """Every kind of codec_lm Linear of the music checkpoint through the decoding step's GEMV, w_2 (K = 4096) included, against
    torch.nn.functional.linear; and the LDS staging forms against each other where both apply (K = 4096 at B <= 7 fits one stage)."""
    cfg = laura_recipe_config("lauramusic")
    sd = make_laura_state_dict(cfg, 10)
    m = music_engine(10)
    rng = np.random.Generator(np.random.PCG64(B))
    for n in LM_LINEARS:
        W, b = _weights(sd, n)
        x = torch.from_numpy(rng.standard_normal((1, B, W.shape[1])).astype(np.float32))
        ref = torch.nn.functional.linear(x, W, b)
        scale = max(1.0, float(ref.abs().max()))
        got = m.engine.linear(n, x, step_form=True).cpu()
        assert float((got - ref).abs().max()) < 2e-5 * scale, (n, B)
        win = m.engine.linear(n, x, step_form=True, gemv_stage="windowed").cpu()
        assert float((win - ref).abs().max()) < 2e-5 * scale, (n, B, "windowed")
        if W.shape[1] <= 1024 or B <= 7:
            one = m.engine.linear(n, x, step_form=True, gemv_stage="single").cpu()
            assert float((one - ref).abs().max()) < 2e-5 * scale, (n, B, "single stage")
            assert float((one - win).abs().max()) < 2e-6 * scale, (n, B, "single stage vs windows")
        again = m.engine.linear(n, x, step_form=True).cpu()
        assert torch.equal(again, got), (n, B, "run to run")


def _forced_inputs(spec, cfg, B, steps, seed):
    lens = [9 + (7 * i) % 17 for i in range(B)]
    text = synthetic_text(cfg, B, lens, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    forced = torch.from_numpy(rng.integers(0, spec.codebook_size, size=(B, steps, spec.predict_nq)).astype(np.int64))
    return lens, text, forced


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 8])
def test_music_persistent_step_equals_the_kernel_chain(B):
    """d = 1024: the persistent step fits 160 KiB of LDS for B <= 2 only (w_2 in 4 slices of 1024); there it must agree with the chain
    (teacher-forced log-probabilities within 2e-5, greedy identical, bit-identical run to run).  B = 8 runs on the chain whatever the
    switch says."""
    cfg = laura_recipe_config("lauramusic")
    spec = laura_spec_from_config(cfg)
    m = music_engine(10)
    steps = 24
    lens, text, forced = _forced_inputs(spec, cfg, B, steps, 50 + B)
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(text), torch.tensor(lens))
        assert m.engine.set_persistent_step(True), "the persistent step must be usable for the music model (B <= 2)"
        _, _, sp = m.engine.decode_codec(outs, lens, steps, sampling=False, forced=forced, return_logp=True)
        _, _, sp2 = m.engine.decode_codec(outs, lens, steps, sampling=False, forced=forced, return_logp=True)
        gp = m.engine.decode_codec(outs, lens, steps, sampling=False)
        assert not m.engine.set_persistent_step(False)
        _, _, sc = m.engine.decode_codec(outs, lens, steps, sampling=False, forced=forced, return_logp=True)
        gc = m.engine.decode_codec(outs, lens, steps, sampling=False)
        m.engine.set_persistent_step(True)
    assert m.engine.persistent_step_fallbacks == 0
    assert torch.equal(sp, sp2)
    if B > 2:
        assert torch.equal(sp, sc)                # the same kernels ran
    err = float((sp - sc).abs().max())
    assert err < 2e-5, err
    assert gp[1] == gc[1] and torch.equal(gp[0], gc[0])


@pytest.mark.gpu
def test_music_chain_decode_at_16_is_bit_identical_run_to_run():
    cfg = laura_recipe_config("lauramusic")
    spec = laura_spec_from_config(cfg)
    m = music_engine(10)
    lens, text, _ = _forced_inputs(spec, cfg, 16, 1, 70)
    with torch.no_grad():
        outs, _ = m.encode(torch.from_numpy(text), torch.tensor(lens))
        a = m.engine.decode_codec(outs, lens, 16, sampling=False, return_logp=True)
        b = m.engine.decode_codec(outs, lens, 16, sampling=False, return_logp=True)
    assert a[1] == b[1] and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    # batch independence: utterance 5 alone (persistent form at B = 1) against its row of the chain's B = 16 batch
    with torch.no_grad():
        t1, o1, l1 = m.engine.decode_codec(outs[5:6, : lens[5]], [lens[5]], 16, sampling=False, return_logp=True)
    assert o1[0] == a[1][5] and torch.equal(t1[0, : o1[0]], a[0][5, : a[1][5]])
    assert float((l1[0] - a[2][5]).abs().max()) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MAN["e2e"]))
def test_music_text2audio_dropin_against_the_reference_pipeline(name, tmp_path):
    """Our Text2Audio with the stand-in text embedder (a callable text_emb_model) and the stand-in FreqCodec ds640 codec against the
    REAL Text2Audio.__call__ (continual mode, greedy) with the same embedder patched in."""
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    from funcodec_amd.config import recipe_config
    from funcodec_amd.synth import make_freq_state_dict, write_checkpoint
    _engine.clear()
    c = MAN["e2e"][name]
    g = golden(name)
    lcfg = laura_recipe_config(c["laura_config"])
    spec = laura_spec_from_config(lcfg)
    lsd = make_laura_state_dict(lcfg, c["laura_seed"])
    ccfg = recipe_config(c["codec_config"])
    csd = make_freq_state_dict(ccfg, c["codec_seed"])
    lsd["quantizer_codebook.embed"] = csd["quantizer.rq.model.embed"][: spec.num_quantizers].copy()
    lc, lp = write_checkpoint(str(tmp_path / "laura"), lcfg, lsd)
    del lsd
    cc, cp = write_checkpoint(str(tmp_path / "codec"), ccfg, csd)
    t2a = Text2Audio(config_file=lc, model_file=lp, device="cuda", text_emb_model=synthetic_text_embedder(lcfg, c["embedder_seed"]),
                     beam_size=1, sampling=False, continual=True, codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False,
                     exclude_prompt=True, max_length=c["max_length"], max_positions=256)
    prompt_audio = synthetic_audio(1, c["prompt_samples"], c["prompt_audio_seed"], "tones")
    ret, decoded = t2a(c["text"], c["prompt_text"], prompt_audio)
    ref_codec = g["decoded_codec"].astype(np.int64)
    got = decoded[0].cpu().numpy()
    assert got.shape == ref_codec.shape, (got.shape, ref_codec.shape)
    assert np.array_equal(got, ref_codec), "decoded codes differ"
    for key in ("gen", "gen_only_lm"):
        ref = torch.from_numpy(g[key])
        assert tuple(ret[key].shape) == tuple(ref.shape), (key, ret[key].shape, ref.shape)
        assert rms(ret[key], ref) < 1e-4, (key, rms(ret[key], ref), float(ref.pow(2).mean().sqrt()))
