"""``Text2Audio.generate_many / generate_batch(length_aware=True)`` on the GPU: the codec calls around the decoding session as
length-aware batches (``speech_lengths``).  What is pinned, on the set-up of test_laura_slots_gpu.py::test_generate_many_keeps_two_slots_full:

* the tokens are those of the default call, bit for bit, with and without prompt recordings (321 .. 4800 samples in one encode call: the
  batched prompt codes equal the one-call-each codes);
* a request's waveforms depend on that request alone: among five, alone, and among seventeen (two groups, regrouped by length), with the
  prompt excluded or not -- torch.equal;
* what stands behind a row's tokens is never read;
* against the default call: shapes, dtypes and sample counts equal, waveforms within WAV_RMS_TOL (1e-4 RMS, the bar of a length-aware
  row against the same row alone, test_ragged_gpu.py::test_ragged_host_keywords_reach_the_engine).  Measured on MI355X: at most
  1.23e-6 over every comparison of this file, on signals of RMS 1.04;
* samples / keep="best" / retries / prefill and a wide session compose with it: tokens and choice equal, waveforms within the bar.
"""
import pytest
import torch

from helpers import rms

from test_gpu_parity import WAV_RMS_TOL
from test_laura import MAN

pytestmark = pytest.mark.gpu

PROMPT_SAMPLES = [321, 2240, 4000, 1600, 4800]          # hop 320: 2, 7, 13, 5 and 15 frames
SEEDS = [1032, 101, 102, 1059, 104]                     # requests 0 and 3 end on <eos> after 6 and 5 frames, the others run to max_length
CASE = MAN["e2e"]["laura_e2e_tinyphn_ds320"]


@pytest.fixture(scope="module")
def t2a(tmp_path_factory):
    return text2audio(tmp_path_factory.mktemp("length_aware"))


def text2audio(tmp):
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config
    from funcodec_amd.synth import make_laura_state_dict, make_state_dict, write_checkpoint
    c = CASE
    lcfg = laura_recipe_config(c["laura_config"])
    spec = laura_spec_from_config(lcfg)
    lsd = make_laura_state_dict(lcfg, c["laura_seed"])
    ccfg = recipe_config(c["codec_config"])
    csd = make_state_dict(arch_from_config(ccfg), c["codec_seed"])
    lsd["quantizer_codebook.embed"] = csd["quantizer.rq.model.embed"][: spec.num_quantizers].copy()
    lc, lp = write_checkpoint(str(tmp / "laura"), lcfg, lsd)
    cc, cp = write_checkpoint(str(tmp / "codec"), ccfg, csd)
    return Text2Audio(config_file=lc, model_file=lp, device="cuda", text_emb_model=None, beam_size=1, sampling=True, continual=True,
                      codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False, exclude_prompt=True, max_length=14,
                      max_positions=256)


def requests(n):
    """(texts, prompt texts, prompt recordings, seeds) of n requests; the first five are the same whatever n"""
    from funcodec_amd.synth import synthetic_audio
    words, pwords = CASE["text"].split(" "), CASE["prompt_text"].split(" ")
    texts = [" ".join(words[i % 3: i % 3 + 3 + (2 * i) % 7]) for i in range(n)]          # 3, 5, 7, 9, 4 words, ...
    ptexts = [" ".join(pwords[: 2 + i % 3]) for i in range(n)]
    sizes = PROMPT_SAMPLES + [320 * (1 + (5 * i) % 7) + 3 * i for i in range(5, n)]
    audios = [synthetic_audio(1, sizes[i], 600 + i, "tones") for i in range(n)]
    return texts, ptexts, audios, SEEDS + [200 + i for i in range(5, n)]


_five = {}


def five(t2a, exclude_prompt, length_aware):
    """generate_many on the five requests with their recordings, computed once per form and shared (nobody changes it)"""
    key = (exclude_prompt, length_aware)
    if key not in _five:
        texts, ptexts, audios, seeds = requests(5)
        t2a.exclude_prompt = exclude_prompt
        try:
            _five[key] = t2a.generate_many(texts, ptexts, audios, slots=2, seeds=seeds, length_aware=length_aware)
        finally:
            t2a.exclude_prompt = True
    return _five[key]


def same_waves(a, b, what):
    for key in ("gen", "gen_only_lm"):
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, (what, key, a[key].shape, b[key].shape)
        assert torch.equal(a[key], b[key]), (what, key, float((a[key] - b[key]).abs().max()))


def close_waves(a, b, what):
    """shapes, dtypes and sample counts equal, both waveforms within WAV_RMS_TOL; the larger of the two distances"""
    worst = 0.0
    for key in ("gen", "gen_only_lm"):
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].device == b[key].device, (what, key)
        d = rms(a[key], b[key])
        print(what, key, "samples", a[key].shape[-1], "rms", d, "signal rms", float(b[key].pow(2).mean().sqrt()))
        assert d < WAV_RMS_TOL, (what, key, d)
        worst = max(worst, d)
    return worst


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_batched_prompt_codes_are_the_one_call_each_codes(t2a):
    audios = requests(17)[2]
    alone, batched = t2a._prompt_codecs(audios), t2a._prompt_codecs(audios, True)
    frames = t2a.codec_model.model.engine.frames
    for i, a in enumerate(audios):
        assert batched[i].shape == alone[i].shape == (frames(a.shape[-1]), t2a.model.predict_nq), i
        differ = (batched[i] != alone[i]).any(dim=1).nonzero().reshape(-1).tolist()
        assert torch.equal(batched[i], alone[i]), (i, a.shape[-1], "frames that differ", differ)


def test_tokens_are_those_of_the_default_call(t2a):
    texts, ptexts, audios, seeds = requests(5)
    assert len({len(t.split(" ")) for t in texts}) > 2
    _, ref = five(t2a, True, False)
    _, got = five(t2a, True, True)
    prompt = [t2a.codec_model.model.engine.frames(n) for n in PROMPT_SAMPLES]
    generated = [int(c.shape[1]) - p for c, p in zip(ref, prompt)]
    print("generated frames", generated, "behind prompts of", prompt)
    assert len(set(generated)) > 1, generated          # a batch of equal rows would prove nothing
    for i in range(5):
        assert got[i].shape == ref[i].shape and torch.equal(got[i], ref[i]), i
    # without recordings: zero-shot from the text alone, nothing excluded
    _, ref = t2a.generate_many(texts, slots=2, seeds=seeds)
    _, got = t2a.generate_many(texts, slots=2, seeds=seeds, length_aware=True)
    for i in range(5):
        assert got[i].shape == ref[i].shape and torch.equal(got[i], ref[i]), i
    # generate_batch: one engine call for the five
    _, ref = t2a.generate_batch(texts, ptexts, audios, seed=77)
    rets, got = t2a.generate_batch(texts, ptexts, audios, seed=77, length_aware=True)
    for i in range(5):
        assert got[i].shape == ref[i].shape and torch.equal(got[i], ref[i]), i
        assert rets[i]["gen"].shape == (1, 1, (got[i].shape[1] - prompt[i]) * 320)


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude_prompt", [True, False])
def test_a_row_depends_on_its_own_request_only(t2a, exclude_prompt):
    rets5, codecs5 = five(t2a, exclude_prompt, True)
    t2a.exclude_prompt = exclude_prompt
    try:
        texts, ptexts, audios, seeds = requests(17)
        rets17, codecs17 = t2a.generate_many(texts, ptexts, audios, slots=2, seeds=seeds, length_aware=True)
        decoded = [int(r["gen"].shape[-1]) for r in rets17]
        print("exclude_prompt", exclude_prompt, "samples decoded by the seventeen", decoded)
        assert len(set(decoded)) > 1, decoded
        for i in range(5):
            r1, c1 = t2a.generate_many(texts[i: i + 1], ptexts[i: i + 1], audios[i: i + 1], slots=2, seeds=seeds[i: i + 1], length_aware=True)
            assert torch.equal(codecs5[i], c1[0]) and torch.equal(codecs5[i], codecs17[i]), i
            same_waves(rets5[i], r1[0], (i, "among five / alone"))
            same_waves(rets5[i], rets17[i], (i, "among five / among seventeen"))
            frames = codecs5[i].shape[1] - (t2a.codec_model.model.engine.frames(PROMPT_SAMPLES[i]) if exclude_prompt else 0)
            assert rets5[i]["gen"].shape == rets5[i]["gen_only_lm"].shape == (1, 1, frames * 320), i
    finally:
        t2a.exclude_prompt = True


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_what_stands_behind_a_row_is_never_read(t2a):
    texts, ptexts, audios, seeds = requests(5)
    _, codecs = five(t2a, True, True)
    text_outs, lens = t2a._encode_texts([" ".join([p, t]).strip() for p, t in zip(ptexts, texts)])
    out_lens = [int(c.shape[1]) for c in codecs]
    excl = [t2a.codec_model.model.engine.frames(n) for n in PROMPT_SAMPLES]
    assert t2a.model.codebook_size == 1024

    def run(fill):
        tokens = torch.full((5, max(out_lens) + 3, t2a.model.predict_nq), fill, dtype=torch.int64, device=t2a.model.device)
        for j, c in enumerate(codecs):
            tokens[j, : out_lens[j]] = c[0]
        return t2a._synthesise(text_outs, lens, tokens, out_lens, excl, length_aware=True)

    (ra, ca), (rb, cb) = run(0), run(1023)
    for j in range(5):
        assert torch.equal(ca[j], cb[j]) and torch.equal(ca[j], codecs[j]), j
        same_waves(ra[j], rb[j], (j, "0 / 1023 behind the row"))
        assert ra[j]["gen"].shape == (1, 1, (out_lens[j] - excl[j]) * 320)


# 8 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude_prompt", [True, False])
def test_against_the_default_call(t2a, exclude_prompt):
    (old, c_old), (new, c_new) = five(t2a, exclude_prompt, False), five(t2a, exclude_prompt, True)
    worst = 0.0
    for i in range(5):
        assert torch.equal(c_old[i], c_new[i]), i
        worst = max(worst, close_waves(new[i], old[i], ("exclude_prompt", exclude_prompt, "request", i)))
    print("exclude_prompt", exclude_prompt, "largest rms(length-aware, default)", worst, "bar", WAV_RMS_TOL)


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_composition_with_best_of_n_retries_and_prefill(t2a):
    texts, ptexts, audios, _ = requests(5)
    seeds = [[300 + 3 * i + k for k in range(3)] for i in range(5)]
    kw = dict(slots=4, seeds=seeds, samples=3, keep="best", retries=1, prefill=4)
    r_old, c_old, ch_old = t2a.generate_many(texts, ptexts, audios, **kw)
    r_new, c_new, ch_new = t2a.generate_many(texts, ptexts, audios, length_aware=True, **kw)
    assert ch_old == ch_new and len(r_new) == len(c_new) == 5
    for i in range(5):
        assert torch.equal(c_old[i], c_new[i]), i
        close_waves(r_new[i], r_old[i], ("best of 3", i))


def test_composition_with_a_wide_session(t2a):
    texts, ptexts, audios, seeds = requests(24)
    r_old, c_old = t2a.generate_many(texts, ptexts, audios, slots=20, seeds=seeds)
    r_new, c_new = t2a.generate_many(texts, ptexts, audios, slots=20, seeds=seeds, length_aware=True)
    assert len(r_new) == len(c_new) == 24
    for i in range(24):
        assert torch.equal(c_old[i], c_new[i]), i
        close_waves(r_new[i], r_old[i], ("slots=20", i))
