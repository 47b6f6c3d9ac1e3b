"""``Text2Audio.generate_batch / generate_many(length_aware=True)`` without a device: the grouping rule (laura.tail_groups), the packing
(laura.pack_windows), which codec calls the two forms make (a stand-in codec and a stand-in model record them), and the refusal.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from funcodec_amd.bin.text2audio_inference import Text2Audio
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.engine import EngineError

HOP, NQ, D = 320, 2, 4


# 1 ---------------------------------------------------------------------------------------------------------------------------
def lengths_of(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [int(v) for v in rng.integers(1, 9, size=n)]          # 8 values: ties at every n > 8


@pytest.mark.parametrize("n", [0, 1, 16, 17, 33])
@pytest.mark.parametrize("rows", [16, 5])
def test_tail_groups(n, rows):
    from funcodec_amd.laura import tail_groups
    lengths = lengths_of(n, 40 + n)
    groups = tail_groups(lengths, rows)
    flat = [i for g in groups for i in g]
    assert sorted(flat) == list(range(n))                                          # every index exactly once
    assert all(1 <= len(g) <= rows for g in groups)
    assert [len(g) for g in groups] == [rows] * (n // rows) + ([n % rows] if n % rows else [])
    keys = [(lengths[i], i) for i in flat]
    assert keys == sorted(keys)                                                     # by length, ties to the lower index
    if rows == 16:
        assert len(groups) == {0: 0, 1: 1, 16: 1, 17: 2, 33: 3}[n]


def test_tail_groups_by_hand():
    from funcodec_amd.laura import tail_groups
    assert tail_groups([]) == []
    assert tail_groups([7]) == [[0]]
    assert tail_groups([5, 3, 5, 3, 9], rows=2) == [[1, 3], [0, 2], [4]]
    assert tail_groups([4, 4, 4], rows=16) == [[0, 1, 2]]
    assert tail_groups(list(range(17, 0, -1))) == [list(range(16, 0, -1)), [0]]
    with pytest.raises(ValueError):
        tail_groups([1], rows=0)


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [([0, 0, 0], [5, 2, 7]), ([4, 1, 6], [5, 2, 7]), ([0, 1, 0, 6], [5, 2, 1, 7]), ([3], [3])])
def test_pack_windows(lo, hi):
    from funcodec_amd.laura import pack_windows
    B = len(lo)
    rng = np.random.Generator(np.random.PCG64(3))
    tokens = torch.from_numpy(rng.integers(1, 1024, size=(B, 7, NQ)).astype(np.int64))          # no zero inside: zeros are padding
    emb = torch.from_numpy(rng.standard_normal((B, 7, D)).astype(np.float32)) + 10.0
    for x in (tokens, emb):
        before = x.clone()
        p = pack_windows(x, lo, hi)
        assert p.dtype == x.dtype and tuple(p.shape) == (B, max(h - l for l, h in zip(lo, hi))) + tuple(x.shape[2:])
        for j in range(B):
            k = hi[j] - lo[j]
            assert torch.equal(p[j, :k], x[j, lo[j]: hi[j]]), j
            assert not p[j, k:].any(), j
        assert torch.equal(x, before)


def test_pack_windows_refuses_a_window_outside_the_row():
    from funcodec_amd.laura import pack_windows
    x = torch.zeros((2, 4, NQ), dtype=torch.int64)
    for lo, hi in (([0, 3], [4, 2]), ([0, 0], [4, 5]), ([-1, 0], [4, 4]), ([0], [4])):
        with pytest.raises(ValueError):
            pack_windows(x, lo, hi)


# 3 ---------------------------------------------------------------------------------------------------------------------------
class Codec:
    """Stand-in Speech2Token: records its calls; every output sample is a function of its own row's input at that place alone."""

    def __init__(self, recipe="ds320"):
        self.calls = []
        engine = SimpleNamespace(frames=lambda n: -(-int(n) // HOP), decoded_samples=lambda k: int(k) * HOP, hop_length=HOP)
        self.model = SimpleNamespace(arch=arch_from_config(recipe_config(recipe)), engine=engine)

    def __call__(self, speech, bit_width=None, run_mod="inference", speech_lengths=None):
        speech = torch.as_tensor(speech)
        lens = None if speech_lengths is None else [int(v) for v in torch.as_tensor(speech_lengths).reshape(-1)]
        self.calls.append(dict(run_mod=run_mod, shape=tuple(speech.shape), lengths=lens))
        B = speech.shape[0]
        if run_mod == "encode":                       # code of frame t, stage q: the frame's first sample + q
            T = speech.shape[-1]
            Tf = -(-T // HOP)
            x = torch.zeros((B, Tf * HOP))
            x[:, :T] = speech.reshape(B, T)
            codes = torch.stack([x[:, ::HOP].long() + q for q in range(4)])          # [n_q, B, Tf]
            if lens is not None:
                for b, n in enumerate(lens):
                    codes[:, b, -(-n // HOP):] = 0
            return [codes], None, None, None
        v = speech[..., 0].float() + (0.25 if run_mod == "decode_emb" else 0.0)        # [B, Tf]
        wav = v.repeat_interleave(HOP, dim=1)[:, None, :]
        if lens is not None:
            for b, k in enumerate(lens):
                wav[b, :, k * HOP:] = 0
        return None, None, wav, None


class Model:
    """Stand-in LauraGenMI355X: the prompt's tokens, then out_len - prompt more; the fine predictor's rows from the row's tokens."""
    predict_nq, device, vocab_size = NQ, "cpu", 1

    def __init__(self, gen_lens):
        self.gen_lens, self.emb_calls = gen_lens, []

    def decode_codec_batch(self, text_outs, lens, max_length, sampling, cont, cont_lens, seed):
        n = len(lens)
        cl = cont_lens or [0] * n
        out_lens = [cl[i] + self.gen_lens[i] for i in range(n)]
        tokens = torch.zeros((n, max(out_lens), NQ), dtype=torch.int64)
        for i in range(n):
            if cl[i]:
                tokens[i, : cl[i]] = cont[i, : cl[i]]
            tokens[i, cl[i]: out_lens[i]] = 100 * (i + 1) + torch.arange(self.gen_lens[i])[:, None]
        return tokens, out_lens

    def cal_codec_emb_batch(self, text_outs, lens, tokens, out_lens):
        self.emb_calls.append(list(out_lens))
        return (tokens[..., :1].float() + 0.5).expand(-1, -1, D).contiguous()


def stand_in(gen_lens, recipe="ds320", exclude_prompt=True):
    t2a = object.__new__(Text2Audio)
    t2a.model, t2a.codec_model = Model(gen_lens), Codec(recipe)
    t2a.continual, t2a.exclude_prompt, t2a.sampling, t2a.max_length = True, exclude_prompt, True, 16
    t2a._encode_texts = lambda texts: (torch.zeros((len(texts), 3, D)), [3] * len(texts))
    return t2a


PROMPT_SAMPLES = [321, 2240, 4000, 960, 320]
GEN_LENS = [5, 1, 9, 3, 9]


def prompts():
    return [np.full((1, n), float(10 * (i + 1)), dtype=np.float32) for i, n in enumerate(PROMPT_SAMPLES)]


def same_results(a, b):
    (ra, ca), (rb, cb) = a, b
    assert len(ra) == len(rb) == len(ca) == len(cb)
    for i in range(len(ra)):
        assert torch.equal(ca[i], cb[i]), i
        for key in ("gen", "gen_only_lm"):
            assert ra[i][key].shape == rb[i][key].shape and ra[i][key].dtype == rb[i][key].dtype, (i, key)
            assert torch.equal(ra[i][key], rb[i][key]), (i, key)


@pytest.mark.parametrize("exclude_prompt", [True, False])
def test_codec_calls_of_the_two_forms(exclude_prompt):
    n = len(GEN_LENS)
    texts, ptexts = [f"t{i}" for i in range(n)], [f"p{i}" for i in range(n)]
    frames = [-(-s // HOP) for s in PROMPT_SAMPLES]

    old = stand_in(GEN_LENS, exclude_prompt=exclude_prompt)
    ref = old.generate_batch(texts, ptexts, prompts(), seed=1)
    calls = old.codec_model.calls
    assert [c["run_mod"] for c in calls] == ["encode"] * n + ["decode", "decode_emb"] * n          # one per prompt, two per utterance
    assert all(c["lengths"] is None for c in calls)
    assert [c["shape"][0] for c in calls] == [1] * (3 * n)

    new = stand_in(GEN_LENS, exclude_prompt=exclude_prompt)
    got = new.generate_batch(texts, ptexts, prompts(), seed=1, length_aware=True)
    calls = new.codec_model.calls
    k = GEN_LENS if exclude_prompt else [f + g for f, g in zip(frames, GEN_LENS)]
    assert [c["run_mod"] for c in calls] == ["encode", "decode", "decode_emb"]                       # one per prompt group, two per group
    assert calls[0]["lengths"] == PROMPT_SAMPLES and calls[0]["shape"] == (n, max(PROMPT_SAMPLES))
    assert calls[1]["lengths"] == k and calls[1]["shape"] == (n, max(k), NQ)
    assert calls[2]["lengths"] == k and calls[2]["shape"] == (n, max(k), D)
    assert new.model.emb_calls == old.model.emb_calls                                                # the fine predictor runs as ever
    same_results(got, ref)                                                                           # request order, the same rows
    for i in range(n):
        assert got[0][i]["gen"].shape == (1, 1, k[i] * HOP) and got[1][i].shape == (1, frames[i] + GEN_LENS[i], NQ)
        assert float(got[1][i][0, 0, 0]) == 10 * (i + 1)                                             # request i's own prompt in front


def test_prompt_groups_of_sixteen():
    t2a = stand_in([])
    sizes = [320 * (1 + (7 * i) % 5) + i for i in range(17)]
    wavs = [np.full((1, s), float(i + 1), dtype=np.float32) for i, s in enumerate(sizes)]
    per = t2a._prompt_codecs(wavs, True)
    calls = t2a.codec_model.calls
    assert [(c["run_mod"], c["shape"], c["lengths"]) for c in calls] == [("encode", (16, max(sizes[:16])), sizes[:16]),
                                                                         ("encode", (1, sizes[16]), sizes[16:])]
    alone = stand_in([])._prompt_codecs(wavs)
    for i in range(17):
        assert per[i].shape == (-(-sizes[i] // HOP), NQ) and torch.equal(per[i], alone[i]), i


def test_a_row_without_frames_keeps_the_one_utterance_calls():
    """k_j = 0 (the LM ended on its first step, the prompt excluded): the row is left out of the batch and goes through the two
    calls of the default form, whatever they give (the engine refuses a decode of zero frames in both forms)."""
    gen = [4, 0, 2]
    new = stand_in(gen)
    tokens, out_lens = new.model.decode_codec_batch(None, [3] * 3, 16, True, torch.full((3, 2, NQ), 7), [2] * 3, 0)
    rets, codecs = new._synthesise(torch.zeros((3, 3, D)), [3] * 3, tokens, out_lens, [2] * 3, True)
    calls = new.codec_model.calls
    assert [(c["run_mod"], c["shape"][:2], c["lengths"]) for c in calls] == [
        ("decode", (2, 4), [4, 2]), ("decode_emb", (2, 4), [4, 2]), ("decode", (1, 0), None), ("decode_emb", (1, 0), None)]
    old = stand_in(gen)
    same_results((rets, codecs), old._synthesise(torch.zeros((3, 3, D)), [3] * 3, tokens, out_lens, [2] * 3))
    assert rets[1]["gen"].shape == (1, 1, 0)


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe,key", [("ds320tf", "seq_model: transformer"), ("freqmp", "freq_codec"), ("ds320q0", "q0_ds_ratio"),
                                        ("ds320seg", "segment_dur")])
def test_refusal_names_the_key_before_any_call(recipe, key):
    n = 2
    texts, ptexts = ["a", "b"], ["p", "q"]
    t2a = stand_in(GEN_LENS[:n], recipe)
    with pytest.raises(EngineError, match=key) as e:
        t2a.generate_batch(texts, ptexts, prompts()[:n], seed=1, length_aware=True)
    assert "length_aware=True" in str(e.value)
    with pytest.raises(EngineError, match=key):
        t2a.generate_many(texts, ptexts, prompts()[:n], seeds=[1, 2], length_aware=True)
    with pytest.raises(EngineError, match=key):
        t2a.generate_many(texts, seeds=[1, 2], length_aware=True)                      # no prompts: refused all the same
    assert t2a.codec_model.calls == [] and t2a.model.emb_calls == []
    t2a.generate_batch(texts, ptexts, prompts()[:n], seed=1)                           # the default form is untouched
    assert len(t2a.codec_model.calls) == 3 * n
