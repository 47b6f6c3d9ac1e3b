"""`-m gpu` tests of the per-row bit rate (fc_engine_set_row_nq; ``bit_width`` / ``n_q`` per row in batches, streams and slot sessions).

A residual quantiser is a prefix code, so the yardstick is the product's own one-count call: row b of a call with a table equals, bit
for bit, what the call with n_q = that row's count gives the row alone.  One test pins the whole against the real reference through a
committed golden fixture.  Every equality is torch.equal: nothing in the arithmetic of a kept stage changes."""
import copy
import functools

import numpy as np
import pytest
import torch

from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.engine import EngineError
from funcodec_amd.synth import make_state_dict
from helpers import audio, engine_for, golden, manifest

pytestmark = pytest.mark.gpu
MAN = manifest()
NAN = float("nan")


# ---- 1. per op, every instantiation ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rvq_engine(dim, q0):
    """the tiny net with 32 stages of 64 codes in `dim` dims behind CostumeQuantizer's projection (the quantiser alone is exercised)"""
    from funcodec_amd.model import EncodecMI355X
    cfg = copy.deepcopy(recipe_config("tiny"))
    cfg["quantizer_conf"]["num_quantizers"] = 32
    if dim != 16:
        cfg["quantizer_conf"]["codec_dim"] = dim
    if q0:
        cfg["quantizer_conf"]["q0_ds_ratio"] = 2
    arch = arch_from_config(cfg)
    assert arch.codebook_dim == dim and arch.num_quantizers == 32
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 7).items()})
    return m


def _two_row_set_frames(B):
    """frames per utterance so that B of them are just past the row count above which launch_rvq_encode takes the two-row-set form
    (more than 16 rows per CU), odd so that the 32-row workgroups straddle utterances"""
    n = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    return (n // B + 2) | 1


def _check_rvq_rows(eng, x, B, counts, cap):
    """x [B * Tf, D]: the call with a table against one call per utterance at its own count"""
    Tf = x.shape[0] // B
    codes, quant = eng.rvq_encode(x, cap, n_q_rows=counts)
    assert codes.shape == (cap, B * Tf) and quant.shape == x.shape
    for b, k in enumerate(counts):
        rows = slice(b * Tf, (b + 1) * Tf)
        c1, q1 = eng.rvq_encode(x[rows], k)
        assert torch.equal(codes[:k, rows], c1), (b, k)
        assert torch.equal(quant[rows], q1), (b, k)
        assert int(codes[k:, rows].abs().max()) == 0 if k < cap else True, (b, k)
    return codes, quant


@pytest.mark.parametrize("dim,q0,big", [(16, False, False), (16, False, True), (32, False, False), (64, False, True), (128, False, False),
                                        (128, False, True), (256, False, False), (512, False, False), (16, True, False), (128, True, False),
                                        (512, True, False)])
def test_rvq_rows_equal_one_call_per_utterance_at_its_own_count(dim, q0, big):
    """B = 5 utterances of 7 frames: a 16-row workgroup straddles three of them.  `big`: enough rows for the two-row-set form."""
    eng = _rvq_engine(dim, q0).engine
    B, counts = 5, [1, 32, 2, 31, 8]
    Tf = _two_row_set_frames(B) if big else 7
    g = torch.Generator().manual_seed(1000 + dim + Tf)
    x = (torch.randn(B * Tf, dim, generator=g) * 1.5).to(eng.device)
    _check_rvq_rows(eng, x, B, counts, 32)
    if not big:      # a cap below the stage count, and counts that end every workgroup early
        _check_rvq_rows(eng, x, B, [3, 1, 2, 1, 3], 5)
        # isolation: NaN in every other utterance leaves the rest as they were
        clean_c, clean_q = eng.rvq_encode(x, 32, n_q_rows=counts)
        bad = x.clone()
        for b in (0, 2, 4):
            bad[b * Tf:(b + 1) * Tf] = NAN
        c, q = eng.rvq_encode(bad, 32, n_q_rows=counts)
        for b in (1, 3):
            rows = slice(b * Tf, (b + 1) * Tf)
            assert torch.equal(c[:, rows], clean_c[:, rows]) and torch.equal(q[rows], clean_q[rows]), b
        for b in (0, 2, 4):      # the codes of an all-NaN row stay in range, and 0 behind its count
            rows = slice(b * Tf, (b + 1) * Tf)
            assert int(c[:, rows].min()) >= 0 and int(c[:, rows].max()) < 64 and int(c[counts[b]:, rows].abs().max()) == 0


def test_engine_refuses_a_call_that_does_not_fit_the_table():
    """the C side's own rules: refused before the first launch, and the table stays as it was"""
    import ctypes as C
    eng = _rvq_engine(16, False).engine
    x = torch.randn(10, 16).to(eng.device)
    want = eng.rvq_encode(x, 6, n_q_rows=[2, 6])
    lib, h = eng.lib, eng._h

    def set_rows(rows):
        return lib.fc_engine_set_row_nq(h, None if rows is None else (C.c_int32 * len(rows))(*rows), 0 if rows is None else len(rows), eng._stream())
    try:
        assert set_rows([0, 1]) != 0 and b"[1, num_quantizers" in lib.fc_last_error()
        assert set_rows([1, 33]) != 0
        assert set_rows([2, 6]) == 0
        with pytest.raises(EngineError, match="n_q is the cap"):
            eng.rvq_encode(x, 5)
        with pytest.raises(EngineError, match="multiple"):
            eng.rvq_encode(x[:9], 6)
        wav = torch.zeros(3, 64)
        with pytest.raises(EngineError, match="set for 2 rows"):
            eng.encode(wav, 6)
        with pytest.raises(EngineError, match="set for 2 rows"):
            eng.decode_codes(torch.zeros(3, 4, 6, dtype=torch.long))
        got = eng.rvq_encode(x, 6)          # the table set by hand is still in force
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    finally:
        assert set_rows(None) == 0
    eng.check_status()


# ---- 2. pinned to the real reference -----------------------------------------------------------------------------------------------
def test_golden_batch_with_a_count_per_row():
    """tiny_b3_t1003 (the reference's own indices, 6 stages, 3 utterances; bit-exact at full n_q, which is asserted first): with a
    count per row the result is golden[:k_b, b]."""
    name = "tiny_b3_t1003"
    c = MAN["cases"][name]
    m = engine_for(c["config"], c["weight_seed"], c["codebook_decay"])
    wav = audio(c["batch"], c["samples"], c["audio_seed"], c["audio_kind"])
    ref = torch.from_numpy(golden(name)["indices"].astype(np.int64)).to(m.device)
    full = m.engine.encode(wav, c["n_q"])["codes"]
    assert torch.equal(full, ref), "the fixture must be bit-exact at full n_q for this test to say anything"
    counts = [2, 6, 1]
    got = m.engine.encode(wav, 6, n_q_rows=counts)["codes"]
    for b, k in enumerate(counts):
        assert torch.equal(got[:k, b], ref[:k, b]), b
        assert int(got[k:, b].abs().max()) == 0 if k < 6 else True, b
    m.engine.check_status()


# ---- 3. batch against one-utterance calls --------------------------------------------------------------------------------------------
BW = 12000.0          # one stage of the tiny quantisers: log2(64) bits x 16000 / 8 frames per second


def _counts(B):
    return [(1, 6, 2, 5, 3, 4)[b % 6] for b in range(B)]


@pytest.mark.parametrize("with_lengths", [False, True])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("cfg_name", ["tiny", "tinywn"])
def test_inference_rows_equal_the_one_utterance_call_with_the_rows_bit_width(cfg_name, B, with_lengths):
    m = engine_for(cfg_name, 5)
    hop = m.engine.hop_length
    T = 23 * hop + 3                        # 24 frames: the rows of a 16-row workgroup belong to two utterances
    wav = audio(B, T, 700 + B, "tones")
    counts = _counts(B)
    lens = [T - ((5 * b) % (11 * hop)) for b in range(B)] if with_lengths else [T] * B
    kw = dict(speech_lengths=torch.tensor(lens)) if with_lengths else {}
    r = m.inference(wav, bit_width=[k * BW for k in counts], **kw)
    cap = max(counts)
    codes, (quant, scale), subq, rec = r["code_indices"][0], r["code_embeddings"][0], r["sub_quants"][0], r["recon_speech"]
    assert codes.shape == (cap, B, m.engine.frames(T)) and subq.shape[:2] == (cap, B)
    for b, k in enumerate(counts):
        n = lens[b]
        # the B = 1 call of the same kind: the length-aware call runs other conv forms than the plain one (same codes, other last bits)
        one = m.inference(wav[b:b + 1, :n], bit_width=k * BW, **(dict(speech_lengths=[n]) if with_lengths else {}))
        f = m.engine.frames(n)
        assert one["code_indices"][0].shape == (k, 1, f)
        assert torch.equal(codes[:k, b, :f], one["code_indices"][0][:, 0]), (b, k)
        assert torch.equal(quant[b, :f], one["code_embeddings"][0][0][0]), (b, k)
        assert torch.equal(scale[b], one["code_embeddings"][0][1][0]), (b, k)
        assert torch.equal(subq[:k, b, :, :f], one["sub_quants"][0][:, 0]), (b, k)
        assert torch.equal(rec[b, :, :n], one["recon_speech"][0]), (b, k)
        assert int(codes[k:, b].abs().max()) == 0 and float(subq[k:, b].abs().max()) == 0.0 if k < cap else True, (b, k)
        # behind a row's length everything is zero, as in every length-aware call
        assert int(codes[:, b, f:].abs().sum()) == 0 and float(quant[b, f:].abs().sum()) == 0.0 and float(rec[b, :, n:].abs().sum()) == 0.0
    # inference_encoding takes the same keyword
    e = m.inference_encoding(wav, bit_width=torch.tensor([k * BW for k in counts]), **kw)
    assert torch.equal(e["code_indices"][0], codes) and torch.equal(e["code_embeddings"][0][0], quant)
    m.engine.check_status()


@pytest.mark.parametrize("cfg_name", ["tinycd", "tinyq0", "tinyst", "tinyfreq"])
def test_projection_q0_stereo_and_freq_codec_rows(cfg_name):
    """codec_dim projection, q0_ds_ratio > 1, stereo and the STFT-domain codec go through the same quantiser and decode head: row b
    of the call with a table is row b of the same batch at n_q = the row's count"""
    from helpers import freq_engine_for
    m = freq_engine_for(cfg_name, 3) if cfg_name == "tinyfreq" else engine_for(cfg_name, 5)
    ch = m.engine.channels
    B, T = 3, 1777 if cfg_name == "tinyfreq" else 331
    wav = audio(B, T, 750, "tones", ch)
    cap = m.arch.num_quantizers
    counts = [1, cap, 2]
    r = m.engine.encode_decode(wav, cap, n_q_rows=counts)
    for b, k in enumerate(counts):
        same = m.engine.encode_decode(wav, k)
        assert torch.equal(r["codes"][:k, b], same["codes"][:, b]), (b, k)
        assert torch.equal(r["quantized"][b], same["quantized"][b]) and torch.equal(r["recon"][b], same["recon"][b]), (b, k)
        assert torch.equal(r["sub_quants"][:k, b], same["sub_quants"][:, b]), (b, k)
        assert int(r["codes"][k:, b].abs().max()) == 0 and float(r["sub_quants"][k:, b].abs().max()) == 0.0 if k < cap else True
    m.engine.check_status()


# ---- 4. decode ignores what it must not read ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lengths", [False, True])
def test_decode_does_not_read_codes_behind_a_rows_count(with_lengths):
    m = engine_for("tiny", 5)
    hop = m.engine.hop_length
    B, T = 3, 23 * hop + 3
    counts = [2, 6, 1]
    enc = m.inference_encoding(audio(B, T, 703, "tones"), bit_width=[k * BW for k in counts])
    tok = enc["code_indices"][0].permute(1, 2, 0).contiguous()          # [B, Tf, 6], zeros behind a row's count
    Tf = tok.shape[1]
    lens = [Tf, Tf - 5, Tf - 9]
    kw = dict(token_lengths=torch.tensor(lens)) if with_lengths else {}
    want = m.inference_decoding(tok, bit_width=[k * BW for k in counts], **kw)
    for b, k in enumerate(counts):       # row b is what the decode of its first k stages alone gives
        f = lens[b] if with_lengths else Tf
        one = m.inference_decoding(tok[b:b + 1, :f, :k].contiguous(), **(dict(token_lengths=[f]) if with_lengths else {}))
        assert torch.equal(want["recon_speech"][b, :, :f * hop], one["recon_speech"][0]), (b, k)
        assert torch.equal(want["code_embeddings"][0][0][b, :f], one["code_embeddings"][0][0][0]), (b, k)
    for junk in (-1, m.arch.codebook_size + 5):
        bad = tok.clone()
        for b, k in enumerate(counts):
            bad[b, :, k:] = junk
        got = m.inference_decoding(bad, bit_width=[k * BW for k in counts], **kw)
        assert torch.equal(got["recon_speech"], want["recon_speech"]), junk
        assert torch.equal(got["code_embeddings"][0][0], want["code_embeddings"][0][0]), junk
        m.engine.check_status()          # nothing was reported as out of range
    # the same junk inside a row's count is still loud
    bad = tok.clone()
    bad[0, 0, 0] = m.arch.codebook_size + 5
    m.inference_decoding(bad, bit_width=[k * BW for k in counts], **kw)
    with pytest.raises(EngineError, match="outside"):
        m.engine.check_status()


# ---- 5. isolation --------------------------------------------------------------------------------------------------------------------
def test_nan_in_every_other_row_leaves_a_rows_results_unchanged():
    m = engine_for("tiny", 5)
    hop = m.engine.hop_length
    B, T = 5, 23 * hop + 3
    counts = [6, 2, 1, 5, 3]
    wav = audio(B, T, 705, "tones")
    clean = m.inference(wav, bit_width=[k * BW for k in counts])
    bad = wav.clone()
    bad[0::2] = NAN
    got = m.inference(bad, bit_width=[k * BW for k in counts])
    for b in (1, 3):
        assert torch.equal(got["code_indices"][0][:, b], clean["code_indices"][0][:, b]), b
        assert torch.equal(got["code_embeddings"][0][0][b], clean["code_embeddings"][0][0][b]), b
        assert torch.equal(got["sub_quants"][0][:, b], clean["sub_quants"][0][:, b]), b
        assert torch.equal(got["recon_speech"][b], clean["recon_speech"][b]), b
    m.engine.check_status()


# ---- 6. sessions ---------------------------------------------------------------------------------------------------------------------
class _Ref:
    """one utterance of a session test and what the offline calls give for it"""

    def __init__(self, m, seed, T):
        self.m, self.T = m, T
        self.wav = audio(1, T, seed, "tones")
        full = m.engine.encode(self.wav, m.arch.num_quantizers)
        self.codes, self.scale = full["codes"][:, 0], full["scale"].reshape(())
        self._quant = {}

    def quant(self, k):
        """quantized [Tf, D] of the offline call at n_q = k"""
        if k not in self._quant:
            self._quant[k] = self.m.engine.encode(self.wav, k)["quantized"][0]
        return self._quant[k]

    def emb(self, a, b, k):
        """the embeddings the offline decode looks up for frames a .. b at n_q = k"""
        tok = self.codes[:k, a:b].t().contiguous()[None]
        return self.m.engine.decode_codes(tok)[1][0]


def _check_push(ref, k, a, codes, quant, cap):
    """codes [cap, n], quantized [n, D] of one push of an utterance: frames a .. a + n with k stages"""
    n = codes.shape[-1]
    assert torch.equal(codes[:k], ref.codes[:k, a:a + n]), (a, k)
    assert int(codes[k:].abs().max()) == 0 if k < cap else True, (a, k)
    assert torch.equal(quant, ref.quant(k)[a:a + n]), (a, k)


def test_stream_rows_change_their_count_at_every_push():
    m = engine_for("tinyss", 5)
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    frames = [9, 5, 3, 7, 4]                                       # the last push is final and 3 samples longer
    T = sum(frames) * hop + 3
    refs = [_Ref(m, 720 + b, T) for b in range(3)]
    wav = torch.cat([r.wav for r in refs], 0)
    scale = torch.stack([r.scale for r in refs])
    plan = [[6, 3, 2], [6, 1, 2], [6, 6, 2], [6, 2, 2], [6, 5, 2]]  # row 0 all stages, row 1 another count at every push, row 2 two
    st = m.open_stream(3, n_q=plan[0], scale=scale)
    twin = m.open_stream(3, scale=scale)                           # decodes the offline embeddings of the same frame ranges
    assert st.n_q == cap and st.min_first_samples <= frames[0] * hop and st.min_first_frames <= frames[0]
    pos = 0
    for p, (nf, rows) in enumerate(zip(frames, plan)):
        last = p == len(frames) - 1
        n = nf * hop + (3 if last else 0)
        if p:
            with pytest.raises(EngineError):                       # a refused set_n_q changes nothing
                st.set_n_q([1, cap + 1, 1])
            st.set_n_q(rows)
        codes, quant = st.encode(wav[:, pos * hop:pos * hop + n], final=last)
        f = codes.shape[-1]
        assert f == (nf + 1 if last else nf)
        for b, k in enumerate(rows):
            _check_push(refs[b], k, pos, codes[:, b], quant[b], cap)
        tok = codes.permute(1, 2, 0).contiguous()
        for b, k in enumerate(rows):                               # what lies behind a row's count is not read
            tok[b, :, k:] = -1
        rec = st.decode(tok, final=last)
        emb = torch.stack([refs[b].emb(pos, pos + f, k) for b, k in enumerate(rows)])
        assert torch.equal(emb, quant)
        assert torch.equal(rec, twin.decode_emb(emb, final=last)), p
        pos += f
    m.engine.check_status()


def test_slots_change_their_count_in_the_middle_of_an_utterance():
    """S = 4: slot 0 runs all stages throughout, slot 1 starts a push later and changes its count at every push, slot 2 ends an
    utterance with 2 stages and starts the next with 4, slot 3 idles; idle rows and what lies behind a row's count hold NaN."""
    m = engine_for("tinyss", 5)
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    st, twin = m.open_slots(4), m.open_slots(4)
    st.pad_value = twin.pad_value = NAN
    first = max(st.min_first_samples // hop, st.min_first_frames, 6)
    # per slot: (round of the first push, utterance, [(frames, stages)] per push; the last push is final and 3 samples longer)
    A, B_, C_, D_ = (_Ref(m, 730 + i, T) for i, T in enumerate([(first + 17) * hop + 3, (first + 14) * hop + 3, (first + 4) * hop + 3,
                                                                 (first + 3) * hop + 3]))
    lines = {0: [(0, A, [(first, 6), (4, 6), (5, 6), (4, 6), (4, 6)])],
             1: [(1, B_, [(first, 3), (2, 1), (6, 6), (3, 2), (3, 5)])],
             2: [(0, C_, [(first, 2), (4, 2)]), (3, D_, [(first, 4), (3, 4)])]}
    pos = {}
    for r in range(6):
        push, meta = {}, {}
        for slot, utts in lines.items():
            for r0, ref, steps in utts:
                i = r - r0
                if not 0 <= i < len(steps):
                    continue
                nf, k = steps[i]
                last = i == len(steps) - 1
                if i == 0:
                    pos[slot] = 0
                    if slot == 2:
                        st.start(slot, ref.scale, n_q=k)           # the count comes with start ...
                    else:
                        st.start(slot, ref.scale)
                        st.set_n_q(slot, k)
                    twin.start(slot, ref.scale)
                else:
                    st.set_n_q(slot, k)                            # ... or between two pushes of a running utterance
                a = pos[slot] * hop
                push[slot] = (ref.wav[0, a:a + nf * hop + (3 if last else 0)], last)
                meta[slot] = (ref, k, last)
        with pytest.raises(EngineError):                           # refused: nothing changes
            st.set_n_q(1, cap + 1)
        out = st.encode(push)
        assert set(out) == set(push)
        dec, dec_twin = {}, {}
        for slot, (codes, quant) in out.items():
            ref, k, last = meta[slot]
            f = codes.shape[-1]
            _check_push(ref, k, pos[slot], codes, quant, cap)
            tok = codes.t().contiguous()
            tok[:, k:] = m.arch.codebook_size + 5                  # not read, never reported
            emb = ref.emb(pos[slot], pos[slot] + f, k)
            assert torch.equal(emb, quant)
            dec[slot], dec_twin[slot] = (tok, last), (emb, last)
            pos[slot] += f
        got, want = st.decode(dec), twin.decode_emb(dec_twin)
        for slot in dec:
            assert torch.equal(got[slot], want[slot]), (r, slot)
    m.engine.check_status()


# ---- 7. idle path --------------------------------------------------------------------------------------------------------------------
def test_a_plain_call_after_a_call_with_a_table_is_untouched():
    m = engine_for("tiny", 5)
    hop = m.engine.hop_length
    wav = audio(3, 23 * hop + 3, 707, "tones")
    before = m.inference(wav)
    tok = before["code_indices"][0].permute(1, 2, 0).contiguous()
    dec_before = m.inference_decoding(tok)
    m.inference(wav, bit_width=[BW, 6 * BW, 2 * BW])
    m.inference_decoding(tok, bit_width=[BW, 6 * BW, 2 * BW])
    with pytest.raises(EngineError):                                # a refused call leaves no table behind either
        m.engine.encode(wav[:2], 6, n_q_rows=[1, 2, 3])
    after, dec_after = m.inference(wav), m.inference_decoding(tok)
    assert torch.equal(after["code_indices"][0], before["code_indices"][0])
    assert torch.equal(after["code_embeddings"][0][0], before["code_embeddings"][0][0])
    assert torch.equal(after["sub_quants"][0], before["sub_quants"][0])
    assert torch.equal(after["recon_speech"], before["recon_speech"])
    assert torch.equal(dec_after["recon_speech"], dec_before["recon_speech"])
    # another batch width is fine again: no table is left behind
    m.inference(wav[:2])
    m.engine.check_status()
