"""`-m gpu` tests of streaming a causal transformer net through the session's key / value cache (``open_stream(..., max_frames=N)``,
fc_seqstream_*, csrc/seqstream_kernels.hip).  The yardsticks are float64 (the stage) and the real reference's fixture (end to end), never
the engine's own offline call.

The thresholds of the cached attention (csrc/seq_kernels.h) and the pushes on both sides of each:
  * kSeqCachedSplitMaxQueries = 16: pushes of 15 and 16 frames take the split form, pushes of 17, 24, 32, 33, 500 the many-query form;
  * kSeqCachedTilesPerUnit = 2: a split push with pos + n <= 32 runs on one unit (the pushes up to position 32 of SCHEDULE), the
    16-frame push from 32 to 48 and the 1-frame pushes at 65 on two or more;
  * kSeqCachedMaxUnits = 16: reached past 512 keys, by the 1-frame pushes at positions 1024 .. 1026 of LONG_SCHEDULE (5 tiles per unit)
    and not by anything in SCHEDULE.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import record_report
from helpers import audio, golden, index_report, rms
from test_gpu_parity import WAV_RMS_TOL, _assert_flips_are_near_ties, _prefix_before
from test_seq_transformer_gpu import BLOCK_ABS_TOL, BLOCK_RMS_TOL, MAN, _block_engine, _engine, _state, transformer_f64
from test_seqstream_host import LONG_SCHEDULE, SCHEDULE, causal_tinytf
from test_stream_gpu import pushes, stream_decode, stream_encode

from funcodec_amd.engine import EngineError

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def _tiny():
    """the tiny causal transformer net (tinytf made causal as _block_engine does): hop 8, 6 quantisers, first push 7 frames"""
    from funcodec_amd.model import EncodecMI355X
    arch, sd = _state(causal_tinytf(), 31)
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m, sd


def _streamed(st, x, schedule, decoder=False):
    out, pos = [], 0
    for n in schedule:
        out.append(st.seq_forward(x[..., pos:pos + n].contiguous(), decoder=decoder))
        pos += n
    assert pos == x.shape[-1]
    return torch.cat(out, -1)


# ---- 1. the stage against float64 ----------------------------------------------------------------------------------------------
def _stage_case(C, B, schedule, decoder=False):
    m, sd, prefix, arch = _block_engine(C, True)
    if decoder:
        prefix = [k[: -len(".after_norm.weight")] for k in sd if k.startswith("decoder.") and k.endswith(".after_norm.weight")][0]
    T = sum(schedule)
    x = torch.randn(B, C, T, generator=torch.Generator().manual_seed(C * 7919 + B * 31 + T))
    st = m.open_stream(B, max_frames=T)                    # the last push ends exactly at the bound
    y = _streamed(st, x.cuda(), schedule, decoder).cpu().double()
    ref = transformer_f64(x, sd, prefix, arch.lstm_layers, True, False)
    e_max, e_rms = float((y - ref).abs().max()), float((y - ref).pow(2).mean().sqrt())
    print(f"seqstream stage C={C} B={B} T={T} decoder={decoder}: max abs {e_max:.3e}, rms {e_rms:.3e}")
    assert bool(torch.isfinite(y).all())
    assert e_max < BLOCK_ABS_TOL and e_rms < BLOCK_RMS_TOL, (C, B, T, e_max, e_rms)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [64, 128, 256, 512, 1024])
def test_streamed_stage_against_float64(C, B):
    _stage_case(C, B, SCHEDULE)                            # max_frames = 131: not a multiple of 16


@pytest.mark.parametrize("C", [64, 512])
def test_streamed_stage_against_float64_long(C):
    _stage_case(C, 1, LONG_SCHEDULE)


def test_streamed_stage_against_float64_decoder_side():
    _stage_case(128, 3, SCHEDULE, decoder=True)


# ---- 2. bit for bit ---------------------------------------------------------------------------------------------------------------
BITS = [130, 1, 16, 17, 100, 1, 15, 1, 300, 1, 1]          # split pushes on 5 .. 16 units (the cap) and many-query pushes, to 583 frames


def test_replay_batch_independence_and_a_dirty_cache_bit_for_bit():
    C, B, T = 256, 3, sum(BITS)
    m, sd, prefix, arch = _block_engine(C, True)
    x = torch.randn(B, C, T, generator=torch.Generator().manual_seed(77)).cuda()
    st = m.open_stream(B, max_frames=T + 5)
    first = _streamed(st, x, BITS)
    st.reset()
    assert torch.equal(_streamed(st, x, BITS), first)
    for b in range(B):                                     # a row's result does not depend on B
        one = m.open_stream(1, max_frames=T + 5)
        assert torch.equal(_streamed(one, x[b:b + 1], BITS), first[b:b + 1]), b
    dirty = m.open_stream(B, max_frames=T + 5)
    dirty.state.fill_(0xFF)                                # NaN in every float: a frame is written before it is read, loads are clamped
    dirty.reset()
    got = _streamed(dirty, x, BITS)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, first)
    m.engine.check_status()


# ---- 3. end to end against the real reference ----------------------------------------------------------------------------------------
def check_against_reference(name, m, arch, sd, n_q, wav, ref_idx, ref_enc, ref_quant, ref_recon, scale, how, max_frames):
    """tests/test_stream_gpu.py::check_against_reference with sessions opened with max_frames: the same bars"""
    B, T = wav.shape[0], wav.shape[-1]
    hop = m.engine.hop_length
    st = m.open_stream(B, n_q=n_q, scale=scale, max_frames=max_frames)
    chunks = pushes(T, hop, how)
    codes, quant, enc, emitted = stream_encode(st, wav, chunks)
    assert sum(emitted) == ref_idx.shape[2] == m.engine.frames(T)
    e_enc = rms(enc, ref_enc)
    rep = index_report(codes, ref_idx)
    fchunks = [max(1, n // hop) for n in chunks]
    fchunks[-1] += codes.shape[-1] - sum(fchunks)
    recon = stream_decode(st, codes.permute(1, 2, 0).contiguous(), fchunks)[..., :T]
    recon_e = stream_decode(m.open_stream(B, n_q=n_q, scale=scale, max_frames=max_frames), quant, fchunks, emb=True)[..., :T]
    e_wav = rms(recon, ref_recon)
    print(f"{name} [{how}] B={B} T={T}: enc_out rms {e_enc:.3e}, mismatched indices {rep['mismatched_indices']}/{rep['total_indices']}, "
          f"recon rms {e_wav:.3e}, from embeddings {rms(recon_e, ref_recon):.3e}")
    assert e_enc < 2e-5
    assert arch.codebook_dim == arch.dimension
    if rep["mismatched_indices"] == 0:
        assert rms(quant, ref_quant) == 0.0
        assert e_wav < WAV_RMS_TOL
        assert rms(recon_e, ref_recon) < WAV_RMS_TOL
    else:
        proofs = _assert_flips_are_near_ties(sd["quantizer.rq.model.embed"], torch.as_tensor(ref_enc).float().cpu(), np.asarray(ref_idx), codes,
                                             got_enc=enc.float().cpu(), max_frames=max(1, rep["frames"] // 250))
        print(f"{name} [{how}]: tie proofs (stage, frame, gap, bound) {proofs}")
        Tf = ref_idx.shape[2]
        for b in range(B):
            cut = _prefix_before([p[1] for p in proofs], Tf, hop, b)
            n = T if cut is None else min(cut, T)
            if n > 0:
                assert rms(recon[b, :, :n], torch.as_tensor(ref_recon)[b, :, :n]) < WAV_RMS_TOL, (b, n)
                assert rms(recon_e[b, :, :n], torch.as_tensor(ref_recon)[b, :, :n]) < WAV_RMS_TOL, (b, n)
    return codes, recon


@pytest.mark.parametrize("how", ["frames1", "mixed", "single"])
def test_streamed_against_reference_golden(how):
    name = "ss320tfc_b2_t16000"
    c = MAN["cases"][name]
    m, sd = _engine(c["config"], c["weight_seed"])
    wav = audio(c["batch"], c["samples"], c["audio_seed"], c["audio_kind"])
    g = golden(name)
    codes, recon = check_against_reference(name, m, m.arch, sd, c["n_q"], wav, g["indices"].astype(np.int64), g["encoder_out"], g["quantized"],
                                           g["recon"], torch.from_numpy(g["scale"]), how, c["frames"])
    off = m.engine.encode_decode(wav, c["n_q"], use_scale=True)
    record_report("seqstream_vs_offline", fixture=name, chunking=how, codes_equal=bool(torch.equal(off["codes"], codes)),
                  recon_max_abs=float((off["recon"] - recon).abs().max()))


# ---- 4. rules ---------------------------------------------------------------------------------------------------------------------
def test_a_push_past_max_frames_is_refused_and_changes_nothing():
    m, sd = _tiny()
    hop = m.engine.hop_length
    wav = audio(1, hop * 11, 81, "tones")
    st = m.open_stream(1, max_frames=10)
    assert st.max_frames == 10
    first = st.encode(wav[..., :7 * hop])
    assert first[0].shape[-1] == 7
    assert st.encode(wav[..., 7 * hop:10 * hop])[0].shape[-1] == 3
    with pytest.raises(EngineError, match="max_frames"):
        st.encode(wav[..., 10 * hop:])
    # the library's own refusal, reached through the hook (the host check above comes first otherwise): before the first launch, and
    # the session goes on
    x = torch.zeros(1, m.arch.bottleneck_channels, 1).cuda()
    with pytest.raises(EngineError, match="max_frames"):
        st.seq_forward(x)
    tok = first[0].permute(1, 2, 0).contiguous()
    assert st.decode(tok).shape[-1] == 7 * hop            # not broken: the decoder side still has room
    st.reset()
    again = st.encode(wav[..., :7 * hop])
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    with pytest.raises(EngineError, match="seq_model: transformer"):
        m.open_stream(1)
    with pytest.raises(EngineError, match="seq_model: transformer"):
        m.open_slots(1)
    with pytest.raises(EngineError, match="max_frames"):
        m.open_stream(1, max_frames=6)                     # below the first push (7 frames)


def test_max_frames_for_a_net_without_a_transformer_is_refused():
    from helpers import engine_for
    with pytest.raises(EngineError, match="max_frames"):
        engine_for("tinywn", 5).open_stream(1, max_frames=64)


# ---- 5. neighbours ------------------------------------------------------------------------------------------------------------------
def test_sessions_and_offline_calls_do_not_disturb_each_other():
    m, sd = _tiny()
    hop, nq = m.engine.hop_length, m.arch.num_quantizers
    B, nfr = 2, 40
    a, b = audio(B, hop * nfr, 51, "tones"), audio(B, hop * nfr, 52, "noise")
    chunks = pushes(hop * nfr, hop, "mixed")
    fch = [n // hop for n in chunks]

    def alone(wav):
        st = m.open_stream(B, max_frames=nfr)
        codes, quant, enc, emitted = stream_encode(st, wav, chunks)
        tok = codes.permute(1, 2, 0).contiguous()
        return codes, quant, tok, stream_decode(st, tok, fch)
    ca, qa, ta, ra = alone(a)
    cb, qb, tb, rb = alone(b)
    off_ref = m.engine.encode_decode(a, nq)
    s1, s2 = m.open_stream(B, max_frames=nfr), m.open_stream(B, max_frames=nfr)
    o1, o2, pos = [], [], 0
    for i, n in enumerate(chunks):                         # two sessions interleaved, an offline call between the pushes
        final = i == len(chunks) - 1
        o1.append(s1.encode(a[..., pos:pos + n], final=final))
        off = m.engine.encode_decode(a, nq)
        assert torch.equal(off["codes"], off_ref["codes"]) and torch.equal(off["recon"], off_ref["recon"])
        o2.append(s2.encode(b[..., pos:pos + n], final=final))
        pos += n
    assert torch.equal(torch.cat([o[0] for o in o1], -1), ca) and torch.equal(torch.cat([o[0] for o in o2], -1), cb)
    assert torch.equal(torch.cat([o[1] for o in o1], 1), qa) and torch.equal(torch.cat([o[1] for o in o2], 1), qb)
    w1, w2, pos = [], [], 0
    for n in fch:
        w1.append(s1.decode(ta[:, pos:pos + n]))
        off = m.engine.encode_decode(a, nq)
        assert torch.equal(off["recon"], off_ref["recon"])
        w2.append(s2.decode(tb[:, pos:pos + n]))
        pos += n
    assert torch.equal(torch.cat(w1, -1), ra) and torch.equal(torch.cat(w2, -1), rb)


# ---- 6. a bit rate per row -----------------------------------------------------------------------------------------------------------
def test_rows_with_their_own_stage_counts_equal_the_session_with_that_count():
    m, sd = _tiny()
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    frames = [9, 5, 1, 7, 4]
    plan = [[6, 3, 2], [6, 1, 2], [6, 6, 2], [6, 2, 2], [6, 5, 2]]      # row 0 all stages, row 1 another count at every push, row 2 two
    T = sum(frames) * hop
    wav = audio(3, T, 91, "tones")
    chunks = [f * hop for f in frames]
    uniform = {}
    for k in sorted({k for rows in plan for k in rows}):   # the session with that one count, the same pushes: (codes, quantized) per push
        u = m.open_stream(3, n_q=k, max_frames=sum(frames))
        uniform[k] = [u.encode(wav[..., sum(chunks[:p]):sum(chunks[:p + 1])], final=p == len(chunks) - 1) for p in range(len(chunks))]
    st = m.open_stream(3, n_q=plan[0], max_frames=sum(frames))
    twin = m.open_stream(3, max_frames=sum(frames))        # decodes the same embeddings without any row counts
    assert st.n_q == cap
    pos = 0
    for p, (n, rows) in enumerate(zip(chunks, plan)):
        last = p == len(chunks) - 1
        if p:
            st.set_n_q(rows)
        codes, quant = st.encode(wav[..., pos:pos + n], final=last)
        for b, k in enumerate(rows):
            uc, uq = uniform[k][p]
            assert torch.equal(codes[:k, b], uc[:, b]) and torch.equal(quant[b], uq[b]), (p, b, k)
            assert k == cap or int(codes[k:, b].abs().max()) == 0, (p, b, k)
        tok = codes.permute(1, 2, 0).contiguous()
        for b, k in enumerate(rows):                       # what lies behind a row's count is not read
            tok[b, :, k:] = -1
        assert torch.equal(st.decode(tok, final=last), twin.decode_emb(quant, final=last)), p
        pos += n
    m.engine.check_status()
