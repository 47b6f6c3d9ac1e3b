"""`-m gpu` tests of the streaming session (funcodec_amd/stream.py, fc_stream_*).  The yardstick is the reference -- its committed goldens
and the CPU oracle -- never the engine's own offline call; the bars are those of test_gpu_parity.test_e2e_against_reference_golden."""
import functools

import numpy as np
import pytest
import torch

from conftest import record_report
from helpers import audio, engine_for, golden, index_report, manifest, oracle_for, rms, state_for
from test_gpu_parity import WAV_RMS_TOL, _assert_flips_are_near_ties, _prefix_before

pytestmark = pytest.mark.gpu
MAN = manifest()
GOLDENS = ["ss320_b1_t8000", "tinywn_b2_t777", "tinystwn_b2_t777", "ds320wn_b1_t12000"]
MIXED = [3, 1, 5, 2, 1, 8]


def pushes(T, hop, how):
    """sample counts of the pushes of a T-sample utterance: every push but the last a multiple of the hop"""
    if how == "single":
        return [T]
    frames = [1] * (T // hop) if how == "frames1" else []
    left = T // hop
    while how == "mixed" and left > 0:
        frames.append(min(MIXED[len(frames) % len(MIXED)], left))
        left -= frames[-1]
    out = [f * hop for f in frames]
    if T % hop:
        out.append(T % hop)
    return out


def stream_encode(st, wav, chunks):
    codes, quant, enc, pos = [], [], [], 0
    for i, n in enumerate(chunks):
        c, q, e = st.encode(wav[..., pos:pos + n], final=i == len(chunks) - 1, want_enc_out=True)
        pos += n
        codes.append(c); quant.append(q); enc.append(e)
    return torch.cat(codes, -1), torch.cat(quant, 1), torch.cat(enc, 1), [c.shape[-1] for c in codes]


def stream_decode(st, tokens, frame_chunks, emb=False):
    out, pos = [], 0
    for n in frame_chunks:
        out.append((st.decode_emb if emb else st.decode)(tokens[:, pos:pos + n]))
        pos += n
    return torch.cat(out, -1)


def check_against_reference(name, m, arch, sd, n_q, wav, ref_idx, ref_enc, ref_quant, ref_recon, scale, how):
    """the bars of test_e2e_against_reference_golden on a streamed encode and a streamed decode of the streamed codes"""
    B, T = wav.shape[0], wav.shape[-1]
    hop = m.engine.hop_length
    st = m.open_stream(B, n_q=n_q, scale=scale)
    chunks = pushes(T, hop, how)
    codes, quant, enc, emitted = stream_encode(st, wav, chunks)
    assert sum(emitted) == ref_idx.shape[2] == m.engine.frames(T)
    e_enc = rms(enc, ref_enc) if ref_enc is not None else float("nan")
    rep = index_report(codes, ref_idx)
    fchunks = [max(1, n // hop) for n in chunks]
    fchunks[-1] += codes.shape[-1] - sum(fchunks)
    recon = stream_decode(st, codes.permute(1, 2, 0).contiguous(), fchunks)[..., :T]
    recon_e = stream_decode(m.open_stream(B, n_q=n_q, scale=scale), quant, fchunks, emb=True)[..., :T]
    e_wav = rms(recon, ref_recon)
    print(f"{name} [{how}] B={B} T={T}: enc_out rms {e_enc:.3e}, mismatched indices {rep['mismatched_indices']}/{rep['total_indices']}, "
          f"recon rms {e_wav:.3e}, from embeddings {rms(recon_e, ref_recon):.3e}")
    if ref_enc is not None:
        assert e_enc < 2e-5
    projected = arch.codebook_dim != arch.dimension
    qtol = 1e-5 * float(np.sqrt((np.asarray(ref_quant) ** 2).mean())) if projected else 0.0
    if rep["mismatched_indices"] == 0:
        assert rms(quant, ref_quant) <= qtol
        assert e_wav < WAV_RMS_TOL
        assert rms(recon_e, ref_recon) < WAV_RMS_TOL
    else:
        proofs = _assert_flips_are_near_ties(sd["quantizer.rq.model.embed"], torch.as_tensor(ref_enc).float().cpu(), np.asarray(ref_idx), codes,
                                             got_enc=enc.float().cpu(), max_frames=max(1, rep["frames"] // 250))
        Tf = ref_idx.shape[2]
        for b in range(B):
            cut = _prefix_before([p[1] for p in proofs], Tf, hop, b)
            n = T if cut is None else min(cut, T)
            if n > 0:
                assert rms(recon[b, :, :n], torch.as_tensor(ref_recon)[b, :, :n]) < WAV_RMS_TOL, (b, n)
    return codes, recon


@pytest.mark.parametrize("how", ["frames1", "mixed", "single"])
@pytest.mark.parametrize("name", GOLDENS)
def test_streamed_against_reference_golden(name, how):
    c = MAN["cases"][name]
    m = engine_for(c["config"], c["weight_seed"], c["codebook_decay"])
    cfg, arch, sd = state_for(c["config"], c["weight_seed"], c["codebook_decay"])
    wav = audio(c["batch"], c["samples"], c["audio_seed"], c["audio_kind"], c.get("channels", 1))
    g = golden(name)
    scale = torch.from_numpy(g["scale"]) if "scale" in g else None
    codes, recon = check_against_reference(name, m, arch, sd, c["n_q"], wav, g["indices"].astype(np.int64), g.get("encoder_out"), g["quantized"],
                                           g["recon"], scale, how)
    # recorded, not asserted: streamed against the engine's own offline call (the planner may pick another kernel class for a short chunk)
    off = m.engine.encode_decode(wav, c["n_q"], use_scale=True)
    record_report("stream_vs_offline", fixture=name, chunking=how, codes_equal=bool(torch.equal(off["codes"], codes)),
                  recon_max_abs=float((off["recon"] - recon).abs().max()))


@pytest.mark.parametrize("extra", ["0", "1", "hop-1"])
@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("cfg_name", ["tinyss", "tinywn"])
def test_streamed_against_the_oracle(cfg_name, B, extra):
    """lengths and seeds without a golden: pushes of one frame (shorter than most carries) and pushes longer than any carry"""
    m = engine_for(cfg_name, 5)
    cfg, arch, sd = state_for(cfg_name, 5)
    hop = m.engine.hop_length
    T = hop * 40 + {"0": 0, "1": 1, "hop-1": hop - 1}[extra]
    wav = audio(B, T, 300 + B, "tones")
    ref = oracle_for(cfg_name, 5).inference(wav, bit_width=None, use_scale=True)
    for how in ("frames1", "mixed"):
        check_against_reference(cfg_name, m, arch, sd, arch.num_quantizers, wav, ref["code_indices"][0].numpy(), ref["encoder_out"],
                                ref["code_embeddings"][0][0], ref["recon_speech"], ref["scale"], how)


def _run(m, B, wav, chunks, scale=None, st=None):
    st = st or m.open_stream(B, scale=scale)
    codes, quant, enc, emitted = stream_encode(st, wav, chunks)
    rec = stream_decode(st, codes.permute(1, 2, 0).contiguous(), [codes.shape[-1]])
    return codes, quant, rec, emitted, st


@pytest.mark.parametrize("cfg_name", ["tinyss", "tinywn"])
def test_causality_batch_independence_and_replay_bit_for_bit(cfg_name):
    m = engine_for(cfg_name, 5)
    hop = m.engine.hop_length
    B, nfr = 3, 30
    a = audio(B, hop * nfr, 41, "tones")
    b = a.clone()
    mpush = 12                                             # identical first 12 one-frame pushes, different rest
    b[..., mpush * hop:] = audio(B, hop * (nfr - mpush), 42, "noise")
    chunks = [hop] * nfr
    ca, qa, ra, ea, st = _run(m, B, a, chunks)
    cb, qb, rb, eb, _ = _run(m, B, b, chunks)
    assert ea == eb and sum(ea[:mpush]) > 0, "the start-up must be over before the utterances part"
    n = sum(ea[:mpush])                                    # frames emitted up to push m
    assert torch.equal(ca[..., :n], cb[..., :n]) and torch.equal(qa[:, :n], qb[:, :n])
    ena, enb = stream_encode(m.open_stream(B), a, chunks)[2], stream_encode(m.open_stream(B), b, chunks)[2]
    assert torch.equal(ena[:, :n], enb[:, :n]) and not torch.equal(ena[:, n:], enb[:, n:])     # the check can fail: the rest does differ
    # decode: the samples of the first n frames do not depend on later frames
    st_a, st_b = m.open_stream(B), m.open_stream(B)
    wa = torch.cat([st_a.decode(ca.permute(1, 2, 0)[:, :n].contiguous()), st_a.decode(ca.permute(1, 2, 0)[:, n:].contiguous())], -1)
    wb = torch.cat([st_b.decode(cb.permute(1, 2, 0)[:, :n].contiguous()), st_b.decode(cb.permute(1, 2, 0)[:, n:].contiguous())], -1)
    assert torch.equal(wa[..., :n * hop], wb[..., :n * hop])
    # a stream of the batch equals the same stream run alone
    for i in range(B):
        ci, qi, ri, _, _ = _run(m, 1, a[i:i + 1], chunks)
        assert torch.equal(ci, ca[:, i:i + 1]) and torch.equal(qi, qa[i:i + 1]) and torch.equal(ri, ra[i:i + 1])
    # reset, then replay, with the workspace filled with something else in between
    m.engine._ws.fill_(0xA5)
    st.reset()
    c2, q2, r2, _, _ = _run(m, B, a, chunks, st=st)
    assert torch.equal(c2, ca) and torch.equal(q2, qa) and torch.equal(r2, ra)


def test_sessions_and_offline_calls_do_not_disturb_each_other():
    m = engine_for("tinywn", 5)
    hop = m.engine.hop_length
    B, nfr = 2, 24
    a, b = audio(B, hop * nfr, 51, "tones"), audio(B, hop * nfr, 52, "noise")
    chunks = pushes(hop * nfr, hop, "mixed")
    ca, qa, ra, _, _ = _run(m, B, a, chunks)
    cb, qb, rb, _, _ = _run(m, B, b, chunks)
    off_ref = m.engine.encode_decode(a, m.arch.num_quantizers)
    s1, s2 = m.open_stream(B), m.open_stream(B)
    o1, o2, pos = [], [], 0
    for i, n in enumerate(chunks):                         # two sessions interleaved, an offline call between the pushes
        final = i == len(chunks) - 1
        o1.append(s1.encode(a[..., pos:pos + n], final=final))
        off = m.engine.encode_decode(a, m.arch.num_quantizers)
        assert torch.equal(off["codes"], off_ref["codes"]) and torch.equal(off["recon"], off_ref["recon"])
        o2.append(s2.encode(b[..., pos:pos + n], final=final))
        pos += n
    c1, c2 = torch.cat([o[0] for o in o1], -1), torch.cat([o[0] for o in o2], -1)
    assert torch.equal(c1, ca) and torch.equal(c2, cb)
    assert torch.equal(torch.cat([o[1] for o in o1], 1), qa) and torch.equal(torch.cat([o[1] for o in o2], 1), qb)
    # decode: two sessions interleaved push by push against each of them run alone under the same chunking, bit for bit
    ta, tb = c1.permute(1, 2, 0).contiguous(), c2.permute(1, 2, 0).contiguous()
    alone_a, alone_b = stream_decode(m.open_stream(B), ta, (10, 1, 13)), stream_decode(m.open_stream(B), tb, (10, 1, 13))
    w1, w2, pos = [], [], 0
    for n in (10, 1, 13):
        w1.append(s1.decode(ta[:, pos:pos + n]))
        m.engine.encode_decode(a, m.arch.num_quantizers)
        w2.append(s2.decode(tb[:, pos:pos + n]))
        pos += n
    assert torch.equal(torch.cat(w1, -1), alone_a) and torch.equal(torch.cat(w2, -1), alone_b)


def test_a_push_that_breaks_the_rules_fails_with_a_message():
    from funcodec_amd.engine import EngineError
    m = engine_for("tinywn", 5)
    hop = m.engine.hop_length
    st = m.open_stream(1)
    with pytest.raises(EngineError, match="multiple of the hop"):
        st.encode(torch.zeros(1, hop * 9 + 3))
    st.encode(torch.zeros(1, hop * 9), final=True)
    with pytest.raises(EngineError, match="final push"):
        st.encode(torch.zeros(1, hop))
    st.reset()
    with pytest.raises(EngineError, match="first push"):   # a whole utterance shorter than the start-up: the offline call's job
        st.encode(torch.zeros(1, hop * 2), final=True)


@pytest.mark.parametrize("cfg_name", ["tinyss", "tinywn"])
def test_frames_of_one_push_do_not_depend_on_later_samples(cfg_name):
    """Look-ahead inside ONE push, where it could happen: two utterances that share their first 20 frames and differ afterwards, each
    encoded (and its codes decoded) in a single push.  Past the start-up reflection -- at most 14 frames of samples for these nets, the sum
    over the layers of padding_total x samples per column -- a frame sees nothing later, so the first 20 frames agree bit for bit while
    the rest differs.  (With pushes that END at frame 20 the later samples are not even passed in: that shows determinism only.)"""
    m = engine_for(cfg_name, 5)
    hop = m.engine.hop_length
    B, nfr, keep = 2, 36, 20
    a = audio(B, hop * nfr, 61, "tones")
    b = a.clone()
    b[..., keep * hop:] = audio(B, hop * (nfr - keep), 62, "noise")
    sa, sb = m.open_stream(B), m.open_stream(B)
    ca, qa, ea = sa.encode(a, final=True, want_enc_out=True)
    cb, qb, eb = sb.encode(b, final=True, want_enc_out=True)
    assert torch.equal(ea[:, :keep], eb[:, :keep]) and torch.equal(ca[..., :keep], cb[..., :keep]) and torch.equal(qa[:, :keep], qb[:, :keep])
    assert not torch.equal(ea[:, keep:], eb[:, keep:])
    # decoder: embeddings that agree on the first 20 frames only (the synthetic codebooks give these nets nearly constant codes)
    za = ea
    zb = torch.cat([ea[:, :keep], eb[:, keep:]], 1).contiguous()
    wa, wb = sa.decode_emb(za, final=True), sb.decode_emb(zb, final=True)
    assert torch.equal(wa[..., :keep * hop], wb[..., :keep * hop]) and not torch.equal(wa[..., keep * hop:], wb[..., keep * hop:])


@functools.lru_cache(maxsize=None)
def _seam_net(H):
    """(model, state dict) of a causal weight_norm net whose bottleneck LSTMs are H wide, 2 layers"""
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.model import EncodecMI355X
    from funcodec_amd.synth import make_state_dict
    cfg = recipe_config("ds320wn" if H == 512 else "tinywn")
    if H != 512:
        for k in ("encoder_conf", "decoder_conf"):
            cfg[k].update(n_filters=H // 4)            # ratios (4, 2): the bottleneck is 4 n_filters wide
    arch = arch_from_config(cfg)
    assert (arch.bottleneck_channels, arch.lstm_layers, arch.causal) == (H, 2, True)
    sd = make_state_dict(arch, 700 + H)
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m, sd


@pytest.mark.parametrize("T2", [1, 10])
@pytest.mark.parametrize("T1", [1, 7])
@pytest.mark.parametrize("H", [64, 512])
def test_lstm_seam_one_push_equals_two_bit_for_bit(H, T1, T2):
    """The LSTM stage of a stream over T1 + T2 steps in one push against two pushes of T1 and T2 steps: the same kernel, the same order per
    accumulator and the same state, so the bits are the same; both within test_lstm_kernels.py's float64 bar.  Encoder and decoder LSTM."""
    from test_lstm_kernels import _check, _torch_lstm
    m, sd = _seam_net(H)
    B, T = 3, T1 + T2
    x = torch.randn(B, H, T, generator=torch.Generator().manual_seed(10 * H + T))
    for decoder in (False, True):
        side = "decoder." if decoder else "encoder."
        prefix = [k[: -len(".weight_ih_l0")] for k in sd if k.startswith(side) and k.endswith(".weight_ih_l0")][0]
        st = m.open_stream(B)
        whole = st.lstm_forward(x, decoder=decoder)
        st.reset()
        parts = torch.cat([st.lstm_forward(x[..., :T1].contiguous(), decoder=decoder), st.lstm_forward(x[..., T1:].contiguous(), decoder=decoder)], -1)
        assert torch.equal(whole, parts), (H, T1, T2, decoder, float((whole - parts).abs().max()))
        refs = []
        for dtype in (torch.float64, torch.float32):
            with torch.no_grad():
                refs.append(_torch_lstm(sd, prefix, H, 2, dtype)(x.to(dtype).permute(2, 0, 1))[0].permute(1, 2, 0).double().contiguous())
        _check((H, 2, False, B, T, 1.0), whole.cpu(), refs[0], refs[1], "stream")
        m.engine.check_status()


def test_decode_final_raises_while_frames_are_held_back_and_a_failed_push_invalidates_the_utterance():
    from funcodec_amd.engine import EngineError
    m = engine_for("tinywn", 5)
    hop = m.engine.hop_length
    st = m.open_stream(1)
    few = torch.zeros(1, st.min_first_frames - 1, m.arch.num_quantizers, dtype=torch.long)
    assert st.decode(few).shape[-1] == 0
    st.reset()
    with pytest.raises(EngineError, match="fewer than"):
        st.decode(few, final=True)
    # a push that fails inside the library (a workspace that is too small): the session refuses to go on until reset, then replays
    wav = audio(1, hop * 20, 71, "tones")
    good = m.open_stream(1).encode(wav, final=True)
    st.reset()
    keep_ws, keep_need = m.engine._ws, st._ws_bytes
    m.engine._ws, st._ws_bytes = torch.empty(8192, dtype=torch.uint8, device=m.device), 8192
    with pytest.raises(EngineError, match="workspace too small"):
        st.encode(wav, final=True)
    m.engine._ws, st._ws_bytes = keep_ws, keep_need
    with pytest.raises(EngineError, match="fc_stream_reset"):
        st.encode(wav, final=True)
    st.reset()
    again = st.encode(wav, final=True)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])
