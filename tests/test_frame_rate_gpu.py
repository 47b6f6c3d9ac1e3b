"""A stage count per FRAME chosen on the device by a target SNR (fc_engine_set_rate_frames, fc_engine_set_frame_nq; csrc/
rvq_rate_kernels.h states the rule) on the MI355X: the pick against ``rate_pick_frames`` of the device's own errors, the row
outputs against float64 numpy, every frame against today's call with its count, and the decode with a count per frame.  Comparisons
are exact unless said otherwise."""
import numpy as np
import pytest
import torch

from funcodec_amd.engine import EngineError, rate_pick_frames, rate_targets
from helpers import audio, engine_for
from test_rvq_rate_gpu import _codebooks, _rvq_engine

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
B, TF, CAP = 5, 7, 32
TARGETS = [6.0, 12.0, 20.0, 12.0, 6.0]
CAPS = [32, 9, 32, 20, 5]
GARBAGE = (-1, (1 << 40) + 5)


def frame_rows(dim, Tf=TF, seed=0, rows=B):
    """[rows * Tf, dim] float32: every FRAME is the sum of its own number (0 .. 32) of random code vectors, one of each of its first
    stages, plus 0.02 N(0, 1); frame (1, 2 mod Tf) is all zero.  (The seeds used below were checked on the CPU with a numpy greedy
    quantiser: the smallest relative distance of an err * F from its threshold is 1e-5 or more.)"""
    rng = np.random.default_rng(7000 + 31 * dim + 7 * Tf + seed)
    cb = _codebooks(dim)
    x = np.zeros((rows, Tf, dim), np.float32)
    for b in range(rows):
        for t in range(Tf):
            dep = int(rng.integers(0, 33))
            idx = rng.integers(0, cb.shape[1], dep)
            x[b, t] = cb[np.arange(dep), idx].astype(np.float64).sum(0) + 0.02 * rng.standard_normal(dim)
    x[1, 2 % Tf] = 0.0
    return torch.from_numpy(x.reshape(-1, dim))


def tree_sum(vals):
    """the order the row sums take: 256 partials (partial j takes t = j, j + 256, ...), then a binary tree -- in float64"""
    p = np.zeros(256, np.float64)
    for t, v in enumerate(vals):
        p[t % 256] = p[t % 256] + np.float64(v)
    o = 128
    while o >= 1:
        p[:o] = p[:o] + p[o:2 * o]
        o //= 2
    return p[0]


def frame_margin(err, E, ratios, caps, floor, frames=None):
    m = INF
    for b, rho in enumerate(ratios):
        if not np.all(np.isfinite(E[b][:caps[b] + 1])) or rho in (0.0, INF) or E[b][0] == 0.0:
            continue
        F = err.shape[2] if frames is None else frames[b]
        thr = float(E[b][0]) * rho
        lo = min(floor, caps[b])
        v = err[lo:caps[b] + 1, b, :F].astype(np.float64) * float(F)
        if v.size:
            m = min(m, float(np.min(np.abs(v - thr) / thr)))
    return m


def check_frames(eng, x, Bn, targets, floor=0, caps=None, beam=1):
    """One frame-mode call of the hook against rate_pick_frames, float64 numpy and today's call per count; returns its outputs."""
    dim, Tf = x.shape[1], x.shape[0] // Bn
    cap_rows = [CAP] * Bn if caps is None else list(caps)
    ratios = rate_targets(eng.arch, targets, Bn)
    full_c, _ = eng.rvq_encode(x, CAP, n_q_rows=caps, beam=beam)
    codes, quant, rate = eng.rvq_encode(x, CAP, n_q_rows=caps, beam=beam, target_snr_db=targets, min_n_q=floor, per_frame=True)
    kf = rate["n_q_frames"].cpu().numpy()
    err = rate["stage_errors"].cpu().numpy()
    E = rate["row_errors"].cpu().numpy()
    assert rate["n_q_frames"].dtype == torch.int32 and kf.shape == (Bn, Tf) and rate["n_codes_rows"].dtype == torch.int32
    margin = frame_margin(err, E, ratios, cap_rows, floor)
    print(f"D {dim} Tf {Tf} floor {floor} beam {beam}: mean k per row {kf.mean(1).round(2).tolist()}, margin {margin:.3e}")
    assert margin >= 1e-6, "an err * F lies on its threshold: pick another seed"
    for b in range(Bn):
        assert np.array_equal(kf[b], rate_pick_frames(err[:, b], E[b], ratios[b], floor, cap_rows[b])), b
    assert rate["n_q_rows"].tolist() == kf.max(1).tolist() and rate["n_codes_rows"].tolist() == kf.sum(1).tolist()
    ach = np.array([tree_sum([err[kf[b, t], b, t] for t in range(Tf)]) for b in range(Bn)])
    np.testing.assert_allclose(rate["achieved_errors"].cpu().numpy(), ach, rtol=1e-12, atol=0)
    # every frame is the frame of today's call with its count: the frames with k >= 1 as utterances of one frame each
    flat = kf.reshape(-1)
    c, fc = codes.cpu().numpy(), full_c.cpu().numpy()
    for n, k in enumerate(flat):
        assert np.array_equal(c[:k, n], fc[:k, n]) and not c[k:, n].any(), n
    idx = torch.from_numpy(np.nonzero(flat >= 1)[0]).to(x.device)
    zero = torch.from_numpy(np.nonzero(flat == 0)[0]).to(x.device)
    assert float(quant[zero].abs().sum()) == 0.0 and int(codes[:, zero].abs().sum()) == 0
    if beam == 1 and caps is None:
        c1, q1 = eng.rvq_encode(x[idx].contiguous(), CAP, n_q_rows=flat[flat >= 1].tolist())
        assert torch.equal(codes[:, idx], c1) and torch.equal(quant[idx], q1)
    # the decode with a count per frame gives the call's quantized, whoever found the codes (where the net has no projection between
    # the codebooks' space and the decoder's: the hook's quantized lives in the former, the decode call's embeddings in the latter)
    tok = codes.reshape(CAP, Bn, Tf).permute(1, 2, 0).contiguous()
    if dim == eng.arch.dimension:
        _, emb = eng.decode_codes(tok, n_q_frames=rate["n_q_frames"])
        assert torch.equal(emb, quant.reshape(Bn, Tf, dim))
    return dict(codes=codes, quant=quant, kf=kf, rate=rate, full=full_c, tok=tok)


@pytest.mark.parametrize("dim", [16, 128, 512])
@pytest.mark.parametrize("floor", [0, 2])
def test_the_pick_per_frame_and_every_frame_against_its_count(dim, floor):
    eng = _rvq_engine(dim).engine
    x = frame_rows(dim).to(eng.device)
    r = check_frames(eng, x, B, TARGETS, floor)
    assert r["kf"].min() >= floor and len(set(r["kf"].reshape(-1).tolist())) > 3, "the frames take different counts"
    assert floor > 0 or r["kf"][1, 2] == 0, "the all-zero frame meets its threshold without a stage"
    c = check_frames(eng, x, B, TARGETS, floor, caps=CAPS)
    assert all(int(c["kf"][b].max()) <= CAPS[b] for b in range(B))
    eng.check_status()


def test_a_row_longer_than_the_256_partial_sums():
    eng = _rvq_engine(128).engine
    x = frame_rows(128, 300).to(eng.device)
    check_frames(eng, x, B, TARGETS)
    eng.check_status()


def test_with_rvq_beam_a_frame_takes_a_prefix_of_the_full_depth_path():
    eng = _rvq_engine(16).engine
    x = frame_rows(16, seed=2).to(eng.device)
    check_frames(eng, x, B, TARGETS, beam=4)
    eng.check_status()


def test_a_nan_row_takes_its_cap_in_every_frame_and_leaves_the_others_alone():
    eng = _rvq_engine(128).engine
    x = frame_rows(128, seed=3).to(eng.device)
    clean = check_frames(eng, x, B, TARGETS, caps=CAPS)
    bad = x.clone()
    for b in (0, 2, 4):
        bad[b * TF + 3] = NAN                                          # one frame poisons the row's sums
    codes, quant, rate = eng.rvq_encode(bad, CAP, n_q_rows=CAPS, target_snr_db=TARGETS, min_n_q=0, per_frame=True)
    kf = rate["n_q_frames"].cpu().numpy()
    for b in (0, 2, 4):
        assert kf[b].tolist() == [CAPS[b]] * TF
    for b in (1, 3):
        rows = slice(b * TF, (b + 1) * TF)
        assert np.array_equal(kf[b], clean["kf"][b])
        assert torch.equal(codes[:, rows], clean["codes"][:, rows]) and torch.equal(quant[rows], clean["quant"][rows])
        assert torch.equal(rate["achieved_errors"][b], clean["rate"]["achieved_errors"][b])
    eng.check_status()


def test_a_row_alone_and_among_four_others_gives_equal_results():
    eng = _rvq_engine(128).engine
    x = frame_rows(128, seed=4).to(eng.device).reshape(B, TF, 128)
    row, others = x[2:3], x[[0, 1, 3, 4]]
    alone = eng.rvq_encode(row.reshape(-1, 128), CAP, target_snr_db=[12.0], per_frame=True)
    first = eng.rvq_encode(torch.cat([row, others]).reshape(-1, 128), CAP, target_snr_db=[12.0, 3.0, 40.0, 6.0, INF], per_frame=True)
    last = eng.rvq_encode(torch.cat([others, row]).reshape(-1, 128), CAP, target_snr_db=[3.0, 40.0, 6.0, INF, 12.0], per_frame=True)
    for (codes, quant, rate), b in ((first, 0), (last, 4)):
        rows = slice(b * TF, (b + 1) * TF)
        assert torch.equal(rate["n_q_frames"][b], alone[2]["n_q_frames"][0])
        assert torch.equal(codes[:, rows], alone[0]) and torch.equal(quant[rows], alone[1])
        for key in ("n_q_rows", "n_codes_rows", "achieved_errors"):
            assert torch.equal(rate[key][b], alone[2][key][0]), key
    eng.check_status()


# ---- the offline calls -----------------------------------------------------------------------------------------------------------------
def _frames_of(m, lens):
    return [m.engine.frames(int(n)) for n in lens]


def test_ragged_lengths_with_nan_behind_them():
    m = engine_for("tiny", 5, 0.8)
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    T = 3003
    lens = [T, T - 7 * hop - 3, T - 100 * hop]
    wav = audio(3, T, 761, "tones").clone()
    for b, n in enumerate(lens):
        wav[b, n:] = NAN                                               # never read
    targets = [2.0, 6.0, 4.0]
    r = m.inference(wav, target_snr_db=targets, per_frame=True, min_n_q=0, speech_lengths=torch.tensor(lens))
    kf = r["n_q_frames"]
    assert kf.dtype == torch.int32 and r["row_snr_db"].dtype == torch.float64 and bool(torch.isfinite(r["row_snr_db"]).all())
    assert r["n_q_rows"].tolist() == kf.max(1).values.tolist() and r["n_codes_rows"].tolist() == kf.sum(1).tolist()
    assert bool(torch.isfinite(r["recon_speech"]).all())
    for b, n in enumerate(lens):                                       # a row is the row alone, its counts too; zeros behind its frames
        f = m.engine.frames(n)
        one = m.inference(wav[b:b + 1, :n], target_snr_db=targets[b], per_frame=True, min_n_q=0, speech_lengths=[n])
        assert torch.equal(one["n_q_frames"][0], kf[b, :f]) and int(kf[b, f:].abs().sum()) == 0
        assert torch.equal(one["code_indices"][0][:, 0], r["code_indices"][0][:, b, :f])
        assert torch.equal(one["recon_speech"][0, :, :n], r["recon_speech"][b, :, :n])
        assert torch.equal(one["row_snr_db"][0], r["row_snr_db"][b])
    # the engine's pick is rate_pick_frames of its own errors, with the row's own frame count
    e = m.engine.encode(wav, cap, target_snr_db=targets, lengths=lens, per_frame=True, min_n_q=0, want_stage_errors=True)
    err, E = e["stage_errors"].cpu().numpy(), e["row_errors"].cpu().numpy()
    ratios = rate_targets(m.arch, targets, 3)
    fr = _frames_of(m, lens)
    assert frame_margin(err, E, ratios, [cap] * 3, 0, fr) >= 1e-6, "pick another seed"
    for b in range(3):
        assert np.array_equal(e["n_q_frames"][b].cpu().numpy(), rate_pick_frames(err[:, b], E[b], ratios[b], 0, cap, fr[b])), b
    assert torch.equal(e["n_q_frames"], kf)
    m.engine.check_status()


def test_decode_with_a_count_per_frame_reads_nothing_behind_it():
    m = engine_for("tiny", 5, 0.8)
    wav = audio(3, 2003, 762, "tones")
    r = m.inference(wav, target_snr_db=[2.0, 6.0, 4.0], per_frame=True, min_n_q=0)
    kf = r["n_q_frames"]
    assert len(set(kf.reshape(-1).tolist())) > 1
    tok = r["code_indices"][0].permute(1, 2, 0).contiguous()
    want = m.inference_decoding(tok, n_q_frames=kf)
    assert torch.equal(want["code_embeddings"][0][0], r["code_embeddings"][0][0])
    behind = torch.arange(tok.shape[2], device=tok.device)[None, None, :] >= kf[:, :, None]
    for g in GARBAGE:
        dirty = torch.where(behind, torch.full_like(tok, g), tok)
        got = m.inference_decoding(dirty, n_q_frames=kf)
        assert torch.equal(got["recon_speech"], want["recon_speech"]) and torch.equal(got["code_embeddings"][0][0], want["code_embeddings"][0][0])
        m.engine.check_status()                                        # no FC_STATUS_BAD_CODE
    # the length-aware decode: garbage counts behind a row's frames are not looked at either
    lens = [tok.shape[1], tok.shape[1] - 5, 9]
    rag = m.inference_decoding(tok, n_q_frames=kf, token_lengths=torch.tensor(lens))
    kdirty = kf.clone()
    for b, f in enumerate(lens):
        kdirty[b, f:] = 77
    rag2 = m.inference_decoding(tok, n_q_frames=kdirty, token_lengths=torch.tensor(lens))
    assert torch.equal(rag["recon_speech"], rag2["recon_speech"])
    m.engine.check_status()


def test_freq_codec_in_frame_mode():
    from helpers import freq_engine_for
    m = freq_engine_for("tinyfreq", 3)
    wav = audio(3, 1777, 762, "tones")
    cap = m.arch.num_quantizers
    r = m.engine.encode_decode(wav, cap, target_snr_db=[1.0, INF, 3.0], per_frame=True, min_n_q=0, want_stage_errors=True)
    err, E = r["stage_errors"].cpu().numpy(), r["row_errors"].cpu().numpy()
    ratios = rate_targets(m.arch, [1.0, INF, 3.0], 3)
    assert frame_margin(err, E, ratios, [cap] * 3, 0) >= 1e-6
    for b in range(3):
        assert np.array_equal(r["n_q_frames"][b].cpu().numpy(), rate_pick_frames(err[:, b], E[b], ratios[b], 0, cap)), b
    _, emb = m.engine.decode_codes(r["codes"].permute(1, 2, 0).contiguous(), n_q_frames=r["n_q_frames"])
    assert torch.equal(emb, r["quantized"])
    m.engine.check_status()


def test_a_plain_call_after_a_frame_call_is_untouched_and_refusals_come_before_a_launch():
    import ctypes as C
    m = engine_for("tiny", 5, 0.8)
    eng, lib = m.engine, m.engine.lib
    wav = audio(3, 23 * eng.hop_length + 3, 763, "tones")
    before = m.inference(wav)
    rate_before = m.inference(wav, target_snr_db=3.0)
    m.inference(wav, target_snr_db=[1.0, 4.0, INF], per_frame=True, min_n_q=1)
    for kw, word in ((dict(per_frame=True), "target"), (dict(per_frame=True, target_snr_db=3.0, min_n_q=7), "min_n_q"),
                     (dict(per_frame=True, target_snr_db=3.0, min_n_q=-1), "min_n_q")):
        with pytest.raises(EngineError, match=word):
            m.inference(wav, **kw)
    with pytest.raises(EngineError, match="min_n_q"):                 # the floor above a row's cap
        eng.encode(wav, 6, n_q_rows=[1, 2, 3], target_snr_db=3.0, min_n_q=2, per_frame=True)
    # the C side: frame mode needs a rate, an output and a floor in [0, num_quantizers]
    out = torch.zeros(3 * 64, dtype=torch.int32, device=eng.device)
    assert lib.fc_engine_set_rate_frames(eng._h, 0, C.c_void_p(out.data_ptr()), None, None, None) != 0 and "no rate is set" in lib.fc_last_error().decode()
    Tf = eng.frames(wav.shape[-1])
    with eng._rate([0.1] * 3, 1, 6, Tf):
        assert lib.fc_engine_set_rate_frames(eng._h, 0, None, None, None, None) != 0 and "n_q_frames_out" in lib.fc_last_error().decode()
        assert lib.fc_engine_set_rate_frames(eng._h, 7, C.c_void_p(out.data_ptr()), None, None, None) != 0 and "min_nq" in lib.fc_last_error().decode()
    # a frame table of another shape, or beside a row table: refused before the first launch
    tok = before["code_indices"][0].permute(1, 2, 0).contiguous()
    kf = torch.full((3, Tf), 2, dtype=torch.int32, device=eng.device)
    with pytest.raises(EngineError, match="n_q_frames"):
        eng.decode_codes(tok, n_q_frames=kf[:, :-1])
    with pytest.raises(EngineError, match="give one of them"):
        eng.decode_codes(tok, n_q_rows=[1, 2, 3], n_q_frames=kf)
    with eng._frame_nq(kf[:2], 2, Tf):
        with pytest.raises(EngineError, match=r"set for \[2\]\[%d\]" % Tf):
            eng.decode_codes(tok)
    with eng._row_nq([1, 2, 3]):
        assert lib.fc_engine_set_frame_nq(eng._h, C.c_void_p(kf.data_ptr()), 3, Tf, None) != 0 and "fc_engine_set_row_nq" in lib.fc_last_error().decode()
    assert int(out.abs().sum()) == 0
    again, rate_again = m.inference(wav), m.inference(wav, target_snr_db=3.0)
    for a, b in ((again, before), (rate_again, rate_before)):
        assert torch.equal(a["code_indices"][0], b["code_indices"][0]) and torch.equal(a["recon_speech"], b["recon_speech"])
        assert torch.equal(a["code_embeddings"][0][0], b["code_embeddings"][0][0]) and torch.equal(a["sub_quants"][0], b["sub_quants"][0])
    assert "n_q_frames" not in again and "n_q_frames" not in rate_again and torch.equal(rate_again["n_q_rows"], rate_before["n_q_rows"])
    dec_before = eng.decode_codes(tok)
    eng.decode_codes(tok, n_q_frames=kf)
    assert torch.equal(eng.decode_codes(tok)[0], dec_before[0])
    eng.check_status()


def test_a_session_push_is_refused_by_name_while_frame_mode_or_a_frame_table_is_set():
    m = engine_for("tinyss", 5)
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    st = m.open_stream(2)
    slots = m.open_slots(2)
    slots.start(0)
    n = max(st.min_first_samples, slots.min_first_samples, 8 * hop) // hop * hop
    wav = audio(2, n, 764, "tones").to(m.device)
    with m.engine._rate([0.1, 0.1], 0, cap, n // hop, per_frame=True):
        with pytest.raises(EngineError, match="frame mode is set.*offline calls only"):
            st.encode(wav)
        with pytest.raises(EngineError, match="frame mode is set.*offline calls only"):
            slots.encode({0: (wav[0], False)})
    st.reset()
    codes, _ = st.encode(wav)
    kf = torch.full((2, n // hop), 1, dtype=torch.int32, device=m.device)
    with m.engine._frame_nq(kf, 2, n // hop):
        with pytest.raises(EngineError, match="fc_engine_set_frame_nq.*offline decode calls only"):
            st.decode(codes.permute(1, 2, 0).contiguous())
    from funcodec_amd import io as fio
    p1 = fio.pack_frame_codes(np.zeros((cap, 3), np.int64), [1, 0, 1], bits=m.engine.code_bits)
    with pytest.raises(EngineError, match="row 0: packet field mode.*offline calls only"):      # sessions decode packets of mode 0
        st.decode_packed([p1, p1])
    m.engine.check_status()
