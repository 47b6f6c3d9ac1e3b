"""A stage count per row chosen on the device by a target SNR (fc_engine_set_rate; csrc/rvq_rate_kernels.h states the rule) on the
MI355X: the stage errors against a float32 restatement, the row errors against their float64 sum, the pick against ``rate_pick``, and
every output against today's call with the chosen counts."""
import copy
import functools

import numpy as np
import pytest
import torch

from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.engine import EngineError, rate_pick, rate_targets
from funcodec_amd.synth import make_state_dict
from helpers import audio, engine_for

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
DIMS = (16, 32, 64, 128, 256, 512)
DEPTH = (2, 6, 12, 20, 32)
B, TF, CAP = 5, 7, 32
BW = 12000.0          # one stage of the tiny quantisers: log2(64) bits x 16000 / 8 frames per second


# ---- the engine and its inputs ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _arch(dim):
    cfg = copy.deepcopy(recipe_config("tiny"))
    cfg["quantizer_conf"]["num_quantizers"] = 32
    if dim != 16:
        cfg["quantizer_conf"]["codec_dim"] = dim
    arch = arch_from_config(cfg)
    assert arch.codebook_dim == dim and arch.num_quantizers == 32 and arch.codebook_size == 64
    return arch


@functools.lru_cache(maxsize=None)
def _codebooks(dim):
    """[32, 64, dim] float32: sigma falls by 0.8 per stage"""
    return make_state_dict(_arch(dim), 7, 0.8)["quantizer.rq.model.embed"].astype(np.float32)


@functools.lru_cache(maxsize=None)
def _rvq_engine(dim):
    """the tiny net with 32 stages of 64 codes in `dim` dims (the quantiser alone is exercised)"""
    from funcodec_amd.model import EncodecMI355X
    m = EncodecMI355X(_arch(dim), "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(_arch(dim), 7, 0.8).items()})
    return m


def rate_rows(dim, Tf=TF, seed=0, depth=DEPTH):
    """[len(depth) * Tf, dim] float32: every frame of row b is the sum of depth_b random code vectors, one of each of the stages
    0 .. depth_b - 1, plus 0.02 N(0, 1) -- rows a 64-code quantiser can code, to very different depths (Gaussian rows it cannot: at
    128 dims and more they stay below 2 dB at every stage)."""
    rng = np.random.default_rng(9000 + 31 * dim + 7 * Tf + seed)
    cb = _codebooks(dim)
    x = np.zeros((len(depth), Tf, dim), np.float32)
    for b, dep in enumerate(depth):
        for t in range(Tf):
            idx = rng.integers(0, cb.shape[1], dep)
            x[b, t] = cb[np.arange(dep), idx].astype(np.float64).sum(0) + 0.02 * rng.standard_normal(dim)
    return torch.from_numpy(x.reshape(-1, dim))


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _norm32(r):
    """|r|^2 of rows r [..., D] in the order of rvq_row_norm: four chains over D / 4, squares rounded separately, (p0 + p1) + (p2 + p3)"""
    D = r.shape[-1]
    c = r.reshape(r.shape[:-1] + (4, D // 4))
    s = np.zeros(c.shape[:-1], np.float32)
    for d in range(D // 4):
        s = s + c[..., d] * c[..., d]
    return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])


def stage_errors32(x, cb, codes, caps, frames=None):
    """x [B, Tf, D] float32, codes [nq, B, Tf] (full depth), caps [B] -> err [nq + 1, B, Tf] float32: the residual chain in float32,
    element-wise; 0 behind a row's cap and behind its frames"""
    nq, Bn, Tf = codes.shape
    r = x.astype(np.float32).copy()
    err = np.zeros((nq + 1, Bn, Tf), np.float32)
    with np.errstate(all="ignore"):
        for i in range(nq + 1):
            for b in range(Bn):
                f = Tf if frames is None else frames[b]
                if i <= caps[b]:
                    err[i, b, :f] = _norm32(r[b, :f])
                if i < min(caps[b], nq):
                    r[b, :f] = r[b, :f] - cb[i][codes[i, b, :f]]
    return err


def _margin(E, ratios, caps, floor=1):
    """the smallest relative distance of a curve point from its row's threshold (a target of +inf has none)"""
    m = INF
    for b, rho in enumerate(ratios):
        Eb = [float(v) for v in E[b]]
        if not np.all(np.isfinite(Eb[:caps[b] + 1])) or rho in (0.0, INF) or Eb[0] == 0.0:
            continue
        thr = Eb[0] * rho
        m = min(m, min(abs(Eb[k] - thr) / thr for k in range(floor, caps[b] + 1)))
    return m


def _check_rate(eng, x, Bn, target, min_n_q=1, caps=None, beam=1, dim=None):
    """One rate call of the hook against the restatement, rate_pick and today's per-row call; returns its outputs."""
    dim = x.shape[1]
    Tf = x.shape[0] // Bn
    cap_rows = [CAP] * Bn if caps is None else list(caps)
    target = [target] * Bn if isinstance(target, float) else target         # (the hook reads one value as one utterance)
    ratios = rate_targets(eng.arch, target, Bn)
    full_c, _ = eng.rvq_encode(x, CAP, n_q_rows=caps, beam=beam)                       # the codes at the cap
    codes, quant, rate = eng.rvq_encode(x, CAP, n_q_rows=caps, beam=beam, target_snr_db=target, min_n_q=min_n_q)
    ks = rate["n_q_rows"].tolist()
    E = rate["row_errors"].cpu().numpy()
    serr = rate["stage_errors"]
    assert rate["n_q_rows"].dtype == torch.int32 and E.dtype == np.float64 and E.shape == (Bn, CAP + 1) and serr.shape == (CAP + 1, Bn, Tf)
    want = stage_errors32(x.cpu().numpy().reshape(Bn, Tf, dim), _codebooks(dim), full_c.cpu().numpy().reshape(CAP, Bn, Tf), cap_rows)
    got = serr.cpu().numpy()
    differ = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(differ) == 0, (f"stage errors differ from the float32 restatement at {len(differ)} of {want.size} places, first (stage, row, frame) "
                              f"{differ[0].tolist()}: {got[tuple(differ[0])]!r} against {want[tuple(differ[0])]!r}; stages {sorted(set(differ[:, 0].tolist()))}")
    sums = want.astype(np.float64).sum(-1).T                                            # [B, nq + 1]
    np.testing.assert_allclose(E, sums, rtol=1e-12, atol=0)
    margin = _margin(E, ratios, cap_rows, min_n_q)
    print(f"D {dim} Tf {Tf} beam {beam}: k = {ks}, margin {margin:.3e}")
    assert margin >= 1e-6, "a curve point lies on its threshold: pick another seed"
    assert ks == [rate_pick(E[b], ratios[b], min_n_q, cap_rows[b]) for b in range(Bn)]
    for b, k in enumerate(ks):
        rows = slice(b * Tf, (b + 1) * Tf)
        assert torch.equal(codes[:k, rows], full_c[:k, rows]), b
        assert k == CAP or int(codes[k:, rows].abs().max()) == 0, b
    if beam == 1:                                                                       # bit for bit today's per-row call
        c1, q1 = eng.rvq_encode(x, CAP, n_q_rows=ks)
        assert torch.equal(codes, c1) and torch.equal(quant, q1)
    return dict(codes=codes, quant=quant, ks=ks, E=E, serr=serr, full=full_c)


# ---- 1. stage and row errors, every instantiation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_stage_errors_row_errors_and_the_pick(dim):
    eng = _rvq_engine(dim).engine
    x = rate_rows(dim).to(eng.device)
    r = _check_rate(eng, x, B, 12.0)
    assert len(set(r["ks"])) > 1, "the rows take different counts"
    eng.check_status()


def test_rows_past_the_two_row_set_threshold():
    """enough frames for launch_rvq_encode's two-row-set form, odd so that workgroups straddle utterances, and more than 256 frames a
    row: every thread of the row sums adds several"""
    eng = _rvq_engine(128).engine
    n = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    Tf = (n // B + 2) | 1
    x = rate_rows(128, Tf).to(eng.device)
    r = _check_rate(eng, x, B, 12.0)
    assert len(set(r["ks"])) > 1
    eng.check_status()


# ---- 2. targets per row, the floor, a cap per row --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 128])       # (in 16 dims 64 codes keep gaining on every row up to the last stage)
def test_targets_per_row_floor_and_caps(dim):
    eng = _rvq_engine(dim).engine
    x = rate_rows(dim, seed=1).to(eng.device)
    targets = [200.0, 12.0, INF, 6.0, 20.0]                          # row 0: out of reach; row 2: the best count
    r = _check_rate(eng, x, B, targets)
    # the row built from 2 code vectors is best coded by about 2 stages: a missed target does not send it to the cap
    assert r["ks"][0] < 8 and r["E"][0][r["ks"][0]] == r["E"][0][1:].min()
    assert r["E"][2][r["ks"][2]] == r["E"][2][1:].min()
    f = _check_rate(eng, x, B, targets, min_n_q=3)
    # (behind its own 2 stages that row's curve jumps up and then creeps down to the last stage: the best count from 3 on may be the cap)
    assert min(f["ks"]) >= 3 and f["E"][0][f["ks"][0]] == f["E"][0][3:].min()
    caps = [32, 4, 32, 1, 8]
    c = _check_rate(eng, x, B, targets, caps=caps)
    assert all(k <= cap for k, cap in zip(c["ks"], caps)) and c["ks"][3] == 1 and c["ks"][0] == r["ks"][0] and c["ks"][0] < 8
    with pytest.raises(EngineError, match="min_n_q"):               # the floor above a row's cap
        eng.rvq_encode(x, CAP, n_q_rows=caps, target_snr_db=targets, min_n_q=3)
    eng.check_status()


# ---- 3. with the search over the stages ------------------------------------------------------------------------------------------------
def test_with_rvq_beam_the_rows_take_a_prefix_of_the_full_depth_path():
    m = _rvq_engine(16)
    eng = m.engine
    x = rate_rows(16, seed=2).to(eng.device)
    g = _check_rate(eng, x, B, 12.0)
    s = _check_rate(eng, x, B, 12.0, beam=4)
    tok = s["codes"].reshape(CAP, B, TF).permute(1, 2, 0).contiguous()
    _, emb = eng.decode_codes(tok, n_q_rows=s["ks"])
    assert torch.equal(s["quant"].reshape(B, TF, 16), emb)
    assert bool((s["serr"][CAP] <= g["serr"][CAP]).all()), "the search codes no frame worse than greedy"
    print(f"k greedy {g['ks']} k rvq_beam 4 {s['ks']}")
    eng.check_status()


# ---- 4. isolation ----------------------------------------------------------------------------------------------------------------------
def test_nan_rows_take_their_cap_and_leave_the_others_unchanged():
    eng = _rvq_engine(128).engine
    x = rate_rows(128, seed=3).to(eng.device)
    caps = [32, 9, 5, 32, 32]
    clean = _check_rate(eng, x, B, 12.0, caps=caps)
    bad = x.clone()
    for b in (0, 2, 4):
        bad[b * TF:(b + 1) * TF] = NAN
    codes, quant, rate = eng.rvq_encode(bad, CAP, n_q_rows=caps, target_snr_db=12.0)
    ks = rate["n_q_rows"].tolist()
    for b in (1, 3):
        rows = slice(b * TF, (b + 1) * TF)
        assert ks[b] == clean["ks"][b]
        assert torch.equal(codes[:, rows], clean["codes"][:, rows]) and torch.equal(quant[rows], clean["quant"][rows])
        assert torch.equal(rate["stage_errors"][:, b], clean["serr"][:, b])
        assert np.array_equal(rate["row_errors"][b].cpu().numpy(), clean["E"][b])
    for b in (0, 2, 4):
        assert ks[b] == caps[b]
    eng.check_status()


def test_a_row_gets_the_same_count_and_bits_wherever_it_stands():
    eng = _rvq_engine(64).engine
    x = rate_rows(64, seed=4).to(eng.device).reshape(B, TF, 64)
    row = x[2:3]
    others = x[[0, 1, 3, 4]]
    alone = eng.rvq_encode(row.reshape(-1, 64), CAP, target_snr_db=[12.0])
    first = eng.rvq_encode(torch.cat([row, others]).reshape(-1, 64), CAP, target_snr_db=[12.0, 3.0, 40.0, 6.0, INF])
    last = eng.rvq_encode(torch.cat([others, row]).reshape(-1, 64), CAP, target_snr_db=[3.0, 40.0, 6.0, INF, 12.0])
    for (codes, quant, rate), b in ((first, 0), (last, 4)):
        rows = slice(b * TF, (b + 1) * TF)
        assert int(rate["n_q_rows"][b]) == int(alone[2]["n_q_rows"][0])
        assert torch.equal(codes[:, rows], alone[0]) and torch.equal(quant[rows], alone[1])
        assert torch.equal(rate["row_errors"][b], alone[2]["row_errors"][0]) and torch.equal(rate["stage_errors"][:, b], alone[2]["stage_errors"][:, 0])
    assert 1 < int(alone[2]["n_q_rows"][0]) < CAP
    eng.check_status()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
def _same_as_bit_width(m, wav, targets, **kw):
    """inference with targets against a second call with the bit widths of the returned counts"""
    r = m.inference(wav, target_snr_db=targets, **kw)
    ks = r["n_q_rows"].tolist()
    cap = m.arch.num_quantizers
    assert r["n_q_rows"].dtype == torch.int32 and r["row_snr_db"].dtype == torch.float64 and len(ks) == wav.shape[0]
    assert all(1 <= k <= cap for k in ks)
    s = m.inference(wav, bit_width=[k * BW for k in ks], **kw)
    assert "n_q_rows" not in s
    codes = r["code_indices"][0]
    assert codes.shape[0] == cap                                        # the shape of the call at the cap, zeros behind a row's count
    top = max(ks)
    assert torch.equal(codes[:top], s["code_indices"][0]) and int(codes[top:].abs().sum()) == 0
    assert torch.equal(r["code_embeddings"][0][0], s["code_embeddings"][0][0])
    assert torch.equal(r["sub_quants"][0][:top], s["sub_quants"][0]) and float(r["sub_quants"][0][top:].abs().sum()) == 0.0
    if kw.get("need_recon", True):
        assert torch.equal(r["recon_speech"], s["recon_speech"])
    else:
        assert r["recon_speech"] is None
    return r, ks


def _engine_pick_matches(m, wav, targets, lengths=None):
    """the engine call's own outputs: the device's pick is rate_pick of the device's row errors, off every threshold"""
    cap = m.arch.num_quantizers
    e = m.engine.encode(wav, cap, target_snr_db=targets, lengths=lengths, want_stage_errors=True)
    E = e["row_errors"].cpu().numpy()
    ratios = rate_targets(m.arch, targets, wav.shape[0])
    margin = _margin(E, ratios, [cap] * wav.shape[0])
    print(f"k = {e['n_q_rows'].tolist()}, margin {margin:.3e}")
    assert margin >= 1e-6
    assert e["n_q_rows"].tolist() == [rate_pick(E[b], ratios[b], 1, cap) for b in range(wav.shape[0])]
    frames = [wav.shape[-1]] * wav.shape[0] if lengths is None else list(lengths)
    for b, n in enumerate(frames):
        f = m.engine.frames(int(n))
        se = e["stage_errors"][:, b].double().cpu().numpy()
        np.testing.assert_allclose(E[b], se[:, :f].sum(-1), rtol=1e-12, atol=0)
        assert float(np.abs(se[:, f:]).sum()) == 0.0
    return e["n_q_rows"].tolist()


def test_inference_with_targets_equals_inference_with_the_chosen_bit_widths():
    m = engine_for("tiny", 5, 0.8)
    wav = audio(3, 3003, 760, "tones")
    targets = [2.0, 6.0, INF]
    r, ks = _same_as_bit_width(m, wav, targets)
    assert ks == _engine_pick_matches(m, wav, targets)
    snr = r["row_snr_db"].tolist()
    assert all(np.isfinite(snr)) and (ks[0] == 6 or snr[0] >= 2.0)
    _same_as_bit_width(m, wav, targets, need_recon=False)
    e = m.inference_encoding(wav, target_snr_db=targets)
    assert e["n_q_rows"].tolist() == ks and torch.equal(e["code_indices"][0], r["code_indices"][0])
    # a bit width per row is the cap per row
    c = m.inference(wav, target_snr_db=INF, bit_width=[2 * BW, 6 * BW, 3 * BW])
    assert all(k <= cap for k, cap in zip(c["n_q_rows"].tolist(), (2, 6, 3)))
    # the targets are sliced with the micro-batches of a wide call
    whole, m.engine.micro_batch = m.engine.micro_batch, 2
    try:
        p = m.inference(wav, target_snr_db=targets)
    finally:
        m.engine.micro_batch = whole
    assert p["n_q_rows"].tolist() == ks and torch.equal(p["code_indices"][0], r["code_indices"][0])
    assert torch.equal(p["recon_speech"], r["recon_speech"]) and torch.equal(p["row_snr_db"], r["row_snr_db"])
    m.engine.check_status()


def test_inference_with_targets_and_lengths():
    m = engine_for("tiny", 5, 0.8)
    hop = m.engine.hop_length
    T = 3003
    lens = [T, T - 7 * hop - 3, T - 100 * hop]
    wav = audio(3, T, 761, "tones").clone()
    for b, n in enumerate(lens):
        wav[b, n:] = NAN                                             # never read
    targets = [2.0, 6.0, INF]
    r, ks = _same_as_bit_width(m, wav, targets, speech_lengths=torch.tensor(lens))
    assert ks == _engine_pick_matches(m, wav, targets, lens)
    for b, n in enumerate(lens):                                     # a row is the row alone: its count too
        one = m.inference(wav[b:b + 1, :n], target_snr_db=targets[b], speech_lengths=[n])
        assert one["n_q_rows"].tolist() == [ks[b]]
        f = m.engine.frames(n)
        assert torch.equal(one["code_indices"][0][:, 0], r["code_indices"][0][:, b, :f])
    m.engine.check_status()


def test_freq_codec_with_targets():
    from helpers import freq_engine_for
    m = freq_engine_for("tinyfreq", 3)
    wav = audio(3, 1777, 762, "tones")
    cap = m.arch.num_quantizers
    r = m.engine.encode_decode(wav, cap, target_snr_db=[1.0, INF, 3.0])
    ks = r["n_q_rows"].tolist()
    s = m.engine.encode_decode(wav, cap, n_q_rows=ks)
    for key in ("codes", "quantized", "sub_quants", "recon"):
        assert torch.equal(r[key], s[key]), key
    E = r["row_errors"].cpu().numpy()
    ratios = rate_targets(m.arch, [1.0, INF, 3.0], 3)
    assert _margin(E, ratios, [cap] * 3) >= 1e-6 and ks == [rate_pick(E[b], ratios[b], 1, cap) for b in range(3)]
    m.engine.check_status()


# ---- 6. leaves no trace ----------------------------------------------------------------------------------------------------------------
def test_a_plain_call_after_a_rate_call_is_untouched():
    m = engine_for("tiny", 5, 0.8)
    wav = audio(3, 23 * m.engine.hop_length + 3, 763, "tones")
    before = m.inference(wav)
    m.inference(wav, target_snr_db=[1.0, 4.0, INF], min_n_q=2)
    with pytest.raises(EngineError):                                 # a refused call leaves no rate behind either
        m.engine.encode(wav, 6, n_q_rows=[1, 2, 3], target_snr_db=3.0, min_n_q=2)
    after = m.inference(wav[:2])                                      # another batch width is fine again
    again = m.inference(wav)
    for a, b in ((again, before), (after, m.inference(wav[:2]))):
        assert torch.equal(a["code_indices"][0], b["code_indices"][0]) and torch.equal(a["recon_speech"], b["recon_speech"])
        assert torch.equal(a["code_embeddings"][0][0], b["code_embeddings"][0][0]) and torch.equal(a["sub_quants"][0], b["sub_quants"][0])
    assert torch.equal(after["code_indices"][0], before["code_indices"][0][:, :2])
    m.engine.check_status()


def test_engine_refuses_a_rate_that_does_not_fit_before_any_launch():
    """the C side's own rules: refused before the first launch, nothing is left behind"""
    import ctypes as C
    m = engine_for("tiny", 5, 0.8)
    eng, lib = m.engine, m.engine.lib
    wav = audio(3, 331, 765, "tones")
    before = eng.encode(wav, 6)
    out = torch.zeros(3, dtype=torch.int32, device=eng.device)

    def set_rate(ratios, min_nq=1, n_q_out=out):
        return lib.fc_engine_set_rate(eng._h, (C.c_double * len(ratios))(*ratios), len(ratios), min_nq,
                                      None if n_q_out is None else C.c_void_p(n_q_out.data_ptr()), None, None, eng._stream())
    for ratios, min_nq, n_q_out, word in (([0.1, -0.5, 0.1], 1, out, "negative"), ([0.1, NAN, 0.1], 1, out, "NaN"), ([0.1] * 3, 0, out, "min_nq"),
                                          ([0.1] * 3, 7, out, "min_nq"), ([0.1] * 3, 1, None, "n_q_rows_out")):
        assert set_rate(ratios, min_nq, n_q_out) != 0 and word in lib.fc_last_error().decode(), word
    with eng._rate([0.1, 0.1], 1, 6, eng.frames(331)):               # another batch width
        with pytest.raises(EngineError, match="a rate is set for 2 rows"):
            eng.encode(wav, 6)
    with eng._rate([0.1] * 3, 4, 6, eng.frames(331)):                # the floor above the call's n_q, and above a row's cap
        with pytest.raises(EngineError, match="min_nq = 4 lies above n_q = 3"):
            eng.encode(wav, 3)
        with eng._row_nq([6, 2, 6]):
            with pytest.raises(EngineError, match="above the cap of row 1"):
                eng.encode(wav, 6)
    with eng._rate([0.1] * 3, 1, 6, eng.frames(331)):                # the hook wants both error outputs: it has no workspace
        x = torch.zeros(6, 16, device=eng.device)
        codes = torch.zeros(6, 6, dtype=torch.int64, device=eng.device)
        assert lib.fc_rvq_encode_rate(eng._h, C.c_void_p(x.data_ptr()), 6, 6, 1, C.c_void_p(codes.data_ptr()), None, eng._stream()) != 0
        assert "stage_errors_out" in lib.fc_last_error().decode()
    after = eng.encode(wav, 6)
    assert int(out.abs().sum()) == 0 and "n_q_rows" not in after
    assert torch.equal(after["codes"], before["codes"]) and torch.equal(after["quantized"], before["quantized"])
    eng.check_status()


def test_a_session_push_is_refused_by_name_while_a_rate_is_set():
    m = engine_for("tinyss", 5)
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    st = m.open_stream(2)
    slots = m.open_slots(2)
    slots.start(0)
    n = max(st.min_first_samples, slots.min_first_samples, 8 * hop) // hop * hop
    wav = audio(2, n, 764, "tones").to(m.device)
    with m.engine._rate([0.1, 0.1], 1, cap, n // hop):
        with pytest.raises(EngineError, match="offline calls only"):
            st.encode(wav)
        with pytest.raises(EngineError, match="offline calls only"):
            slots.encode({0: (wav[0], False)})
    st.reset()                                                        # (the host side of the session had counted the refused push)
    codes, _ = st.encode(wav)                                         # cleared: the push goes through
    assert codes.shape[-1] == n // hop
    m.engine.check_status()
