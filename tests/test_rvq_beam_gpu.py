"""`-m gpu` tests of the quantiser's search over the stages (csrc/rvq_beam_kernels.h; fc_rvq_encode_beam, fc_engine_set_rvq_beam).

The reference has no such search, so the yardsticks are the specification's own: the guarantee against the greedy codes (which stay the
product's reference-exact ones), float64 scores of every decision from the GPU's own parents, a float64 restatement of the whole search
where nothing is near a tie (tests/test_rvq_beam_host.py), independence of a frame from its neighbours, and, through the engine, the
per-op hook on a call's own encoder output.

Bounds.  tau = 8 D 2^-24 (|r_parent|^2 + max_k |e_k|^2) bounds the fp32 expansion (|r|^2 - 2 r.e) + |e|^2 of a candidate's score; the
float64 recomputation of an error from the codes allows the rounding of a D-term fp32 sum, 2 D 2^-24 relative."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from funcodec_amd.engine import EngineError
from helpers import audio, engine_for, freq_engine_for, rms
from test_gpu_parity import WAV_RMS_TOL
from test_rvq_beam_host import beam_arch, beam_ref64, beam_rows, beam_state, tau

pytestmark = pytest.mark.gpu
NAN = float("nan")
SHAPES = [(16, 64), (128, 1024), (512, 64)]        # (D, K): the tiny fixture, a full-width quantiser, the widest rows a fixture has
WIDTHS = [2, 4, 8]


@functools.lru_cache(maxsize=None)
def _eng(dim, K=64):
    from funcodec_amd.model import EncodecMI355X
    m = EncodecMI355X(beam_arch(dim, K), "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in beam_state(dim, K).items()})
    return m.engine


@functools.lru_cache(maxsize=None)
def _cb(dim, K=64):
    return beam_state(dim, K)["quantizer.rq.model.embed"].astype(np.float64)       # [32, K, D]


def _err64(x, cb, codes):
    """|x - sum_i E_i[codes[i]]|^2 per frame in float64; x [N, D], codes [S, N]"""
    r = x.astype(np.float64).copy()
    for i in range(codes.shape[0]):
        r -= cb[i][codes[i]]
    return (r ** 2).sum(-1)


def _call(eng, x, n_q, W, **kw):
    codes, quant, paths, errors = eng.rvq_encode(x, n_q, beam=W, return_paths=True, **kw)
    return codes.cpu().numpy(), quant.cpu(), paths.cpu().numpy(), errors.cpu().numpy()


# ---- 1. never worse -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("dim,K", SHAPES)
def test_no_frame_is_coded_worse_than_greedy(dim, K, W):
    eng, cb = _eng(dim, K), _cb(dim, K)
    better = total = 0
    for N in (1, 5, 33):
        for n_q in (1, 2, 8, 32):
            x = beam_rows(N, dim, n_q, W)
            x[N // 2] = 0.0                                   # an all-zero frame
            g, gq = eng.rvq_encode(x, n_q)
            codes, quant, paths, errors = _call(eng, x, n_q, W)
            g = g.cpu().numpy()
            assert np.array_equal(paths[0], g), (N, n_q)                              # slot 0 is today's path
            win = np.array([[np.array_equal(paths[s][:, n], codes[:, n]) for s in range(W)].index(True) for n in range(N)])
            ew = errors[win, np.arange(N)]
            assert (ew <= errors[0]).all(), (N, n_q)                                  # exactly, under the kernel's own formula
            live = ~(x == 0).all(1).numpy()
            assert (ew[live] == errors.min(0)[live]).all(), (N, n_q)                  # the smallest error wins
            e_b, e_g = _err64(x.numpy(), cb, codes), _err64(x.numpy(), cb, g)
            assert (e_b <= e_g * (1 + 2 * dim * 2.0 ** -24)).all(), (N, n_q, float((e_b / e_g).max()))
            assert np.array_equal(codes[:, N // 2], g[:, N // 2]), "an all-zero frame keeps its greedy codes"
            if n_q == 1:
                assert np.array_equal(codes, g)
            assert codes.min() >= 0 and codes.max() < K and paths.min() >= 0 and paths.max() < K
            # quantized is the sum of the final codes' vectors in stage order (bit for bit fc_decode_codes' emb_out: test 5)
            q = torch.zeros(N, dim)
            for i in range(n_q):
                q = q + torch.from_numpy(beam_state(dim, K)["quantizer.rq.model.embed"][i][codes[i]])
            assert torch.equal(quant, q), (N, n_q)
            better += int((e_b < e_g).sum()); total += N
    print(f"D {dim} K {K} W {W}: {better} of {total} frames coded better than greedy")
    assert better > 0, "the search never found anything: it is not searching"
    eng.check_status()


# ---- 2. every decision, from the GPU's own parents ------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("dim,K,S", [(16, 64, 8), (128, 1024, 32), (512, 64, 8)])
def test_every_kept_candidate_is_among_the_best_to_within_fp32_rounding(dim, K, S, W):
    """The kept set of stage i is the set of final paths of the call with n_q = i + 1 (the search is deterministic and its stages do not
    look ahead), its parents are those of the call with n_q = i: every stage of every frame is rebuilt, none left out."""
    eng, cb = _eng(dim, K), _cb(dim, K)
    N = 33
    x = beam_rows(N, dim, S, W)
    x64 = x.double().numpy()
    g = eng.rvq_encode(x, S)[0].cpu().numpy()
    parents = np.zeros((1, 0, N), np.int64)                    # one hypothesis in front of stage 0
    e2max = (cb ** 2).sum(-1).max(-1)                          # [32]
    worst = 0.0
    for i in range(S):
        codes, _, paths, errors = _call(eng, x, i + 1, W)
        assert np.array_equal(paths[0], g[:i + 1]), i          # slot 0 follows g
        H = parents.shape[0]
        R = np.repeat(x64[None], H, 0)                         # [H, N, D] the parents' residuals
        for j in range(i):
            R = R - cb[j][parents[:, j, :]]
        r2 = (R ** 2).sum(-1)                                  # [H, N]
        sc = r2[:, :, None] - 2.0 * np.einsum("hnd,kd->hnk", R, cb[i]) + (cb[i] ** 2).sum(-1)[None, None]
        for n in range(N):
            rest = sc[:, n, :].copy()
            rest[0, g[i, n]] = np.inf
            kth = np.sort(rest.ravel())[W - 2]                 # the (W - 1)-th smallest remaining score
            kept = set()
            for s in range(W):
                match = [h for h in range(H) if np.array_equal(parents[h, :, n], paths[s, :i, n])]
                assert match, (i, n, s, "a kept path does not extend a kept path of the stage before")
                h, c = match[0], int(paths[s, i, n])
                kept.add((h, c))
                t = tau(dim, r2[h, n], e2max[i])
                if s > 0:
                    assert (h, c) != (0, int(g[i, n])), (i, n, s)
                    assert sc[h, n, c] <= kth + t, (i, n, s, sc[h, n, c] - kth, t)
                    worst = max(worst, (sc[h, n, c] - kth) / t)
                assert abs(float(errors[s, n]) - sc[h, n, c]) <= t, (i, n, s, float(errors[s, n]), sc[h, n, c], t)
            assert len(kept) == W, (i, n, "a candidate was kept twice")
        parents = paths
    print(f"D {dim} K {K} W {W}: worst (score - k-th best) / tau = {worst:.3g}")
    eng.check_status()


# ---- 3. exact codes where nothing is near a tie ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("n_q", [1, 2, 8])
def test_codes_equal_the_float64_restatement_where_nothing_is_near_a_tie(n_q, W):
    eng, cb = _eng(16), _cb(16)[:n_q]
    N = 33
    x = beam_rows(N, 16, n_q, W)
    g = eng.rvq_encode(x, n_q)[0].cpu().numpy()
    codes, _, paths, errors = _call(eng, x, n_q, W)
    left_out = 0
    for n in range(N):
        ref = beam_ref64(x[n].double().numpy(), cb, W, g=g[:, n])
        if not ref["clear"]:
            left_out += 1
            continue
        assert np.array_equal(codes[:, n], ref["codes"]), (n, codes[:, n], ref["codes"])
        assert {tuple(p) for p in paths[:, :, n]} == {tuple(p) for p in ref["paths"]}, n
    print(f"n_q {n_q} W {W}: {left_out} of {N} frames left out")
    assert left_out <= N // 10


# ---- 4. independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("dim,K", SHAPES)
def test_a_frame_does_not_depend_on_its_neighbours(dim, K, W):
    eng = _eng(dim, K)
    n_q, at = 8, 17
    x = beam_rows(33, dim, n_q, W).to(eng.device)
    alone = eng.rvq_encode(x[at:at + 1], n_q, beam=W, return_paths=True)
    among = eng.rvq_encode(x, n_q, beam=W, return_paths=True)
    bad = torch.full_like(x, NAN)
    bad[at] = x[at]
    poisoned = eng.rvq_encode(bad, n_q, beam=W, return_paths=True)
    for other in (among, poisoned):
        assert torch.equal(other[0][:, at:at + 1], alone[0]) and torch.equal(other[1][at:at + 1], alone[1])
        assert torch.equal(other[2][:, :, at:at + 1], alone[2]) and torch.equal(other[3][:, at:at + 1], alone[3])
    assert int(poisoned[0].min()) >= 0 and int(poisoned[0].max()) < K           # the codes of an all-NaN frame stay in range
    eng.check_status()


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("dim,K,n_q", [(16, 64, 8), (128, 1024, 32), (512, 64, 8)])
def test_a_stage_count_per_row_gives_each_row_the_call_with_that_count(dim, K, n_q, W):
    """3 utterances of 5 frames: a workgroup (16 / W frames) straddles utterances of different counts"""
    eng = _eng(dim, K)
    counts, Tf = [1, 3, n_q], 5
    x = beam_rows(3 * Tf, dim, n_q, W).to(eng.device)
    codes, quant, paths, errors = eng.rvq_encode(x, n_q, n_q_rows=counts, beam=W, return_paths=True)
    for b, k in enumerate(counts):
        rows = slice(b * Tf, (b + 1) * Tf)
        c1, q1, p1, e1 = eng.rvq_encode(x[rows], k, beam=W, return_paths=True)
        assert torch.equal(codes[:k, rows], c1) and torch.equal(quant[rows], q1), (b, k)
        assert torch.equal(paths[:, :k, rows], p1) and torch.equal(errors[:, rows], e1), (b, k)
        if k < n_q:
            assert int(codes[k:, rows].abs().max()) == 0 and int(paths[:, k:, rows].abs().max()) == 0, (b, k)
    eng.check_status()


# ---- 5. through the engine ------------------------------------------------------------------------------------------------------------
def _hook(m, enc, n_q, W, rows=None):
    """the per-op hook on encoder output rows [B, Tf, D] -> codes [n_q, B, Tf]"""
    B, Tf, D = enc.shape
    codes = m.engine.rvq_encode(enc.reshape(B * Tf, D), n_q, beam=W, n_q_rows=rows)[0]
    return codes.view(n_q, B, Tf)


def test_inference_codes_equal_the_hook_and_everything_else_comes_from_them():
    m = engine_for("tiny", 5)
    n_q, T = m.arch.num_quantizers, 1003
    wav = audio(3, T, 77, "tones")
    plain = m.inference(wav, use_scale=False)
    enc = m.engine.encode(wav, n_q, want_enc_out=True)["enc_out"]
    r = m.inference(wav, use_scale=False, rvq_beam=4)
    codes = r["code_indices"][0]
    assert torch.equal(codes, _hook(m, enc, n_q, 4))
    assert not torch.equal(codes, plain["code_indices"][0]), "the width did not reach the quantiser"
    wav2, emb = m.engine.decode_codes(codes.permute(1, 2, 0).contiguous())
    assert torch.equal(r["code_embeddings"][0][0], emb)
    assert torch.equal(r["recon_speech"], wav2[..., :T])
    sq = r["sub_quants"][0]                                   # [n_q, B, D, Tf]: E_i[codes[i]]
    from helpers import state_for
    E = torch.from_numpy(state_for("tiny", 5)[2]["quantizer.rq.model.embed"]).to(sq.device)
    for i in range(n_q):
        assert torch.equal(sq[i], E[i][codes[i]].permute(0, 2, 1)), i
    # inference_encoding, a bit rate per row, and both together with lengths
    assert torch.equal(m.inference_encoding(wav, rvq_beam=4)["code_indices"][0], codes)
    bw = 12000.0
    rows = m.inference(wav, bit_width=[bw, 3 * bw, 6 * bw], rvq_beam=4)["code_indices"][0]
    assert torch.equal(rows, _hook(m, enc, n_q, 4, rows=[1, 3, 6]))
    # default untouched: the engine is as it was
    again = m.inference(wav, use_scale=False)
    assert torch.equal(again["code_indices"][0], plain["code_indices"][0]) and torch.equal(again["sub_quants"][0], plain["sub_quants"][0])
    assert torch.equal(again["code_embeddings"][0][0], plain["code_embeddings"][0][0]) and torch.equal(again["recon_speech"], plain["recon_speech"])
    m.engine.check_status()


def test_a_ragged_row_equals_the_row_alone():
    m = engine_for("tiny", 5)
    T, L = 1003, 613
    wav = audio(2, T, 78, "tones")
    r = m.inference(wav, speech_lengths=[T, L], rvq_beam=4, bit_width=[6 * 12000.0, 2 * 12000.0])
    for b, (n, k) in enumerate(((T, 6), (L, 2))):
        one = m.inference(wav[b:b + 1, :n], rvq_beam=4, bit_width=k * 12000.0)
        Tf = m.engine.frames(n)
        assert torch.equal(r["code_indices"][0][:k, b:b + 1, :Tf], one["code_indices"][0])
        assert torch.equal(r["code_embeddings"][0][0][b:b + 1, :Tf], one["code_embeddings"][0][0])
        # the decoder is not this feature's: its length-aware pass is held to the one-utterance call by the ragged tests' own bar
        assert rms(r["recon_speech"][b:b + 1, :, :n], one["recon_speech"]) < WAV_RMS_TOL
    m.engine.check_status()


def test_streamed_pushes_and_a_slot_push_equal_the_offline_call():
    """a causal fixture.  A frame's codes depend on its encoder output alone, so a push's codes equal the hook on the push's own encoder
    output, and the offline call's wherever the streamed encoder output equals the offline one bit for bit (which is recorded)."""
    from test_stream_gpu import pushes, stream_encode
    m = engine_for("tinywn", 5)
    hop, n_q, W = m.engine.hop_length, m.arch.num_quantizers, 4
    T = 40 * hop + 3
    wav = audio(2, T, 79, "tones")
    with m.engine._rvq_beam(W):
        off = m.engine.encode(wav, n_q, want_enc_out=True)
    assert torch.equal(off["codes"], _hook(m, off["enc_out"], n_q, W))
    for how in ("mixed", "single"):
        codes, quant, enc, _ = stream_encode(m.open_stream(2, scale=off["scale"], rvq_beam=W), wav, pushes(T, hop, how))
        assert torch.equal(codes, _hook(m, enc, n_q, W)), how
        same = (enc == off["enc_out"]).all(-1)                                        # [B, Tf]
        assert torch.equal(codes.permute(1, 2, 0)[same], off["codes"].permute(1, 2, 0)[same]), how
        print(f"stream [{how}]: {int(same.sum())} of {same.numel()} frames have the offline call's encoder output bit for bit")
        emb = m.engine.decode_codes(codes.permute(1, 2, 0).contiguous())[1]
        assert torch.equal(quant, emb), how
    st = m.open_slots(3, rvq_beam=W)
    st.start(1, scale=float(off["scale"][0]))
    c, q, e = st.encode({1: (wav[0], True)}, want_enc_out=True)[1]
    assert torch.equal(c, _hook(m, e[None], n_q, W)[:, 0])
    same = (e == off["enc_out"][0]).all(-1)
    assert torch.equal(c.t()[same], off["codes"][:, 0].t()[same])
    plain = m.open_slots(3)
    plain.start(1, scale=float(off["scale"][0]))
    assert not torch.equal(plain.encode({1: (wav[0], True)})[1][0], c), "the width did not reach the slot push"
    m.engine.check_status()


def test_freqcodec_encode():
    m = freq_engine_for("tinyfreq", 3)
    n_q = m.arch.num_quantizers
    wav = audio(2, 4000, 80, "tones")
    enc = m.engine.encode(wav, n_q, want_enc_out=True)["enc_out"]
    r = m.inference(wav, rvq_beam=4)
    codes = r["code_indices"][0]
    assert torch.equal(codes, _hook(m, enc, n_q, 4))
    assert not torch.equal(codes, m.inference(wav)["code_indices"][0])
    assert torch.equal(r["code_embeddings"][0][0], m.engine.decode_codes(codes.permute(1, 2, 0).contiguous())[1])
    m.engine.check_status()


def test_the_width_is_part_of_a_captured_pushs_key():
    m = engine_for("tinywn", 5)
    hop, B = m.engine.hop_length, 2
    wav = audio(B, 30 * hop, 81, "tones")

    def run(st):
        out, stats = [st.encode(wav[..., :12 * hop])], []           # the first push of an utterance: a one-off
        for i in range(12, 30):
            st.rvq_beam = 1 if 16 <= i < 22 else 4
            out.append(st.encode(wav[..., i * hop:(i + 1) * hop]))
            stats.append(st.graph_stats())
        return out, stats
    eo, _ = run(m.open_stream(B, rvq_beam=4))
    go, stats = run(m.open_stream(B, rvq_beam=4, graph=True))
    for a, b in zip(eo, go):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    caps = [s["captures"] for s in stats]
    print("captures after each push:", caps)
    # pushes 12 .. 15 with width 4: two parities -> 2 captures; 16 .. 21 with width 1: 2 more; 22 on with width 4 again: none
    assert caps[3] == 2 and caps[5] == 4 and caps[9] == 4 and caps[-1] == 4, caps
    assert stats[-1]["replays"] == len(stats) - 4 and stats[-1]["fallbacks"] == 0
    m.engine.check_status()


# ---- 6. default untouched, and the library's own refusals -----------------------------------------------------------------------------
def test_after_the_width_is_cleared_a_call_equals_a_fresh_engines():
    from funcodec_amd.model import EncodecMI355X
    from helpers import state_for
    cfg, arch, sd = state_for("tiny", 5)
    wav = audio(2, 1003, 82, "tones")

    def fresh():
        m = EncodecMI355X(arch, "cuda:0")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m
    a, b = fresh(), fresh()
    a.engine.set_rvq_beam(4)
    a.engine.set_rvq_beam(1)
    ra, rb = a.engine.encode_decode(wav, 6), b.engine.encode_decode(wav, 6)
    for k in ("codes", "quantized", "sub_quants", "scale", "recon"):
        assert torch.equal(ra[k], rb[k]), k
    a.engine.set_rvq_beam(4)
    assert not torch.equal(a.engine.encode_decode(wav, 6)["codes"], rb["codes"])
    a.engine.set_rvq_beam(None)
    assert torch.equal(a.engine.encode(wav, 6)["codes"], rb["codes"])


def test_the_library_refuses_by_name_and_changes_nothing():
    import copy
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.model import EncodecMI355X
    from funcodec_amd.synth import make_state_dict
    eng = _eng(16)
    lib, h = eng.lib, eng._h
    x = beam_rows(5, 16, 4, 4).to(eng.device)
    eng.set_rvq_beam(4)
    try:
        for w in (0, 3, 16, -1):
            assert lib.fc_engine_set_rvq_beam(h, w, None) != 0 and b"rvq_beam" in lib.fc_last_error(), w
        codes = torch.full((4, 5), -7, dtype=torch.int64, device=eng.device)
        assert lib.fc_rvq_encode_beam(h, C.c_void_p(x.data_ptr()), 5, 4, 3, C.c_void_p(codes.data_ptr()), None, None, None, eng._stream()) != 0
        assert b"rvq_beam" in lib.fc_last_error()
        torch.cuda.synchronize()
        assert int((codes != -7).sum()) == 0                  # nothing was launched
    finally:
        eng.set_rvq_beam(1)
    arch = arch_from_config(recipe_config("tinyq0"))
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(arch, 5).items()})
    assert m.engine.lib.fc_engine_set_rvq_beam(m.engine._h, 4, None) != 0 and b"quantizer_conf.q0_ds_ratio" in m.engine.lib.fc_last_error()
    assert m.engine.lib.fc_engine_set_rvq_beam(m.engine._h, 1, None) == 0
    with pytest.raises(EngineError, match="q0_ds_ratio"):
        m.inference(torch.zeros(1, 640), rvq_beam=2)
