"""The identities that let one kernel serve a stage count per row and a stage count per frame (StageCounts, csrc/ragged_kernels.h;
csrc/rvq_rate_kernels.h states the rules), on the MI355X, bit for bit: a count per frame that repeats its row's count is the count per
row, in the decode and in the encode, and the two ends of the target scale are calls with a plain table.

Shapes: D in {16, 128, 256} are the three block sizes of the sum and decode kernels; B = 3 rows of 1, 5 and 257 frames -- 257 crosses
the 256-thread blocks of the zero kernel off a row boundary and the 256 partial sums of the picks; 64 codes, n_q = 4."""
import numpy as np
import pytest
import torch

from funcodec_amd.synth import make_state_dict
from helpers import audio
from test_rvq_rate_gpu import _arch, _codebooks, _rvq_engine

pytestmark = pytest.mark.gpu
INF = float("inf")
B, NQ = 3, 4
DIMS = (16, 128, 256)
FRAMES = (1, 5, 257)
GARBAGE = (-1, (1 << 40) + 5)


def _tokens(eng, Tf, seed):
    g = torch.Generator().manual_seed(100 + seed)
    return torch.randint(0, eng.arch.codebook_size, (B, Tf, NQ), generator=g).to(eng.device)


def _lengths(Tf):
    return [max(1, n) for n in (1, Tf - 1, Tf)]


@pytest.mark.parametrize("Tf", FRAMES)
@pytest.mark.parametrize("dim", DIMS)
def test_decode_with_a_rows_count_in_every_frame_is_the_decode_with_a_count_per_row(dim, Tf):
    eng = _rvq_engine(dim).engine
    tok = _tokens(eng, Tf, dim + Tf)
    rows = [2, NQ, 1]
    kf = torch.tensor(rows, dtype=torch.int32, device=eng.device)[:, None].expand(B, Tf).contiguous()
    behind = torch.arange(NQ, device=eng.device)[None, None, :] >= kf[:, :, None]
    for lengths in (None, _lengths(Tf)):
        wav_r, emb_r = eng.decode_codes(tok, lengths=lengths, n_q_rows=rows)
        wav_f, emb_f = eng.decode_codes(tok, lengths=lengths, n_q_frames=kf)
        assert torch.equal(wav_f, wav_r) and torch.equal(emb_f, emb_r), lengths
        for g in GARBAGE:                              # out-of-range codes behind the counts: neither call reads or reports them
            dirty = torch.where(behind, torch.full_like(tok, g), tok)
            for kw in (dict(n_q_rows=rows), dict(n_q_frames=kf)):
                wav_d, emb_d = eng.decode_codes(dirty, lengths=lengths, **kw)
                assert torch.equal(wav_d, wav_r) and torch.equal(emb_d, emb_r), (lengths, g, kw.keys())
                eng.check_status()                     # no FC_STATUS_BAD_CODE


@pytest.mark.parametrize("Tf", FRAMES)
@pytest.mark.parametrize("dim", DIMS)
def test_encode_where_every_frame_takes_the_floor_is_the_encode_with_that_count_per_row(dim, Tf):
    eng = _rvq_engine(dim).engine
    wav = audio(B, Tf * eng.hop_length, 900 + Tf, "tones")
    assert eng.frames(wav.shape[-1]) == Tf
    for f in (1, NQ):
        frame = eng.encode(wav, NQ, target_snr_db=-INF, min_n_q=f, per_frame=True)
        row = eng.encode(wav, NQ, n_q_rows=[f] * B)
        assert frame["n_q_frames"].tolist() == [[f] * Tf] * B
        for key in ("codes", "quantized", "sub_quants"):
            assert torch.equal(frame[key], row[key]), (f, key)
    zero = eng.encode(wav, NQ, target_snr_db=-INF, min_n_q=0, per_frame=True)
    assert int(zero["n_q_frames"].abs().sum()) == 0 and zero["n_codes_rows"].tolist() == [0] * B
    assert not zero["codes"].any() and not zero["sub_quants"].any()
    if dim == eng.arch.dimension:
        assert not zero["quantized"].any()
    else:       # the quantised sum is 0 in the codebooks' space; the returned rows are its output projection: one row, the bias, everywhere
        q = zero["quantized"].reshape(B * Tf, -1)
        bias = torch.from_numpy(make_state_dict(_arch(dim), 7, 0.8)["quantizer.output_proj.bias"]).to(q)      # _rvq_engine's checkpoint
        assert torch.equal(q, bias[None, :].expand_as(q))
    eng.check_status()


def _code_sums(dim, Tf):
    """[B * Tf, dim] float32: every frame is the sum of one random code vector of each of the NQ stages plus 0.02 N(0, 1), so a stage
    more lowers a row's error: "the best k" of a target of +inf is the cap.  (Checked on the CPU with a numpy greedy quantiser for
    every shape below: each row's curve falls to its cap.)"""
    rng = np.random.default_rng(5000 + 31 * dim + 7 * Tf)
    cb = _codebooks(dim)[:NQ]
    idx = rng.integers(0, cb.shape[1], (B * Tf, NQ))
    x = cb[np.arange(NQ)[None, :], idx].astype(np.float64).sum(1) + 0.02 * rng.standard_normal((B * Tf, dim))
    return torch.from_numpy(x.astype(np.float32))


@pytest.mark.parametrize("beam", [1, 4])
@pytest.mark.parametrize("Tf", FRAMES)
@pytest.mark.parametrize("dim", DIMS)
def test_the_two_ends_of_the_target_scale_are_calls_with_a_table(dim, Tf, beam):
    eng = _rvq_engine(dim).engine
    x = _code_sums(dim, Tf).to(eng.device)
    caps, floor = [NQ, 2, 3], 2
    for target, rows in ((INF, caps), (-INF, [min(floor, c) for c in caps])):
        codes, quant, rate = eng.rvq_encode(x, NQ, n_q_rows=caps, beam=beam, target_snr_db=target, min_n_q=floor)
        assert rate["n_q_rows"].tolist() == rows, (target, rate["row_errors"].tolist())
        if beam == 1 or rows == caps:                  # a search over fewer stages is another search: the prefix of the full-depth path
            want_c, want_q = eng.rvq_encode(x, NQ, n_q_rows=rows, beam=beam)
        else:
            full, _ = eng.rvq_encode(x, NQ, n_q_rows=caps, beam=beam)
            k = torch.tensor(rows, device=eng.device).repeat_interleave(Tf)
            want_c = torch.where(torch.arange(NQ, device=eng.device)[:, None] < k[None, :], full, torch.zeros_like(full))
            want_q = None
        assert torch.equal(codes, want_c), target
        assert want_q is None or torch.equal(quant, want_q), target
    eng.check_status()
