"""`-m gpu` tests of slot sessions of a causal transformer net (``open_slots(..., max_frames=N)``, fc_seqslots_*, the row-wise kernels of
csrc/seqstream_kernels.hip): every slot at its own position of its own key / value cache.  The yardsticks are float64 on every slot's
utterance alone (the stage) and the real reference's fixture (end to end); between sessions the comparison is bit for bit.

A row of at most kSeqCachedSplitMaxQueries = 16 frames takes the split form (seq_attn_cached_units(n_b, pos_b) waves and a merge), a
longer one the many-query form; ROUNDS (tests/test_seqslots_host.py) mixes both with idle rows in one push, and LONG reaches the cap of
16 units (past 528 cached frames) beside a row that has just started.
"""

import numpy as np
import pytest
import torch

from conftest import record_report
from helpers import audio, golden, index_report, rms
from test_gpu_parity import WAV_RMS_TOL, _assert_flips_are_near_ties, _prefix_before
from test_seq_transformer_gpu import BLOCK_ABS_TOL, BLOCK_RMS_TOL, MAN, _block_engine, _engine, transformer_f64
from test_seqslots_host import ROUNDS, ROUNDS_MAX_FRAMES, utterances
from test_seqstream_gpu import _tiny
from test_slots_gpu import Utt, drive
from test_stream_gpu import pushes

from funcodec_amd.engine import EngineError

pytestmark = pytest.mark.gpu
NAN = float("nan")
# slot 0: 500, 24, then 1-frame pushes to 532 frames (16 units of 3 tiles from 529 on); slot 1 starts late with 7 and runs beside it
LONG = [(-500, 0), (24, 0), (1, -7)] + [(1, 1)] * 7
LONG_MAX_FRAMES = 532


def _inputs(C, rounds, seed):
    """per slot, per utterance: x [C, T] on the device, seeded by (C, slot, utterance) alone"""
    return [[torch.randn(C, sum(u), generator=torch.Generator().manual_seed(seed + C * 7919 + 100 * slot + k)).cuda() for k, u in enumerate(per)]
            for slot, per in enumerate(utterances(rounds))]


def run_rounds(st, xs, rounds, decoder=False, pad=0.0, only=None):
    """Push `rounds` through the stage hook: per slot, per utterance, the outputs of its pushes joined [C, T].  Behind every row's count
    and in idle rows the input holds `pad` and the output must be exactly 0.  only: the one slot of `rounds` that a 1-slot session runs."""
    S, C = st.slots, xs[0][0].shape[0]
    slots = range(S) if only is None else [only]
    outs = [[[] for _ in per] for per in xs]
    at = [[-1, 0] for _ in xs]                             # per slot: utterance index, frames of it pushed
    for row in rounds:
        row = [row[s] for s in slots]
        T = max(abs(n) for n in row)
        if T == 0:
            continue
        x = torch.full((S, C, T), pad, device="cuda")
        for i, (s, n) in enumerate(zip(slots, row)):
            if n < 0:
                at[s] = [at[s][0] + 1, 0]
            k, pos = at[s]
            x[i, :, :abs(n)] = xs[s][k][:, pos:pos + abs(n)]
        y = st.seq_forward(x, [abs(n) for n in row], [n < 0 for n in row], decoder=decoder)
        for i, (s, n) in enumerate(zip(slots, row)):
            assert bool((y[i, :, abs(n):] == 0).all()), (s, n)
            if n:
                outs[s][at[s][0]].append(y[i, :, :abs(n)].clone())
                at[s][1] += abs(n)
    return [[torch.cat(parts, -1) if parts else None for parts in per] for per in outs]      # None: an utterance of a slot that did not run


def _against_f64(tag, C, rounds, max_frames, decoder=False):
    m, sd, prefix, arch = _block_engine(C, True)
    if decoder:
        prefix = [k[: -len(".after_norm.weight")] for k in sd if k.startswith("decoder.") and k.endswith(".after_norm.weight")][0]
    xs = _inputs(C, rounds, 1)
    st = m.open_slots(len(rounds[0]), max_frames=max_frames)
    ys = run_rounds(st, xs, rounds, decoder)
    worst = [0.0, 0.0]
    for slot, (xper, yper) in enumerate(zip(xs, ys)):
        for k, (x, y) in enumerate(zip(xper, yper)):
            ref = transformer_f64(x.cpu()[None], sd, prefix, arch.lstm_layers, True, False)[0]
            d = y.cpu().double() - ref
            e_max, e_rms = float(d.abs().max()), float(d.pow(2).mean().sqrt())
            print(f"seqslots stage {tag} C={C} slot {slot} utterance {k} T={x.shape[-1]}: max abs {e_max:.3e}, rms {e_rms:.3e}")
            assert bool(torch.isfinite(y).all())
            assert e_max < BLOCK_ABS_TOL and e_rms < BLOCK_RMS_TOL, (C, slot, k, e_max, e_rms)
            worst = [max(worst[0], e_max), max(worst[1], e_rms)]
    record_report("seqslots_stage", schedule=tag, C=C, decoder=decoder, worst_max_abs=worst[0], worst_rms=worst[1])
    m.engine.check_status()


# ---- 1. the stage against float64 on every slot's utterance alone ---------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128, 256, 512, 1024])
def test_slot_stage_against_float64(C):
    _against_f64("rounds", C, ROUNDS, ROUNDS_MAX_FRAMES)       # slot 3 ends exactly at the bound, 66: not a multiple of 16


@pytest.mark.parametrize("C", [64, 512])
def test_slot_stage_against_float64_long(C):
    _against_f64("long", C, LONG, LONG_MAX_FRAMES)


def test_slot_stage_against_float64_decoder_side():
    _against_f64("rounds", 128, ROUNDS, ROUNDS_MAX_FRAMES, decoder=True)


# ---- 2. bit for bit ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(x, y) for pa, pb in zip(a, b) for x, y in zip(pa, pb)) and [len(p) for p in a] == [len(p) for p in b]


def test_replay_one_slot_sessions_a_dirty_state_and_nan_behind_the_counts_bit_for_bit():
    C, S = 256, 4
    m, sd, prefix, arch = _block_engine(C, True)
    xs = _inputs(C, ROUNDS, 2)
    st = m.open_slots(S, max_frames=ROUNDS_MAX_FRAMES)
    first = run_rounds(st, xs, ROUNDS)
    assert all(bool(torch.isfinite(y).all()) for per in first for y in per)
    assert _same(run_rounds(st, xs, ROUNDS), first)            # every slot restarted (START) over what the first run left in its cache
    for slot in range(S):                                      # a slot's result depends neither on S nor on the width of the push
        one = m.open_slots(1, max_frames=ROUNDS_MAX_FRAMES)
        got = run_rounds(one, xs, ROUNDS, only=slot)
        assert _same([got[slot]], [first[slot]]), slot
    # NaN in every float of the state: a frame is written before it is read and loads are clamped.  The stage reads nothing else of the
    # state (the slots' scales, which create writes, belong to the convs), so filling after create covers all it can see.
    dirty = m.open_slots(S, max_frames=ROUNDS_MAX_FRAMES)
    dirty.state.fill_(0xFF)
    got = run_rounds(dirty, xs, ROUNDS)
    assert all(bool(torch.isfinite(y).all()) for per in got for y in per) and _same(got, first)
    # NaN in the input behind every row's count and in idle rows
    got = run_rounds(m.open_slots(S, max_frames=ROUNDS_MAX_FRAMES), xs, ROUNDS, pad=NAN)
    assert all(bool(torch.isfinite(y).all()) for per in got for y in per) and _same(got, first)
    m.engine.check_status()


# ---- 3. against the lock-step stream with the same pushes -----------------------------------------------------------------------------
def test_a_slots_stage_against_a_one_row_stream_with_the_same_pushes():
    C = 256
    m, sd, prefix, arch = _block_engine(C, True)
    xs = _inputs(C, ROUNDS, 3)
    ys = run_rounds(m.open_slots(4, max_frames=ROUNDS_MAX_FRAMES), xs, ROUNDS)
    equal, worst = True, 0.0
    for slot, per in enumerate(utterances()):
        for k, sched in enumerate(per):
            cs = m.open_stream(1, max_frames=ROUNDS_MAX_FRAMES)
            x, pos, parts = xs[slot][k], 0, []
            for n in sched:
                parts.append(cs.seq_forward(x[None, :, pos:pos + n].contiguous())[0])
                pos += n
            via = torch.cat(parts, -1)
            ref = transformer_f64(x.cpu()[None], sd, prefix, arch.lstm_layers, True, False)[0]
            for y in (ys[slot][k], via):
                d = y.cpu().double() - ref
                assert float(d.abs().max()) < BLOCK_ABS_TOL and float(d.pow(2).mean().sqrt()) < BLOCK_RMS_TOL, (slot, k)
            equal = equal and bool(torch.equal(via, ys[slot][k]))
            worst = max(worst, float((via - ys[slot][k]).abs().max()))
    # recorded, not asserted: the same tile loop and the same split, so the bits should agree
    record_report("seqslots_vs_stream", stage_C=C, stage_equal=equal, stage_max_abs=worst)


# ---- 4. end to end against the real reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["frames1", "mixed"])
def test_golden_rows_in_slots_0_and_2_three_pushes_apart(how):
    name = "ss320tfc_b2_t16000"
    c = MAN["cases"][name]
    m, sd = _engine(c["config"], c["weight_seed"])
    arch, hop, T, nq = m.arch, m.engine.hop_length, c["samples"], c["n_q"]
    wav = audio(c["batch"], T, c["audio_seed"], c["audio_kind"])
    g = golden(name)
    scale = g["scale"].reshape(-1)
    us = [Utt(wav[b:b + 1], float(scale[b]), pushes(T, hop, how)) for b in range(2)]
    st = m.open_slots(3, n_q=nq, max_frames=c["frames"])
    drive(st, [[(us[0], None)], [], [3, (us[1], None)]], emb=m.open_slots(3, n_q=nq, max_frames=c["frames"]))
    assert arch.codebook_dim == arch.dimension
    for b, u in enumerate(us):
        codes, quant, enc, rec = u.cat()
        rec, rec_e = rec[..., :T], torch.cat(u.rec_e, -1)[..., :T]
        ref_idx, ref_enc, ref_quant, ref_recon = g["indices"][:, b:b + 1].astype(np.int64), g["encoder_out"][b:b + 1], g["quantized"][b:b + 1], g["recon"][b:b + 1]
        assert codes.shape[-1] == ref_idx.shape[2] == m.engine.frames(T)
        e_enc, e_wav, e_wav_e = rms(enc[None], ref_enc), rms(rec[None], ref_recon), rms(rec_e[None], ref_recon)
        rep = index_report(codes[:, None], ref_idx)
        print(f"{name} [{how}] row {b} in slot {2 * b}: enc_out rms {e_enc:.3e}, mismatched indices {rep['mismatched_indices']}/{rep['total_indices']}, "
              f"recon rms {e_wav:.3e}, from embeddings {e_wav_e:.3e}")
        assert e_enc < 2e-5
        if rep["mismatched_indices"] == 0:
            assert rms(quant[None], ref_quant) == 0.0
            assert e_wav < WAV_RMS_TOL and e_wav_e < WAV_RMS_TOL
        else:                                                  # the tie proof of test_seqstream_gpu.check_against_reference, for the one row
            proofs = _assert_flips_are_near_ties(sd["quantizer.rq.model.embed"], torch.as_tensor(ref_enc).float().cpu(), ref_idx, codes[:, None],
                                                 got_enc=enc[None].float().cpu(), max_frames=max(1, rep["frames"] // 250))
            print(f"{name} [{how}] row {b}: tie proofs (stage, frame, gap, bound) {proofs}")
            cut = _prefix_before([p[1] for p in proofs], ref_idx.shape[2], hop, 0)
            n = T if cut is None else min(cut, T)
            if n > 0:
                assert rms(rec[None, ..., :n], torch.as_tensor(ref_recon)[..., :n]) < WAV_RMS_TOL, (b, n)
                assert rms(rec_e[None, ..., :n], torch.as_tensor(ref_recon)[..., :n]) < WAV_RMS_TOL, (b, n)
        # the lock-step session of one row fed the same pushes: the codes are asserted, the rest recorded
        cs = m.open_stream(1, n_q=nq, scale=torch.tensor([float(scale[b])]), max_frames=c["frames"])
        sc, sq, srec, pos = [], [], [], 0
        for i, n in enumerate(u.steps):
            cc, qq = cs.encode(u.wav[None, ..., pos:pos + n], final=i == len(u.steps) - 1)
            pos += n
            sc.append(cc); sq.append(qq)
            if cc.shape[-1]:
                srec.append(cs.decode(cc.permute(1, 2, 0).contiguous()))
        sc, sq, srec = torch.cat(sc, -1), torch.cat(sq, 1), torch.cat(srec, -1)[..., :T]
        assert torch.equal(codes, sc[:, 0]), b
        record_report("seqslots_vs_stream", fixture=name, chunking=how, row=b, quantized_equal=bool(torch.equal(quant, sq[0])),
                      wav_equal=bool(torch.equal(rec, srec[0])), wav_max_abs=float((rec - srec[0]).abs().max()))
    m.engine.check_status()


# ---- 5. rules -------------------------------------------------------------------------------------------------------------------------------
def test_a_push_past_max_frames_names_the_slot_and_changes_nothing_for_any_slot():
    import ctypes as C
    from funcodec_amd.engine import _ptr
    m, sd = _tiny()
    hop, S, bound = m.engine.hop_length, 3, 10
    wavs = [audio(1, hop * 14, 81 + s, "tones")[0] for s in range(S)]

    def run(refusals):
        st = m.open_slots(S, max_frames=bound)
        assert st.max_frames == bound
        out = {s: [] for s in range(S)}
        dec = {s: [] for s in range(S)}

        def push(parts):                                       # {slot: (first frame, frames)}
            res = st.encode({s: wavs[s][..., a * hop:(a + n) * hop] for s, (a, n) in parts.items()})
            for s, (c, q) in res.items():
                out[s] += [c, q]
            for s, w in st.decode({s: c.t().contiguous() for s, (c, q) in res.items()}).items():
                dec[s].append(w)
        push({0: (0, 7), 1: (0, 7)})
        push({0: (7, 3), 1: (7, 1)})                           # slot 0 stands at the bound on both sides, slot 1 at 8
        if refusals:
            with pytest.raises(EngineError, match=r"slot 0.*max_frames"):
                st.encode({0: wavs[0][..., 10 * hop:11 * hop], 1: wavs[1][..., 8 * hop:9 * hop]})
            with pytest.raises(EngineError, match=r"slot 0.*max_frames"):
                st.decode({0: torch.zeros(1, st.n_q, dtype=torch.int64), 1: torch.zeros(1, st.n_q, dtype=torch.int64)})
            ws = st._ws()
            buf = torch.zeros(S, 1, hop, device=m.device)
            codes = torch.empty(st.n_q, S, 1, dtype=torch.int64, device=m.device)
            tok = torch.zeros(S, 1, st.n_q, dtype=torch.int64, device=m.device)
            wout = torch.empty(S, 1, hop, device=m.device)
            cnt = lambda *v: (C.c_int32 * S)(*v)
            with pytest.raises(EngineError, match=r"slot encode: slot 0.*max_frames"):
                m.engine._check(m.engine.lib.fc_slots_encode(st._h, _ptr(buf), hop, cnt(hop, hop, 0), cnt(0, 0, 0), None, _ptr(codes), None, None, _ptr(ws),
                                                             ws.numel(), m.engine._stream()))
            with pytest.raises(EngineError, match=r"slot decode: slot 0.*max_frames"):
                m.engine._check(m.engine.lib.fc_slots_decode_codes(st._h, _ptr(tok), 1, cnt(1, 1, 0), cnt(0, 0, 0), 1, _ptr(wout), None, _ptr(ws),
                                                                   ws.numel(), m.engine._stream()))
        push({1: (8, 2), 2: (0, 7)})                           # slot 1 goes on to the bound, slot 2 starts
        st.start(0)                                            # the refused slot begins again
        push({0: (0, 7), 2: (7, 1)})
        return [t for s in range(S) for t in out[s] + dec[s]]
    clean, tried = run(False), run(True)
    assert len(clean) == len(tried) and all(torch.equal(a, b) for a, b in zip(clean, tried))
    assert torch.equal(clean[0], clean[4]) and torch.equal(clean[1], clean[5])      # slot 0: its restart gives its first push again
    with pytest.raises(EngineError, match="seq_model: transformer"):
        m.open_slots(1)
    with pytest.raises(EngineError, match="max_frames"):
        m.open_slots(1, max_frames=6)                          # below the START push (7 frames)
    m.engine.check_status()


def test_slots_with_their_own_stage_counts_equal_the_session_with_that_count():
    m, sd = _tiny()
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    frames = [9, 5, 1, 7]
    plan = [[6, 3, 2], [6, 1, 2], [6, 6, 5], [6, 2, 2]]
    wavs = [audio(1, sum(frames) * hop, 91 + s, "tones")[0] for s in range(3)]
    cuts = [sum(frames[:p]) * hop for p in range(len(frames) + 1)]
    feed = lambda p: {s: (wavs[s][..., cuts[p]:cuts[p + 1]], p == len(frames) - 1) for s in range(3)}
    uniform = {}
    for k in sorted({k for rows in plan for k in rows}):
        u = m.open_slots(3, n_q=k, max_frames=sum(frames))
        uniform[k] = [u.encode(feed(p)) for p in range(len(frames))]
    st = m.open_slots(3, max_frames=sum(frames))
    assert st.n_q == cap
    for p, rows in enumerate(plan):
        for s, k in enumerate(rows):
            st.set_n_q(s, k)
        got = st.encode(feed(p))
        for s, k in enumerate(rows):
            assert torch.equal(got[s][0][:k], uniform[k][p][s][0]), (p, s, k)
            assert k == cap or int(got[s][0][k:].abs().max()) == 0, (p, s, k)
    m.engine.check_status()
