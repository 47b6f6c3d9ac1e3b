"""`-m gpu` tests of the slot session (funcodec_amd/stream.py StreamSlots, fc_slots_*): slots that start, push and end independently in
one batch.  The yardstick is the reference -- the CPU oracle on every utterance ALONE and the committed goldens -- with the bars of
test_stream_gpu.check_against_reference; between sessions the comparison is bit for bit."""
import numpy as np
import pytest
import torch

from conftest import record_report
from helpers import audio, engine_for, golden, manifest, oracle_for, rms
from test_gpu_parity import WAV_RMS_TOL
from test_stream_gpu import MIXED, _seam_net, pushes

pytestmark = pytest.mark.gpu
MAN = manifest()
NAN = float("nan")


class Utt:
    """one utterance of a test: its audio [C,T], the scale fed in, its push sizes, and what the session gave back for it"""

    def __init__(self, wav, scale, chunks, idle_at=()):
        self.wav, self.scale, self.T = wav, scale, wav.shape[-1]
        self.steps = []                       # per push of the session while the utterance is in its slot: samples, or None (idle)
        for i, n in enumerate(chunks):
            if i in idle_at:
                self.steps += [None, None]
            self.steps.append(n)
        self.pos, self.codes, self.quant, self.enc, self.rec, self.rec_e = 0, [], [], [], [], []

    def cat(self):
        return (torch.cat(self.codes, -1), torch.cat(self.quant, 0), torch.cat(self.enc, 0), torch.cat(self.rec, -1))


def drive(st, timelines, decode=True, emb=None):
    """timelines: per slot a list of (Utt, number of its steps to take or None for all) in order, or an int (idle pushes).  Runs the session
    push by push, every emitted frame decoded in the same round by the same slot.  emb: a second session that only decodes, fed the
    quantised embeddings of the same rounds through decode_emb (its slots get the utterance's scale from start alone)."""
    rows = []
    for tl in timelines:
        row = []
        for item in tl:
            if isinstance(item, int):
                row += [None] * item
            else:
                u, take = item
                steps = u.steps if take is None else u.steps[:take]
                row += [(u, n, i == 0, take is None and i == len(steps) - 1) for i, n in enumerate(steps)]
        rows.append(row)
    for r in range(max(len(row) for row in rows)):
        enc_push = {}
        for slot, row in enumerate(rows):
            if r >= len(row) or row[r] is None or row[r][1] is None:
                continue
            u, n, first, last = row[r]
            if first:
                st.start(slot, u.scale)
                if emb is not None:
                    emb.start(slot, u.scale)
            enc_push[slot] = (u.wav[..., u.pos:u.pos + n], last)
            u.pos += n
        if not enc_push:
            continue
        out = st.encode(enc_push, want_enc_out=True)
        dec_push = {}
        for slot, (c, q, e) in out.items():
            u = rows[slot][r][0]
            u.codes.append(c); u.quant.append(q); u.enc.append(e)
            dec_push[slot] = (c.t().contiguous(), enc_push[slot][1])
        if decode and dec_push:
            for slot, w in st.decode(dec_push).items():
                rows[slot][r][0].rec.append(w)
        if emb is not None and out:
            for slot, w in emb.decode_emb({slot: (q, enc_push[slot][1]) for slot, (c, q, e) in out.items()}).items():
                rows[slot][r][0].rec_e.append(w)


def assert_against_reference(tag, arch, u, ref_idx, ref_enc, ref_quant, ref_recon):
    """codes bit-exact; the bars of test_stream_gpu.check_against_reference for the rest"""
    codes, quant, enc, rec = u.cat()
    ref_idx = torch.as_tensor(np.asarray(ref_idx)).long()
    ref_idx = ref_idx.reshape(ref_idx.shape[0], -1)              # [n_q, 1, Tf] of the one utterance
    e_enc = rms(enc, ref_enc) if ref_enc is not None else float("nan")
    e_q, e_wav = rms(quant, ref_quant), rms(rec[..., :u.T], ref_recon)
    bad = int((codes.cpu() != ref_idx).sum())
    print(f"{tag}: T={u.T}: codes differing {bad}/{ref_idx.numel()}, enc_out rms {e_enc:.3e}, quantized rms {e_q:.3e}, recon rms {e_wav:.3e}")
    assert codes.shape == ref_idx.shape and rec.shape[-1] >= u.T
    assert bad == 0, tag
    assert ref_enc is None or e_enc < 2e-5, tag
    projected = arch.codebook_dim != arch.dimension
    assert e_q <= (1e-5 * float(np.sqrt((np.asarray(ref_quant) ** 2).mean())) if projected else 0.0), tag
    assert e_wav < WAV_RMS_TOL, tag
    if u.rec_e:                                                  # the reconstruction from the embeddings, by a session that only decodes
        rec_e = torch.cat(u.rec_e, -1)
        assert rec_e.shape == rec.shape and rms(rec_e[..., :u.T], ref_recon) < WAV_RMS_TOL, tag


def _utt(m, cfg_name, T, seed, how, idle_at=(), kind="tones"):
    hop = m.engine.hop_length
    wav = audio(1, T, seed, kind, m.engine.channels)
    ref = oracle_for(cfg_name, 5).inference(wav, bit_width=None, use_scale=True)
    return Utt(wav[0] if wav.dim() == 3 else wav, ref["scale"], pushes(T, hop, how), idle_at), ref


# ---- 1. against the oracle and the goldens -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["frames1", "mixed"])
@pytest.mark.parametrize("cfg_name", ["tinyss", "tinywn", "tinystwn"])
def test_staggered_slots_against_the_oracle_on_each_utterance_alone(cfg_name, how):
    """S = 4, six utterances (plus one that is abandoned) spread over the slots, starts staggered by 0 / 3 / 11 pushes, idle pushes in the
    middle of utterances, one slot reused after FINAL and one by a START that abandons its running utterance."""
    m = engine_for(cfg_name, 5)
    arch, hop = m.arch, m.engine.hop_length
    lens = [40 * hop, 40 * hop + 1, 40 * hop + hop - 1, 23 * hop + 7, 9 * hop, 40 * hop + 1]
    us = [_utt(m, cfg_name, T, 400 + i, how, idle_at=(7,) if i in (0, 3) else ()) for i, T in enumerate(lens)]
    dropped, _ = _utt(m, cfg_name, 30 * hop, 450, how)
    st = m.open_slots(4)
    drive(st, [[(us[0][0], None), (us[4][0], None)],            # reused after FINAL
               [3, (us[1][0], None)],
               [11, (dropped, 9), (us[2][0], None)],            # START abandons the running utterance
               [(us[3][0], None), 2, (us[5][0], None)]], emb=m.open_slots(4))
    assert dropped.codes and dropped.rec_e, "the abandoned utterance must be past its start-up: it is running in the library when START drops it"
    for i, (u, ref) in enumerate(us):
        assert u.rec_e
        assert_against_reference(f"{cfg_name} [{how}] utterance {i}", arch, u, ref["code_indices"][0].numpy(), ref["encoder_out"],
                                 ref["code_embeddings"][0][0], ref["recon_speech"])
    m.engine.check_status()


@pytest.mark.parametrize("name", ["tinywn_b2_t777", "tinystwn_b2_t777"])
def test_golden_rows_in_different_slots_three_pushes_apart(name):
    c = MAN["cases"][name]
    m = engine_for(c["config"], c["weight_seed"], c["codebook_decay"])
    hop = m.engine.hop_length
    wav = audio(c["batch"], c["samples"], c["audio_seed"], c["audio_kind"], c.get("channels", 1))
    g = golden(name)
    us = []
    for b in range(2):
        w = wav[b] if wav.dim() == 3 else wav[b:b + 1]
        us.append(Utt(w, float(g["scale"].reshape(-1)[b]) if "scale" in g else None, pushes(c["samples"], hop, "mixed")))
    st = m.open_slots(3, n_q=c["n_q"])
    drive(st, [[(us[0], None)], [], [3, (us[1], None)]])
    for b, u in enumerate(us):
        assert_against_reference(f"{name} row {b}", m.arch, u, g["indices"][:, b:b + 1].astype(np.int64), g["encoder_out"][b:b + 1] if "encoder_out" in g else None,
                                 g["quantized"][b:b + 1], g["recon"][b:b + 1])
    m.engine.check_status()


# ---- 2. a slot depends on nothing but its own pushes ------------------------------------------------------------------------------------
def _crowd(m, cfg_name, n, long_at):
    """n busy neighbours: staggered utterances, the one at `long_at` with pushes ten frames long"""
    hop = m.engine.hop_length
    out = []
    for i in range(n):
        T = (25 + 3 * (i % 4)) * hop + (i * 7) % hop
        wav = audio(1, T, 500 + i, "noise" if i % 2 else "tones", m.engine.channels)
        chunks = pushes(T, hop, "mixed") if i != long_at else [10 * hop] * (T // (10 * hop)) + ([T % (10 * hop)] if T % (10 * hop) else [])
        out.append([i % 5, (Utt(wav[0] if wav.dim() == 3 else wav, 0.5 + 0.1 * (i % 3), chunks), None)])
    return out


@pytest.mark.parametrize("cfg_name", ["tinyss", "tinywn"])
def test_a_slot_gives_the_same_bits_alone_and_among_busy_slots_whatever_lies_behind_its_count(cfg_name):
    m = engine_for(cfg_name, 5)
    hop = m.engine.hop_length
    T = 30 * hop + 7
    wav = audio(1, T, 77, "tones", m.engine.channels)
    mk = lambda: Utt(wav[0] if wav.dim() == 3 else wav, 0.8, pushes(T, hop, "mixed"), idle_at=(3,))
    alone = mk()
    drive(m.open_slots(1), [[(alone, None)]], emb=m.open_slots(1))
    want = alone.cat() + (torch.cat(alone.rec_e, -1),)
    assert all(bool(torch.isfinite(t.float()).all()) for t in want)
    for pad in (0.0, NAN):
        for S, slot in ((3, 0), (3, 2), (17, 16)):
            u = mk()
            crowd = _crowd(m, cfg_name, S - 1, long_at=0)
            st = m.open_slots(S)
            st_e = m.open_slots(S)
            st.pad_value = st_e.pad_value = pad       # what lies behind every row's count, and all of an idle row
            drive(st, crowd[:slot] + [[(u, None)]] + crowd[slot:], emb=st_e)
            for name, a, b in zip(("codes", "quantized", "enc_out", "wav", "wav from embeddings"), u.cat() + (torch.cat(u.rec_e, -1),), want):
                assert torch.equal(a, b), (cfg_name, S, slot, pad, name)
    m.engine.check_status()


def test_behind_a_rows_valid_part_every_output_is_zero_and_nan_input_there_reaches_nothing():
    from funcodec_amd.stream import FC_SLOT_FINAL, FC_SLOT_START
    m = engine_for("tinywn", 5)
    hop = m.engine.hop_length
    st = m.open_slots(4)
    st.pad_value = NAN
    lens = {0: 20 * hop + 3, 2: 12 * hop, 3: 16 * hop + hop - 1}                                 # slot 1 idle: NaN throughout
    rows = {s: (audio(1, n, 90 + s, "tones").to(m.device), FC_SLOT_START | FC_SLOT_FINAL) for s, n in lens.items()}
    out = st._encode_call(rows, True)
    full = [t._base for t in out[0]]                                                             # the batch-wide tensors the slices view
    Tf = full[0].shape[-1]
    assert Tf == m.engine.frames(max(lens.values()))
    for s in range(4):
        n = m.engine.frames(lens[s]) if s in lens else 0
        assert bool((full[0][:, s, n:] == 0).all()) and bool((full[1][s, n:] == 0).all()) and bool((full[2][s, n:] == 0).all()), s
        assert bool(torch.isfinite(full[1][s]).all()) and bool(torch.isfinite(full[2][s]).all())
    dec = st._decode_call({s: (out[s][0].t().contiguous(), FC_SLOT_START | FC_SLOT_FINAL) for s in lens}, True, False)
    wav = dec[0][0]._base
    for s in range(4):
        n = m.engine.frames(lens[s]) * hop if s in lens else 0
        assert bool((wav[s, :, n:] == 0).all()) and bool(torch.isfinite(wav[s]).all()), s
        assert s not in lens or float(wav[s, :, :n].abs().max()) > 0
    m.engine.check_status()


# ---- 3. against CodecStream(batch = 1) with the same pushes --------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["tinyss", "tinywn"])
def test_a_slot_against_a_one_utterance_stream_with_the_same_pushes(cfg_name):
    m = engine_for(cfg_name, 5)
    arch, hop = m.arch, m.engine.hop_length
    T = 40 * hop + 1
    u, ref = _utt(m, cfg_name, T, 600, "mixed")
    other, _ = _utt(m, cfg_name, 33 * hop, 601, "frames1")
    drive(m.open_slots(2), [[2, (other, None)], [(u, None)]])
    cs = m.open_stream(1, scale=ref["scale"])
    sc, sq, srec = [], [], []
    pos = 0
    for i, n in enumerate(u.steps):
        c, q = cs.encode(u.wav[None, ..., pos:pos + n], final=i == len(u.steps) - 1)
        pos += n
        sc.append(c); sq.append(q)
        if c.shape[-1]:
            srec.append(cs.decode(c.permute(1, 2, 0).contiguous()))
    sc, sq, srec = torch.cat(sc, -1), torch.cat(sq, 1), torch.cat(srec, -1)
    codes, quant, enc, rec = u.cat()
    assert torch.equal(codes, sc[:, 0])
    refs = (ref["code_indices"][0].numpy(), ref["encoder_out"], ref["code_embeddings"][0][0], ref["recon_speech"])
    assert_against_reference(f"{cfg_name} slot", arch, u, *refs)
    via_stream = Utt(u.wav, u.scale, [])
    via_stream.codes, via_stream.quant, via_stream.enc, via_stream.rec = [sc[:, 0]], [sq[0]], [enc], [srec[0]]      # (its encoder output is not asked for)
    assert_against_reference(f"{cfg_name} stream", arch, via_stream, *refs)
    # recorded, not asserted: the same kernels in the same form, so the bits should agree
    record_report("slots_vs_stream", config=cfg_name, quantized_equal=bool(torch.equal(quant, sq[0])), wav_equal=bool(torch.equal(rec, srec[0])),
                  wav_max_abs=float((rec - srec[0]).abs().max()))


# ---- 4. the LSTM stage alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 512])
def test_lstm_rows_with_their_own_step_counts_equal_one_row_streams_bit_for_bit(H):
    from test_lstm_kernels import _check, _torch_lstm
    m, sd = _seam_net(H)
    S, T = 4, 10
    steps = [(0, 1, 7, 10), (10, 7, 1, 0)]
    start = [(1, 1, 1, 1), (0, 1, 0, 0)]                  # row 1 is restarted in the second push
    gen = torch.Generator().manual_seed(20 + H)
    xs = [torch.randn(S, H, T, generator=gen) for _ in range(2)]
    for decoder in (False, True):
        side = "decoder." if decoder else "encoder."
        prefix = [k[: -len(".weight_ih_l0")] for k in sd if k.startswith(side) and k.endswith(".weight_ih_l0")][0]
        st = m.open_slots(S)
        ys = [st.lstm_forward(x.clone().masked_fill_(torch.arange(T)[None, None] >= torch.tensor(s)[:, None, None], NAN), s, f, decoder=decoder)
              for x, s, f in zip(xs, steps, start)]      # what lies behind a row's steps is NaN: it must reach nothing
        for b in range(S):
            cs = m.open_stream(1)
            fed = []
            for p in range(2):
                n = steps[p][b]
                assert bool((ys[p][b, :, n:] == 0).all()), (H, decoder, b, p)
                if start[p][b] and p:
                    cs.reset()
                    fed = []
                if n:
                    xb = xs[p][b:b + 1, :, :n].contiguous()
                    want = cs.lstm_forward(xb, decoder=decoder)
                    assert torch.equal(ys[p][b:b + 1, :, :n], want), (H, decoder, b, p, float((ys[p][b:b + 1, :, :n] - want).abs().max()))
                    fed.append((xb, ys[p][b:b + 1, :, :n]))
                if fed and (p == 1 or (start[1][b] and p == 0)):      # the recurrence of one utterance so far, against float64
                    x_all, y_all = torch.cat([f[0] for f in fed], -1), torch.cat([f[1] for f in fed], -1)
                    refs = []
                    for dtype in (torch.float64, torch.float32):
                        with torch.no_grad():
                            refs.append(_torch_lstm(sd, prefix, H, 2, dtype)(x_all.to(dtype).permute(2, 0, 1))[0].permute(1, 2, 0).double().contiguous())
                    _check((H, 2, False, 1, x_all.shape[-1], 1.0), y_all.cpu(), refs[0], refs[1], "slots")
        m.engine.check_status()


# ---- 5. the rules -----------------------------------------------------------------------------------------------------------------------
def test_a_refused_push_names_its_rule_and_changes_nothing():
    import ctypes as C
    from funcodec_amd.engine import EngineError, _ptr
    from funcodec_amd.stream import FC_SLOT_FINAL, FC_SLOT_START
    m = engine_for("tinywn", 5)
    hop, S = m.engine.hop_length, 3
    T = 24 * hop
    wav = audio(1, T, 81, "tones")
    chunks = pushes(T, hop, "mixed")

    def run(refusals):
        u = Utt(wav, 0.7, chunks)
        st = m.open_slots(S)
        need = st.min_first_samples
        Tc = need + 2 * hop
        buf = torch.zeros(S, 1, Tc, device=m.device)
        codes = torch.empty(st.n_q, S, m.engine.frames(Tc), dtype=torch.int64, device=m.device)

        def raw(counts, flags, match, width=Tc, decode=False):
            ws = st._ws()
            with pytest.raises(EngineError, match=match):
                if decode:
                    tok = torch.zeros(S, width, st.n_q, dtype=torch.int64, device=m.device)
                    out = torch.empty(S, 1, width * hop, device=m.device)
                    m.engine._check(m.engine.lib.fc_slots_decode_codes(st._h, _ptr(tok), width, (C.c_int32 * S)(*counts), (C.c_int32 * S)(*flags), 1, _ptr(out),
                                                                       None, _ptr(ws), ws.numel(), m.engine._stream()))
                else:
                    m.engine._check(m.engine.lib.fc_slots_encode(st._h, _ptr(buf), width, (C.c_int32 * S)(*counts), (C.c_int32 * S)(*flags), None, _ptr(codes),
                                                                 None, None, _ptr(ws), ws.numel(), m.engine._stream()))
        if refusals:
            raw([0, 0, 0], [0, 0, 0], "no slot is active")
            raw([need, 0, 0], [0, 0, 0], "push without START")                       # nothing is running in slot 0
            raw([need - hop, 0, 0], [FC_SLOT_START, 0, 0], "at least")                # a START push shorter than fc_slots_min_first
            raw([need + 1, 0, 0], [FC_SLOT_START, 0, 0], "multiple of the hop")
            raw([Tc + hop, 0, 0], [FC_SLOT_START, 0, 0], "count lies in")
            raw([0, need, 0], [FC_SLOT_FINAL, FC_SLOT_START, 0], "idle slot")
            raw([need, 0, 0], [FC_SLOT_START, 0, 0], "wide", width=st.max_chunk + hop)
            raw([0, 0, st.min_first_frames - 1], [0, 0, FC_SLOT_START], "at least", width=st.min_first_frames, decode=True)
            raw([0, 1, 0], [0, 0, 0], "push without START", width=st.min_first_frames, decode=True)
        drive(st, [[(u, 5)]], decode=False)
        assert u.codes, "the start-up must be over: the utterance is running in the library"
        if refusals:                                                                  # in the middle of the utterance, other slots and this one
            raw([hop + 1, 0, 0], [0, 0, 0], "multiple of the hop")
            raw([hop, hop, 0], [0, 0, 0], "slot 1")
        rest = Utt(wav, 0.7, chunks)
        rest.steps, rest.pos = u.steps[5:], u.pos
        tl = [(rest, n, False, i == len(rest.steps) - 1) for i, n in enumerate(rest.steps)]
        for (uu, n, _, last) in tl:
            c, q, e = st.encode({0: (uu.wav[..., uu.pos:uu.pos + n], last)}, want_enc_out=True)[0]
            uu.pos += n
            u.codes.append(c); u.quant.append(q); u.enc.append(e)
        if refusals:
            raw([hop, 0, 0], [0, 0, 0], "FINAL push")                                 # the utterance has ended
        return torch.cat(u.codes, -1), torch.cat(u.quant, 0), torch.cat(u.enc, 0)
    clean, tried = run(False), run(True)
    for a, b in zip(clean, tried):
        assert torch.equal(a, b)
    m.engine.check_status()


# ---- 6. sessions and offline calls on one engine ------------------------------------------------------------------------------------------
def test_a_slot_session_a_stream_and_offline_calls_do_not_disturb_each_other():
    m = engine_for("tinywn", 5)
    hop = m.engine.hop_length
    T = 24 * hop
    a, b = audio(2, T, 51, "tones"), audio(1, T, 52, "noise")
    chunks = pushes(T, hop, "mixed")
    mk = lambda i: Utt(a[i:i + 1], 1.0, chunks)
    alone = [mk(0), mk(1)]
    drive(m.open_slots(2), [[(alone[0], None)], [1, (alone[1], None)]])
    cs = m.open_stream(1)
    stream_alone = [cs.encode(b[..., sum(chunks[:i]):sum(chunks[:i + 1])], final=i == len(chunks) - 1) for i in range(len(chunks))]
    off_ref = m.engine.encode_decode(a, m.arch.num_quantizers)
    us, st, cs = [mk(0), mk(1)], m.open_slots(2), m.open_stream(1)
    got_stream = []
    for r in range(len(chunks) + 1):                    # a slot push, a stream push and an offline call, round by round
        drive_round = {}
        for slot, u in enumerate(us):
            i = r - slot
            if 0 <= i < len(chunks):
                if i == 0:
                    st.start(slot, u.scale)
                drive_round[slot] = (u.wav[..., u.pos:u.pos + chunks[i]], i == len(chunks) - 1)
                u.pos += chunks[i]
        out = st.encode(drive_round, want_enc_out=True)
        if r < len(chunks):
            got_stream.append(cs.encode(b[..., sum(chunks[:r]):sum(chunks[:r + 1])], final=r == len(chunks) - 1))
        off = m.engine.encode_decode(a, m.arch.num_quantizers)
        assert torch.equal(off["codes"], off_ref["codes"]) and torch.equal(off["recon"], off_ref["recon"])
        dec = st.decode({slot: (c.t().contiguous(), drive_round[slot][1]) for slot, (c, q, e) in out.items()})
        for slot, (c, q, e) in out.items():
            us[slot].codes.append(c); us[slot].quant.append(q); us[slot].enc.append(e); us[slot].rec.append(dec[slot])
    for u, w in zip(us, alone):
        for x, y in zip(u.cat(), w.cat()):
            assert torch.equal(x, y)
    for x, y in zip(got_stream, stream_alone):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    m.engine.check_status()


# ---- 7. a slot that only decodes, and a push that fails half-way ----------------------------------------------------------------------
def test_a_session_that_only_decodes_golden_codes_with_the_scale_given_at_start_or_one():
    name = "tinywn_b2_t777"
    c = MAN["cases"][name]
    m = engine_for(c["config"], c["weight_seed"], c["codebook_decay"])
    hop, g = m.engine.hop_length, golden(name)
    assert "scale" in g and float(np.abs(g["scale"] - 1).min()) > 1e-3, "the fixture must carry a scale that is not 1"
    tok = torch.from_numpy(g["indices"].astype(np.int64)).permute(1, 2, 0).contiguous()        # [B, Tf, n_q]
    Tf = tok.shape[1]
    fch = [7, 3, 1, 5, 2, 1, 8]
    st = m.open_slots(3, n_q=c["n_q"])
    st.pad_value = NAN
    rec = {0: [], 2: []}
    for b, slot in ((0, 2), (1, 0)):
        st.start(slot, float(g["scale"].reshape(-1)[b]))
    chunks = []
    while sum(chunks) < Tf:
        chunks.append(min(fch[len(chunks) % len(fch)], Tf - sum(chunks)))
    starts = [sum(chunks[:i]) for i in range(len(chunks))]
    for i in range(len(chunks) + 3):                         # slot 2 carries row 0, slot 0 row 1 three pushes later
        push = {}
        for row, slot, j in ((0, 2, i), (1, 0, i - 3)):
            if 0 <= j < len(chunks):
                push[slot] = (tok[row, starts[j]:starts[j] + chunks[j]], j == len(chunks) - 1)
        for slot, w in st.decode(push).items():
            rec[slot].append(w)
    for b, slot in ((0, 2), (1, 0)):
        w = torch.cat(rec[slot], -1)
        e = rms(w[..., :c["samples"]], g["recon"][b])
        print(f"{name}: decode-only slot {slot}, row {b}: recon rms {e:.3e}")
        assert w.shape[-1] == Tf * hop and e < WAV_RMS_TOL
    # a slot that was never started, in a fresh session: scale 1, i.e. what use_scale=False gives, and not silence
    a, b = m.open_slots(2, n_q=c["n_q"]), m.open_slots(2, n_q=c["n_q"])
    wa, wb = a.decode({1: (tok[0], True)}, use_scale=True)[1], b.decode({1: (tok[0], True)}, use_scale=False)[1]
    assert torch.equal(wa, wb) and float(wa.abs().max()) > 0
    assert rms(wa[..., :c["samples"]] * float(g["scale"].reshape(-1)[0]), g["recon"][0]) < WAV_RMS_TOL
    m.engine.check_status()


def test_a_push_that_fails_after_validation_poisons_every_slot_until_it_is_restarted():
    import ctypes as C
    from funcodec_amd.engine import EngineError, _ptr
    m = engine_for("tinywn", 5)
    hop, S = m.engine.hop_length, 2
    T = 20 * hop
    wavs = [audio(1, T, 71 + i, "tones") for i in range(S)]
    good = m.open_slots(S).encode({i: (w, True) for i, w in enumerate(wavs)})
    st = m.open_slots(S)
    st.encode({0: wavs[0][..., :10 * hop], 1: wavs[1][..., :10 * hop]})                   # both slots are running
    keep_ws, keep_need = m.engine._ws, st._ws_bytes
    m.engine._ws, st._ws_bytes = torch.empty(8192, dtype=torch.uint8, device=m.device), 8192
    with pytest.raises(EngineError, match="workspace too small"):                          # a host-side failure behind the validation
        st.encode({0: wavs[0][..., 10 * hop:11 * hop]})
    m.engine._ws, st._ws_bytes = keep_ws, keep_need
    with pytest.raises(EngineError, match=r"start\(1\)"):                                  # the wrapper: every slot, not only the one pushed
        st.encode({1: wavs[1][..., 10 * hop:11 * hop]})
    ws, buf = st._ws(), torch.zeros(S, 1, hop, device=m.device)
    codes = torch.empty(st.n_q, S, 1, dtype=torch.int64, device=m.device)
    for side in (0, 1):                                                                    # the library: both slots, both sides, its own message
        counts = (C.c_int32 * S)(*[hop if not side else 1] * S)
        with pytest.raises(EngineError, match="restarted with START"):
            if side:
                tok, out = torch.zeros(S, 1, st.n_q, dtype=torch.int64, device=m.device), torch.empty(S, 1, hop, device=m.device)
                m.engine._check(m.engine.lib.fc_slots_decode_codes(st._h, _ptr(tok), 1, counts, (C.c_int32 * S)(), 1, _ptr(out), None, _ptr(ws), ws.numel(),
                                                                   m.engine._stream()))
            else:
                m.engine._check(m.engine.lib.fc_slots_encode(st._h, _ptr(buf), hop, counts, (C.c_int32 * S)(), None, _ptr(codes), None, None, _ptr(ws),
                                                             ws.numel(), m.engine._stream()))
    st.start(0)
    st.start(1)                                                                            # START recovers a slot: the same bits as a fresh session
    again = st.encode({i: (w, True) for i, w in enumerate(wavs)})
    for i in range(S):
        assert torch.equal(again[i][0], good[i][0]) and torch.equal(again[i][1], good[i][1])
    m.engine.check_status()
