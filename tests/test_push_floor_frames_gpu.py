"""A stage count per FRAME of a session push chosen on the device by a noise floor (fc_engine_set_floor_frames; csrc/rvq_rate_kernels.h
states THE PUSH FRAME RULE) on the MI355X: the fused launch against its four-launch chain bit for bit, the device's counts against
``floor_pick_frames`` of the device's own stage errors, a frame's count as a function of that frame alone, both session kinds (eager and
graph replay) against twins under ``set_n_q``, mode-1 packets written and read by sessions, and the refusals."""
import functools
import math

import numpy as np
import pytest
import torch

from funcodec_amd import io as fio
from funcodec_amd.engine import EngineError, floor_pick_frames, floor_value
from helpers import audio, engine_for, state_for

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


def same(a, b):
    """torch.equal that takes a NaN for a NaN (a row of NaN audio is NaN in both runs)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def crossing_db(E, frames, D, lo=1, want=3):
    """(noise_floor_db, k): a floor that errors E[0 .. cap] of `frames` frames cross at count k, lo < k: k is the strict new minimum
    of E[lo ..] nearest to `want`, the threshold lies half-way between E[k] and the smallest error in front of it (frames = 1: one
    frame's own curve, the push frame rule's threshold)"""
    E = [float(v) for v in E]
    new_min = [k for k in range(lo + 1, len(E)) if E[k] < min(E[lo:k])]
    assert new_min, f"the curve never falls behind stage {lo}: {E}"
    k = min(new_min, key=lambda v: abs(v - want))
    thr = 0.5 * (E[k] + min(E[lo:k]))
    assert thr < E[0]
    return 10.0 * math.log10(thr / (frames * D)), k


DECAY = 0.8          # the codebooks' sigma falls by 0.8 a stage: a sum of one code vector per stage is a row the quantiser can code


def hook_rows(m, cfg_name, seed, F, kind):
    """[3 F, D]: row 0 loud (every frame a sum of one code vector per stage plus a little noise: rows the quantiser can code), row 1 the
    same scaled by 1e-3 (kind "quiet") or holding one NaN (kind "nan"), row 2 zeros"""
    cb = state_for(cfg_name, seed, DECAY)[2]["quantizer.rq.model.embed"].astype(np.float64)
    nq, K, D = cb.shape
    rng = np.random.default_rng(4000 + 17 * F + nq)
    x = np.zeros((3, F, D), np.float32)
    for t in range(F):
        x[0, t] = cb[np.arange(nq), rng.integers(0, K, nq)].sum(0) + 0.02 * rng.standard_normal(D)
    x[1] = x[0] * 1e-3
    if kind == "nan":
        x[1, F // 2, D // 3] = NAN
    return torch.from_numpy(x.reshape(3 * F, D))


def spread(seen, lo, cap):
    """a test that shows a spread of counts saw lo, a cap and a count between them: otherwise it shows nothing"""
    assert lo in seen and cap in seen and any(lo < k < cap for k in seen), (sorted(seen), lo, cap)


def frame_floor(m, x, B, want=3):
    """(noise_floor_db, k): a floor that frame 0 of row 0 of x [B F, D] crosses at count k, from the stage errors at the cap"""
    cap, D = m.arch.num_quantizers, m.arch.codebook_dim
    serr = m.engine.rvq_encode(x, cap, noise_floor_db=[-INF] * B, per_frame=True, min_n_q=0)[2]["stage_errors"]
    return crossing_db(serr[:, 0, 0].tolist(), 1, D, want=want)


# ---- 1. the per-op hook: fused against chain ----------------------------------------------------------------------------------------
def _hook_case(cfg_name, seed, F):
    m = engine_for(cfg_name, seed, DECAY)
    eng, cap, D = m.engine, m.arch.num_quantizers, m.arch.codebook_dim
    caps = [cap, cap, cap - 1]
    for lo in (0, 1):
        seen = set()
        for kind in ("quiet", "nan"):
            x = hook_rows(m, cfg_name, seed, F, kind)
            db, k0 = frame_floor(m, x, 3)
            outs = {}
            for fused in (True, False):
                codes, quant, r = eng.rvq_encode(x, cap, n_q_rows=caps, noise_floor_db=[db] * 3, per_frame=True, min_n_q=lo, fused=fused)
                assert set(r) == {"n_q_frames", "stage_errors", "sub_quants"}
                outs[fused] = dict(codes=codes, quantized=quant, **r)
            a, b = outs[True], outs[False]
            assert a["n_q_frames"].dtype == torch.int32 and tuple(a["n_q_frames"].shape) == (3, F)
            for key in ("codes", "quantized", "sub_quants", "n_q_frames", "stage_errors"):
                assert same(a[key], b[key]), (cfg_name, F, kind, lo, key)
            # the stage errors are those of the row-floor hook on the same input
            rows = eng.rvq_encode(x, cap, n_q_rows=caps, noise_floor_db=[db] * 3, min_n_q=1)[2]
            assert same(a["stage_errors"], rows["stage_errors"])
            # the counts are the rule's, from the device's own stage errors
            ks = a["n_q_frames"].cpu().numpy()
            want = floor_pick_frames(a["stage_errors"].cpu().numpy(), F, floor_value(m.arch, db), lo, caps)
            assert np.array_equal(ks, want), (cfg_name, F, kind, lo, ks, want)
            assert ks[0, 0] == max(k0, lo) and (ks[2] == lo).all()
            if kind == "nan":       # the one NaN frame takes the cap, its neighbours in the row do not
                assert ks[1, F // 2] == cap and (np.delete(ks[1], F // 2) == lo).all()
            else:
                assert (ks[1] == lo).all()
            # every frame is what the call gives a one-frame row with that count, zeros behind the count
            flat = ks.reshape(-1)
            c1, q1 = eng.rvq_encode(x, cap, n_q_rows=[max(int(k), 1) for k in flat])
            live = torch.from_numpy(flat > 0).to(quant.device)
            assert same(a["codes"][:, live], c1[:, live]) and same(a["quantized"][live], q1[live])
            assert int(a["codes"][:, ~live].abs().sum()) == 0 and float(a["quantized"][~live].abs().sum()) == 0.0
            stage = torch.arange(cap, device=quant.device)[:, None]
            assert int((a["codes"] * (stage >= torch.from_numpy(flat).to(quant.device)[None, :])).abs().sum()) == 0
            sq = a["sub_quants"]                                                    # [n_q, B, D, F]: their sum in stage order is quantized
            acc = torch.zeros_like(sq[0])
            for i in range(cap):
                acc = acc + sq[i]
            assert same(acc.permute(0, 2, 1).reshape(3 * F, D), a["quantized"])
            seen.update(int(k) for k in flat)
        spread(seen, lo, cap)
    eng.check_status()


@pytest.mark.parametrize("F", [1, 15, 16, 17, 33, 257])
@pytest.mark.parametrize("cfg_name", ["tinyss", "tinywn"])
def test_hook_fused_equals_chain_and_floor_pick_frames(cfg_name, F):
    _hook_case(cfg_name, 5, F)


def test_hook_on_ss320_codebooks():
    _hook_case("ss320", 0, 7)


# ---- 2. a frame's count is the frame's alone -------------------------------------------------------------------------------------------
def test_a_frames_count_does_not_depend_on_the_shape_of_the_push():
    m = engine_for("tinyss", 5, DECAY)
    eng, cap = m.engine, m.arch.num_quantizers
    x = hook_rows(m, "tinyss", 5, 16, "nan")                    # N = 48 rows: 16 loud, 16 quiet (one of them holds a NaN), 16 zeros
    N = x.shape[0]
    db, _ = frame_floor(m, x, 3)
    for lo in (0, 1):
        got = []
        for B in (1, N, 3):
            codes, quant, r = eng.rvq_encode(x, cap, noise_floor_db=[db] * B, per_frame=True, min_n_q=lo)
            assert tuple(r["n_q_frames"].shape) == (B, N // B)
            got.append((r["n_q_frames"].reshape(-1), codes, quant))
        for ks, codes, quant in got[1:]:
            assert torch.equal(ks, got[0][0]) and torch.equal(codes, got[0][1]) and same(quant, got[0][2])
        spread(set(got[0][0].tolist()), lo, cap)
    # one-frame rows and min_n_q >= 1: the rule IS the push rule
    rows = eng.rvq_encode(x, cap, noise_floor_db=[db] * N, min_n_q=1)[2]["n_q_rows"]
    assert torch.equal(rows, got[1][0])
    eng.check_status()


# ---- 3. the search over the stages ---------------------------------------------------------------------------------------------------
def test_beam_frames_keep_the_first_k_codes_of_the_full_depth_path():
    m = engine_for("tinyss", 5, DECAY)
    eng, cap, D = m.engine, m.arch.num_quantizers, m.arch.codebook_dim
    F = 17
    x = hook_rows(m, "tinyss", 5, F, "quiet").view(3, F, D)
    x = torch.cat([x[0], x[0], x[2]], 0)                        # loud, loud again, zeros
    db, _ = frame_floor(m, x, 3)
    full = eng.rvq_encode(x, cap, beam=2)[0]                    # the full-depth path
    seen = set()
    for fused in (True, False):
        # row 1 under a floor of -inf dB: every frame takes its best count
        codes, quant, r = eng.rvq_encode(x, cap, beam=2, noise_floor_db=[db, -INF, db], per_frame=True, min_n_q=0, fused=fused)
        ks = r["n_q_frames"].reshape(-1)
        stage = torch.arange(cap, device=codes.device)[:, None]
        assert torch.equal(codes, full * (stage < ks[None, :]))
        acc = torch.zeros_like(r["sub_quants"][0])
        for i in range(cap):
            acc = acc + r["sub_quants"][i]
        assert torch.equal(acc.permute(0, 2, 1).reshape(3 * F, D), quant)
        seen.update(ks.tolist())
    spread(seen, 0, cap)
    eng.check_status()


# ---- the nets of the session tests ---------------------------------------------------------------------------------------------------
def _matched_model(arch, sd):
    """The net with its random codebooks scaled to half the level of its own encoder output.  An untrained encoder puts its output far
    from its random codebooks (and a louder input does not move it: the last layer is normalised), so that no stage lowers the error and
    every floor picks the same count; at half the level the nearest of 64 random codes lowers it stage after stage."""
    from funcodec_amd.model import EncodecMI355X

    def load(state):
        m = EncodecMI355X(arch, "cuda:0")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        return m
    m0 = load(sd)
    hop = m0.engine.hop_length
    kw = dict(max_frames=64) if arch.seq_model == "transformer" else {}
    st = m0.open_stream(1, **kw)
    first = max(st.min_first_samples // hop, st.min_first_frames)
    enc = st.encode(audio(1, (first + 8) * hop, 801, "tones").unsqueeze(1), want_enc_out=True)[2]
    e_enc = float(enc.double().pow(2).sum(-1).mean())
    cb = sd["quantizer.rq.model.embed"]
    e_cb = float((cb[0].astype(np.float64) ** 2).sum(-1).mean())
    scaled = dict(sd)
    scaled["quantizer.rq.model.embed"] = (cb * np.float32(0.5 * math.sqrt(e_enc / e_cb))).astype(np.float32)
    return load(scaled)


@functools.lru_cache(maxsize=None)
def _matched(cfg_name, seed=5):
    if cfg_name == "causal_tinytf":
        from test_seqstream_gpu import _tiny
        m0, sd = _tiny()
        return _matched_model(m0.arch, sd)
    _, arch, sd = state_for(cfg_name, seed, DECAY)
    return _matched_model(arch, sd)


def _schedule(st, hop):
    """samples per push: the start-up, 1 frame, 1 frame, 17 frames, a final push of odd length"""
    first = max(st.min_first_samples // hop, st.min_first_frames)
    return [first * hop, hop, hop, 17 * hop, 2 * hop + 3]


def _probe_db(m, open_stream, wav, sched, want=3):
    """a floor that the first frame of the session's first 1-frame push crosses at a count between lo and the cap"""
    cap, D = m.arch.num_quantizers, m.arch.codebook_dim
    probe = open_stream()
    probe.encode(wav[:1, :, :sched[0]])
    enc = probe.encode(wav[:1, :, sched[0]:sched[0] + sched[1]], want_enc_out=True)[2]
    assert D == enc.shape[-1]
    serr = m.engine.rvq_encode(enc.reshape(-1, D).contiguous(), cap, noise_floor_db=[-INF], per_frame=True, min_n_q=0)[2]["stage_errors"]
    return crossing_db(serr[:, 0, 0].tolist(), 1, D, want=want)


# ---- 4. both session kinds against twins under set_n_q ---------------------------------------------------------------------------------
STREAMS = [("tinyss", {}, False), ("tinyss", {}, True), ("causal_tinytf", dict(max_frames=64), False)]


@pytest.mark.parametrize("cfg_name,kw,graph", STREAMS, ids=["tinyss", "tinyss-graph", "transformer"])
def test_stream_frames_equal_twins_under_set_n_q(cfg_name, kw, graph):
    m = _matched(cfg_name)
    hop, cap, D = m.engine.hop_length, m.arch.num_quantizers, m.arch.codebook_dim
    caps = [cap, 4, cap]
    plain = m.open_stream(3, **kw)
    plain.set_n_q(caps)
    sched = _schedule(plain, hop)
    w = audio(1, sum(sched), 811, "tones")
    wav = torch.cat([w, w.flip(-1), 0.5 * w], 0).unsqueeze(1)
    db, k0 = _probe_db(m, lambda: m.open_stream(1, **kw), wav, sched)
    # row 0 under the floor, row 1 under a floor of +inf (always min_n_q = 0), row 2 without a floor (its cap in every frame)
    st = m.open_stream(3, noise_floor_db=[db, INF, None], per_frame=True, min_n_q=0, graph=graph, **kw)
    st.set_n_q(caps)
    assert st.per_frame and st.last_n_q_frames is None
    pushes, pos = [], 0
    for p, n in enumerate(sched):
        last = p == len(sched) - 1
        x = wav[..., pos:pos + n]
        codes, quant, enc = st.encode(x, final=last, want_enc_out=True)
        ks = st.last_n_q_frames.clone()
        tc, tq, te = plain.encode(x, final=last, want_enc_out=True)
        assert tuple(ks.shape) == (3, codes.shape[-1]) and ks.dtype == torch.int32
        assert torch.equal(enc, te), p                            # the encoder does not know about counts
        assert (ks[1] == 0).all() and (ks[2] == cap).all()
        assert int(codes[:, 1].abs().sum()) == 0 and float(quant[1].abs().sum()) == 0.0
        assert torch.equal(codes[:, 2], tc[:, 2]) and torch.equal(quant[2], tq[2])
        serr = m.engine.rvq_encode(enc.reshape(-1, D).contiguous(), cap, n_q_rows=caps, noise_floor_db=[-INF] * 3, per_frame=True,
                                   min_n_q=0)[2]["stage_errors"]
        want = floor_pick_frames(serr.cpu().numpy(), codes.shape[-1], [floor_value(m.arch, db), INF, None], 0, caps)
        assert np.array_equal(ks.cpu().numpy(), want), p
        pushes.append((x, last, codes, quant, ks))
        pos += n
    assert int(pushes[1][4][0, 0]) == k0
    seen = set(int(k) for _, _, _, _, ks in pushes for k in ks[0].tolist())          # the counts of the row under the floor
    spread(seen | set(int(k) for _, _, _, _, ks in pushes for k in ks[1:].reshape(-1).tolist()), 0, cap)
    assert any(0 < k < cap for k in seen), seen
    # for every distinct count k of row 0: a twin under set_n_q = k gives the same codes and quantized at the frames that took k
    for k in sorted(seen):
        if k == 0:
            for _, _, codes, quant, ks in pushes:
                sel = ks[0] == 0
                assert int(codes[:, 0, sel].abs().sum()) == 0 and float(quant[0, sel].abs().sum()) == 0.0
            continue
        twin = m.open_stream(3, **kw)
        twin.set_n_q([k, 1, 1])
        for x, last, codes, quant, ks in pushes:
            tc, tq = twin.encode(x, final=last)
            sel = ks[0] == k
            assert torch.equal(codes[:, 0, sel], tc[:, 0, sel]) and torch.equal(quant[0, sel], tq[0, sel]), k
    if graph:
        assert st.graph_stats()["fallbacks"] == 0
    m.engine.check_status()


@pytest.mark.parametrize("cfg_name,kw", [("tinywn", {}), ("causal_tinytf", dict(max_frames=64))], ids=["tinywn", "transformer"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_slots_out_of_phase_equal_one_slot_sessions(cfg_name, kw, graph):
    """S = 5: slot 0 starts a round late, slot 1 idles throughout, slot 2 ends in round 1, slot 3 has no floor, slot 4's audio is NaN, and
    so is everything behind a row's samples and in idle rows."""
    m = _matched(cfg_name)
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    probe = m.open_slots(1, **kw)
    first = max(probe.min_first_samples // hop, probe.min_first_frames)
    T = (first + 24) * hop + 3
    wavs = [audio(1, T, 820 + s, "tones")[0] * g for s, g in enumerate([1.0, 1.0, 0.5, 1.0, 1.0])]
    wavs[4] = torch.full_like(wavs[4], NAN)
    lines = {0: (1, [first, 1, 17]), 2: (0, [first + 1, 2]), 3: (0, [first, 1, 3, 2]), 4: (0, [first, 2, 1, 1])}
    finals = {2: 1}
    sched = [first * hop, hop]
    db, _ = _probe_db(m, lambda: m.open_stream(1, **kw), wavs[0][None, None], sched)
    dbs = {0: db, 2: INF, 3: None, 4: -30.0}              # slot 2 under a floor of +inf dB: always min_n_q = 0
    ss = m.open_slots(5, noise_floor_db=[dbs.get(s) for s in range(5)], per_frame=True, min_n_q=0, graph=graph, **kw)
    ss.pad_value = NAN
    ss.set_n_q(3, 4)
    one = {s: m.open_slots(1, noise_floor_db=dbs[s], per_frame=True, min_n_q=0, **kw) for s in lines}
    one[3].set_n_q(0, 4)
    pos = {s: 0 for s in lines}
    seen = set()
    for r in range(5):
        push = {}
        for s, (r0, steps) in lines.items():
            i = r - r0
            if 0 <= i < len(steps):
                last = finals.get(s) == i
                n = steps[i] * hop + (3 if last else 0)
                push[s] = (wavs[s][pos[s]:pos[s] + n], last)
                pos[s] += n
        if not push:
            break
        res, packets = ss.encode(push, packed=True)
        counts = ss.last_n_q_frames
        assert set(res) == set(push) == set(packets) == set(counts) and 1 not in packets
        for s, (w, last) in push.items():
            ref, ref_p = one[s].encode({0: (w, last)}, packed=True)
            assert same(res[s][0], ref[0][0]) and same(res[s][1], ref[0][1]), (r, s)
            ks = counts[s]
            assert ks.dtype == torch.int32 and ks.dim() == 1 and ks.shape[0] == res[s][0].shape[-1]
            if s == 3:          # no floor beside slots that have one: the slot's fixed n_q in every frame (its one-slot twin sets no floor at all)
                assert (ks == 4).all() and fio.packet_mode(packets[s]) == 1 and fio.packet_mode(ref_p[0]) == 0
                got_codes, got_counts, _ = fio.unpack_frame_packet(packets[s])
                assert got_counts.tolist() == [4] * len(ks) and np.array_equal(got_codes.T, res[s][0][:4].cpu().numpy())
                continue
            assert torch.equal(ks, one[s].last_n_q_frames[0]) and packets[s] == ref_p[0], (r, s)
            assert fio.packet_mode(packets[s]) == 1
            assert s != 4 or (ks == cap).all()                  # NaN audio: what the plain push gives it
            assert s != 2 or (ks == 0).all()
            seen.update(ks.tolist())
    spread(seen, 0, cap)
    if graph:
        assert ss.graph_stats()["fallbacks"] == 0
    m.engine.check_status()


def test_graphed_slots_replay_when_a_floor_changes():
    m = _matched("tinywn")
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    wav = audio(3, 40 * hop, 830, "tones")
    p1 = m.open_slots(1)
    first = max(p1.min_first_samples // hop, p1.min_first_frames)
    db0, _ = _probe_db(m, lambda: m.open_stream(1), wav[:1, None], [first * hop, hop])

    def run(ss):
        out, stats = [], []
        out.append(ss.encode({s: wav[s:s + 1, :first * hop] for s in range(3)}))
        pos = first
        for i in range(14):
            if i >= 6:                                               # from here on a floor changes before every push
                ss.set_noise_floor(i % 3, db0 + 1.5 * (i % 5 - 2))
            if i == 10:
                ss.set_noise_floor(1, None)
            out.append(ss.encode({s: wav[s:s + 1, pos * hop:(pos + 2) * hop] for s in range(3)}))
            out[-1]["k"] = {s: v.tolist() for s, v in ss.last_n_q_frames.items()}
            stats.append(ss.graph_stats())
            pos += 2
        return out, stats
    dbs = [db0, db0 + 3.0, db0 - 3.0]
    eo, _ = run(m.open_slots(3, noise_floor_db=dbs, per_frame=True, min_n_q=0))
    go, stats = run(m.open_slots(3, noise_floor_db=dbs, per_frame=True, min_n_q=0, graph=True))
    for a, b in zip(eo, go):
        assert a.keys() == b.keys() and a.get("k") == b.get("k")
        for s in range(3):
            assert torch.equal(a[s][0], b[s][0]) and torch.equal(a[s][1], b[s][1])
    assert len({str(o["k"]) for o in go[1:]}) > 1, "the floors moved no count"
    assert stats[-1]["fallbacks"] == 0
    assert stats[-1]["captures"] == stats[5]["captures"], "a floor that changes is device data: no further capture"
    assert stats[-1]["replays"] >= stats[5]["replays"] + 8
    m.engine.check_status()


# ---- 5. packets ------------------------------------------------------------------------------------------------------------------------
def test_stream_packets_are_mode_1_and_decode_to_what_the_counts_give():
    m = _matched("tinyss")                                          # no quantiser projections: decoding codes is decoding their sum
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    mk = lambda **kw: m.open_stream(3, **kw)
    plain = mk()
    sched = _schedule(plain, hop)
    w = audio(1, sum(sched), 811, "tones")
    wav = torch.cat([w, w.flip(-1), 0.5 * w], 0).unsqueeze(1)
    db, _ = _probe_db(m, lambda: m.open_stream(1), wav, sched)
    st = mk(noise_floor_db=[db, INF, None], per_frame=True, min_n_q=0)      # under the floor; always min_n_q = 0; no floor: the cap
    dec, dec_tab, dec_emb, dec_rows, dec_const = (mk(per_frame=True), mk(per_frame=True), mk(), mk(), mk(per_frame=True))
    pos, seen = 0, set()
    for p, n in enumerate(sched):
        last = p == len(sched) - 1
        codes, quant, packets = st.encode(wav[..., pos:pos + n], final=last, packed=True)
        ks = st.last_n_q_frames.clone()
        f = codes.shape[-1]
        for b, pk in enumerate(packets):
            assert fio.packet_mode(pk) == 1
            got_codes, got_counts, _ = fio.unpack_frame_packet(pk)
            assert got_counts.tolist() == ks[b].tolist() and len(got_counts) == f
            assert np.array_equal(got_codes.T, codes[:got_codes.shape[1], b].cpu().numpy())
            assert int(codes[got_codes.shape[1]:, b].abs().sum()) == 0
        tokens = codes.permute(1, 2, 0).contiguous()
        out = dec.decode_packed(packets, final=last)
        assert torch.equal(out, dec_tab.decode(tokens, final=last, n_q_frames=ks)), p
        ref = dec_emb.decode_emb(quant, final=last)
        assert torch.equal(out, ref), p                             # exactly the decode of the encode's quantized
        # a table that is constant per row is the decode push under set_n_q of those counts
        rows = [3, 1, cap]
        dec_rows.set_n_q(rows)
        table = torch.tensor(rows, dtype=torch.int32).view(3, 1).expand(3, f).contiguous()
        assert torch.equal(dec_const.decode(tokens, final=last, n_q_frames=table), dec_rows.decode(tokens, final=last)), p
        seen.update(ks.reshape(-1).tolist())
        pos += n
    spread(seen, 0, cap)
    # with no floor set the packets are mode 0 as before
    st2 = mk(per_frame=True)
    assert all(fio.packet_mode(pk) == 0 for pk in st2.encode(wav[..., :sched[0]], packed=True)[2])
    m.engine.check_status()


def test_slot_push_decodes_mode_0_and_mode_1_packets_together():
    m = _matched("tinywn")
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    p1 = m.open_slots(1)
    first = max(p1.min_first_samples // hop, p1.min_first_frames)
    wav = audio(2, (first + 5) * hop, 870, "tones")
    db, _ = _probe_db(m, lambda: m.open_stream(1), wav[:1, None], [first * hop, hop])
    enc1 = m.open_slots(1, noise_floor_db=db, per_frame=True, min_n_q=0)      # writes mode 1
    enc0 = m.open_slots(1, n_q=cap)                                          # writes mode 0
    enc0.set_n_q(0, 3)
    both = m.open_slots(3, per_frame=True)
    alone1, alone0 = m.open_slots(1, per_frame=True), m.open_slots(1)
    pos = 0
    for n in (first * hop, 2 * hop, 3 * hop):
        r1, pk1 = enc1.encode({0: wav[0, pos:pos + n]}, packed=True)
        r0, pk0 = enc0.encode({0: wav[1, pos:pos + n]}, packed=True)
        assert fio.packet_mode(pk1[0]) == 1 and fio.packet_mode(pk0[0]) == 0
        out = both.decode_packed({0: pk1[0], 2: pk0[0]})
        assert set(out) == {0, 2}
        assert torch.equal(out[0], alone1.decode_packed({0: pk1[0]})[0])
        assert torch.equal(out[2], alone0.decode_packed({0: pk0[0]})[0])
        pos += n
    m.engine.check_status()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_first_launch_and_change_nothing():
    m = engine_for("tinyss", 5, DECAY)
    eng, hop, cap, D = m.engine, m.engine.hop_length, m.arch.num_quantizers, m.arch.codebook_dim
    st, twin = m.open_stream(3, per_frame=True), m.open_stream(3)
    first = max(st.min_first_samples // hop, st.min_first_frames)
    w = audio(1, (first + 12) * hop, 860, "tones")
    wav = torch.cat([w, w * 1e-3, torch.zeros_like(w)], 0).unsqueeze(1)
    pos = [first * hop]

    def plain_push_equals_the_twins():
        x = wav[..., pos[0]:pos[0] + hop]
        a, b = st.encode(x), twin.encode(x)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ta = a[0].permute(1, 2, 0).contiguous()
        assert torch.equal(st.decode(ta), twin.decode(ta))
        pos[0] += hop
    a, b = st.encode(wav[..., :pos[0]]), twin.encode(wav[..., :pos[0]])
    assert torch.equal(a[0], b[0])
    ta = a[0].permute(1, 2, 0).contiguous()
    assert torch.equal(st.decode(ta), twin.decode(ta))
    # min_n_q outside [0, n_q], or above a cap
    for bad in (-1, cap + 1):
        with pytest.raises(EngineError, match=r"min_n_q lies in \[0, 6\]"):
            m.open_stream(3, per_frame=True, noise_floor_db=-20.0, min_n_q=bad)
    with pytest.raises(EngineError, match=r"min_n_q lies in \[1, 6\]"):
        m.open_stream(3, noise_floor_db=-20.0, min_n_q=0)           # without per_frame a count of 0 stays refused
    st.set_n_q([cap, 2, cap])
    st.min_n_q = 3
    st.set_noise_floor(-20.0)
    with pytest.raises(EngineError, match="min_n_q = 3 lies above the cap of row 1"):
        st.encode(wav[..., pos[0]:pos[0] + hop])
    st.set_noise_floor(None)
    st.min_n_q = 0
    st.set_n_q([cap] * 3)
    plain_push_equals_the_twins()
    # the library's own words: frame mode without a floor, a null table, min_nq out of range
    table = torch.zeros(3, dtype=torch.int32, device=eng.device)
    frames = torch.zeros((3, 1), dtype=torch.int32, device=eng.device)
    lib, h = eng.lib, eng._h
    assert lib.fc_engine_set_floor_frames(h, 0, frames.data_ptr(), None) != 0
    with pytest.raises(EngineError, match="fc_engine_set_floor_frames: no noise floor is set"):
        eng._check(1)
    with eng._floor([1.0] * 3, 1, table):
        for args, words in (((0, None, None), "n_q_frames_out"), ((-1, frames.data_ptr(), None), r"min_nq lies in \[0, num_quantizers = 6\]"),
                            ((cap + 1, frames.data_ptr(), None), r"min_nq lies in \[0, num_quantizers = 6\]")):
            assert lib.fc_engine_set_floor_frames(h, *args) != 0
            with pytest.raises(EngineError, match=words):
                eng._check(1)
    with pytest.raises(EngineError, match="min_nq lies in"):        # fc_engine_set_floor's own range stays
        with eng._floor([1.0] * 3, 0, table):
            pass
    plain_push_equals_the_twins()
    # a frame table of another shape; beside per-row counts; on an offline call
    x = wav[..., pos[0]:pos[0] + hop]
    codes = twin.encode(x)[0]
    st.encode(x)
    pos[0] += hop
    tokens = codes.permute(1, 2, 0).contiguous()
    with pytest.raises(EngineError, match=r"n_q_frames must be \[3, 1\]"):
        st.decode(tokens, n_q_frames=torch.ones((3, 2), dtype=torch.int32))
    with pytest.raises(EngineError, match="per_frame=True"):
        twin.decode(tokens, n_q_frames=torch.ones((3, 1), dtype=torch.int32))
    other = torch.ones((3, 2), dtype=torch.int32, device=eng.device)
    with eng._push_frame_nq(other):
        with pytest.raises(EngineError, match=r"set for \[3\]\[2\] frames \(fc_engine_set_push_frame_nq\); this push has \[3\]\[1\]"):
            twin.decode(tokens)
        with pytest.raises(EngineError, match="fc_engine_set_push_frame_nq.*session decode pushes only"):
            eng.decode_codes(tokens.expand(3, 2, cap).contiguous())
    twin.set_n_q([2, 2, 2])
    with eng._push_frame_nq(frames + 2):
        with pytest.raises(EngineError, match="fc_engine_set_push_frame_nq.*fc_engine_set_row_nq.*both set"):
            twin.decode(tokens)
    with eng._row_nq([2, 2, 2]):
        with pytest.raises(EngineError, match="fc_engine_set_push_frame_nq: per-row stage counts are set"):
            with eng._push_frame_nq(frames):
                pass
    twin.set_n_q([cap] * 3)
    assert torch.equal(st.decode(tokens), twin.decode(tokens))
    # the existing refusals of the offline frame table and of frame mode by target SNR on a session push stay, word for word
    with eng._frame_nq(frames, 3, 1):
        with pytest.raises(EngineError, match="it is for offline decode calls only"):
            twin.decode(tokens)
    plain_push_equals_the_twins()
    # a malformed mode-1 packet names the row and the field; a session without per_frame refuses mode 1 in today's words
    src = m.open_stream(3, noise_floor_db=-INF, per_frame=True, min_n_q=0)
    packets = src.encode(wav[..., :first * hop], packed=True)[2]
    assert all(fio.packet_mode(pk) == 1 for pk in packets)
    bad = list(packets)
    bad[1] = packets[1][:5] + bytes([packets[1][5] + 1]) + packets[1][6:]          # the bits field
    with pytest.raises(EngineError, match="decode_packed: row 1: packet field bits"):
        st.decode_packed(bad)
    bad[1] = packets[1][:-1]
    with pytest.raises(EngineError, match="decode_packed: row 1: packet field length"):
        st.decode_packed(bad)
    with pytest.raises(EngineError, match=r"row 0: packet field mode: a stage count per frame \(mode 1\) is for offline calls only; "
                                          "sessions decode packets of mode 0"):
        twin.decode_packed(packets)
    plain_push_equals_the_twins()
    eng.check_status()
