"""A stage count per push of a session chosen on the device by a noise floor (fc_engine_set_floor; csrc/rvq_rate_kernels.h states THE PUSH
RULE) on the MI355X: the fused launch against its four-launch chain bit for bit, the device's counts against ``floor_pick`` of the device's
own row errors, and every session kind against a twin session that is fed ``set_n_q`` = the chosen counts before each push."""
import functools
import math

import numpy as np
import pytest
import torch

from funcodec_amd.engine import EngineError, _Ratios, floor_pick, floor_value
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
    """(noise_floor_db, k): a floor that row errors E[0 .. cap] of `frames` frames cross at count k, lo < k: k is the strict new minimum
    of E[lo ..] nearest to `want`, the threshold lies half-way between E[k] and the smallest error in front of it"""
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


# ---- 1. the per-op hook: fused against chain ----------------------------------------------------------------------------------------
def _hook_case(cfg_name, seed, F):
    m = engine_for(cfg_name, seed, DECAY)
    eng, cap, D = m.engine, m.arch.num_quantizers, m.arch.codebook_dim
    seen = set()
    for kind in ("quiet", "nan"):
        x = hook_rows(m, cfg_name, seed, F, kind)
        probe = eng.rvq_encode(x, cap, noise_floor_db=[-INF] * 3)[2]            # at the cap: the row errors the floors are chosen from
        db, k_loud = crossing_db(probe["row_errors"][0].tolist(), F, D)
        caps = [cap, cap, cap - 1]
        outs = {}
        for fused in (True, False):
            codes, quant, r = eng.rvq_encode(x, cap, n_q_rows=caps, noise_floor_db=[db] * 3, min_n_q=1, fused=fused)
            outs[fused] = dict(codes=codes, quantized=quant, **r)
        a, b = outs[True], outs[False]
        assert a["n_q_rows"].dtype == torch.int32 and a["row_errors"].dtype == torch.float64
        for key in ("codes", "quantized", "sub_quants", "n_q_rows", "row_errors", "stage_errors"):
            assert same(a[key], b[key]), (cfg_name, F, kind, key)
        ks = a["n_q_rows"].tolist()
        E = a["row_errors"].cpu().numpy()
        assert ks == floor_pick(E, F, floor_value(m.arch, db), 1, caps).tolist(), (ks, E)
        assert ks == [k_loud, cap if kind == "nan" else 1, 1], (kind, ks)
        # the row sums are the float64 sums of the stage errors
        serr = a["stage_errors"].double().cpu().numpy()
        want = serr.sum(2).T
        ok = np.isclose(E, want, rtol=1e-12, atol=0) | (np.isnan(E) & np.isnan(want))
        assert ok.all()
        # every row is what the call with n_q_rows = the chosen counts gives it, zeros behind its count
        c2, q2 = eng.rvq_encode(x, cap, n_q_rows=ks)
        assert same(a["quantized"], q2) and same(a["codes"], c2)
        cd = a["codes"].view(cap, 3, F)
        for row, k in enumerate(ks):
            assert int(cd[k:, row].abs().max()) == 0 if k < cap else True
        sq = a["sub_quants"]                                                      # [n_q, B, D, F]: their sum in stage order is quantized
        acc = torch.zeros_like(sq[0])
        for i in range(cap):
            acc = acc + sq[i]
        assert same(acc.permute(0, 2, 1).reshape(3 * F, D), a["quantized"])
        seen.update(ks)
    assert len(seen) >= 3 and 1 in seen and cap in seen, seen      # min_n_q, a cap and a count between them: otherwise this shows nothing
    eng.check_status()


@pytest.mark.parametrize("F", [1, 2, 7, 100, 256, 257])
@pytest.mark.parametrize("cfg_name", ["tinyss", "tinywn"])
def test_hook_fused_equals_chain_and_floor_pick(cfg_name, F):
    _hook_case(cfg_name, 5, F)


def test_hook_on_ss320_codebooks():
    _hook_case("ss320", 0, 7)


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
    _, arch, sd = state_for(cfg_name, seed, DECAY)
    return _matched_model(arch, sd)


# ---- 2. CodecStream -----------------------------------------------------------------------------------------------------------------
def _stream_rows(m, seed, T):
    """[3, 1, T]: loud, the same scaled by 1e-3, zeros"""
    w = audio(1, T, seed, "tones")
    return torch.cat([w, w * 1e-3, torch.zeros_like(w)], 0).unsqueeze(1)


def _push_errors(m, enc, caps):
    """row errors [B, n_q + 1] of one push from its encoder output [B, Tf, D] (these nets quantise the encoder output itself)"""
    cap = m.arch.num_quantizers
    B, Tf, D = enc.shape
    assert D == m.arch.codebook_dim
    r = m.engine.rvq_encode(enc.reshape(B * Tf, D).contiguous(), cap, n_q_rows=caps, noise_floor_db=[-INF] * B)[2]
    return r["row_errors"].cpu().numpy()


def _schedule(st, hop):
    """samples per push: the start-up, 1 frame, 3 frames, a final push of odd length"""
    first = max(st.min_first_samples // hop, st.min_first_frames)
    return [first * hop, hop, 3 * hop, 2 * hop + 3]


def _twin_pushes(m, open_session, wav, caps, dbs):
    """Push wav through a session with floors `dbs` and a twin without a floor that is fed set_n_q(k of this push) before each push;
    returns both sessions and, per push, (codes, quantized, enc_out, packets, counts, twin codes, twin quantized, twin enc_out)."""
    hop = m.engine.hop_length
    st = open_session(noise_floor_db=dbs, min_n_q=1)
    twin = open_session()
    st.set_n_q(caps)
    out, pos = [], 0
    sched = _schedule(st, hop)
    for p, n in enumerate(sched):
        last = p == len(sched) - 1
        x = wav[..., pos:pos + n]
        codes, quant, enc, packets = st.encode(x, final=last, want_enc_out=True, packed=True)
        ks = st.last_n_q_rows.tolist()
        twin.set_n_q(ks)
        tc, tq, te = twin.encode(x, final=last, want_enc_out=True)
        out.append((codes, quant, enc, packets, ks, tc, tq, te))
        pos += n
    return st, twin, out


def test_stream_rows_take_the_count_their_push_picks():
    m = _matched("tinyss")
    hop, cap, D = m.engine.hop_length, m.arch.num_quantizers, m.arch.codebook_dim
    caps = [cap, 4, 2]
    probe = m.open_stream(3)
    probe.set_n_q(caps)
    sched = _schedule(probe, hop)
    wav = _stream_rows(m, 811, sum(sched))
    E, pos = [], 0
    for p, n in enumerate(sched):                                   # the probing run at the caps
        enc = probe.encode(wav[..., pos:pos + n], final=p == len(sched) - 1, want_enc_out=True)[2]
        E.append((_push_errors(m, enc, caps), enc.shape[1]))
        pos += n
    db_loud, _ = crossing_db(E[1][0][0], E[1][1], D)                # the loud row crosses inside its 1-frame push
    db_zero = max(10.0 * math.log10(max(e[2][0], 1e-30) / (f * D)) for e, f in E) + 3.0       # the zero row's input lies below its floor in every push
    dbs = [db_loud, db_loud, db_zero]
    st, twin, out = _twin_pushes(m, lambda **kw: m.open_stream(3, **kw), wav, caps, dbs)
    floors = [floor_value(m.arch, v) for v in dbs]
    seen = set()
    for p, (codes, quant, enc, packets, ks, tc, tq, te) in enumerate(out):
        f = codes.shape[-1]
        assert f == E[p][1]
        assert ks == floor_pick(E[p][0], f, floors, 1, caps).tolist(), (p, ks)
        assert ks[2] == 1, "the zero row takes min_n_q in every push"
        assert torch.equal(codes, tc) and torch.equal(quant, tq) and torch.equal(enc, te), p
        for b, k in enumerate(ks):
            assert k <= caps[b] and (k == cap or int(codes[k:, b].abs().max()) == 0), (p, b, k)
            assert packets[b][4] == k and int.from_bytes(packets[b][:4], "little") == f       # the packet carries k_b
        last = p == len(out) - 1
        twin.set_n_q(ks)
        assert torch.equal(st.decode_packed(packets, final=last), twin.decode(codes.permute(1, 2, 0).contiguous(), final=last)), p
        seen.update(ks)
    assert len(seen) >= 2, f"every row of every push took the same count: {seen}"
    st.set_noise_floor(None)                                        # and back: nothing is set on the engine, the caps hold
    assert st._push_floor() is None
    m.engine.check_status()


# ---- 3. StreamSlots -----------------------------------------------------------------------------------------------------------------
def test_slots_out_of_phase_equal_one_slot_sessions():
    """S = 5: slot 0 starts a round late, slot 1 idles throughout, slot 2 ends in round 1, slots 3 and 4 run; slot 4's audio is NaN, and so
    is everything behind a row's samples and in idle rows.  A floor per slot."""
    m = _matched("tinywn")
    hop, cap, D = m.engine.hop_length, m.arch.num_quantizers, m.arch.codebook_dim
    probe = m.open_slots(1)
    first = max(probe.min_first_samples // hop, probe.min_first_frames)
    T = (first + 8) * hop + 3
    wavs = [audio(1, T, 820 + s, "tones")[0] * g for s, g in enumerate([1.0, 1.0, 0.5, 1.0, 1.0])]
    wavs[4] = torch.full_like(wavs[4], NAN)
    # per slot: round of the first push and the frames of its pushes (the last one of slot 2 is FINAL and 3 samples longer)
    lines = {0: (1, [first, 1, 2]), 2: (0, [first + 1, 2]), 3: (0, [first, 1, 3, 2]), 4: (0, [first, 2, 1, 1])}
    finals = {2: 1}
    # floors: from a probing run of every slot's first push alone (slot 4 is NaN: any floor)
    dbs, want = {}, {0: 2, 2: 5, 3: 3}
    for s in (0, 2, 3):
        p1 = m.open_slots(1)
        enc = p1.encode({0: wavs[s][:lines[s][1][0] * hop]}, want_enc_out=True)[0][2]
        dbs[s] = crossing_db(_push_errors(m, enc[None], [cap])[0], enc.shape[0], D, want=want[s])[0]
    dbs[4] = -30.0
    ss = m.open_slots(5, noise_floor_db=[dbs.get(s) for s in range(5)], min_n_q=1)
    ss.pad_value = NAN
    ss.set_n_q(3, 4)
    one = {s: m.open_slots(1, noise_floor_db=dbs[s]) for s in lines}
    one[3].set_n_q(0, 4)
    pos = {s: 0 for s in lines}
    assert ss.last_n_q_rows == {s: 0 for s in range(5)}
    seen = set()
    for r in range(5):
        if r == 3:
            ss.set_noise_floor(3, None)                              # slot 3 returns to its fixed n_q
            one[3].set_noise_floor(0, None)
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
        before = ss.last_n_q_rows
        res, packets = ss.encode(push, packed=True)
        counts = ss.last_n_q_rows
        assert set(res) == set(push) == set(packets) and 1 not in packets      # the idle slot gives no packet
        for s in range(5):
            if s not in push:
                assert counts[s] == before[s], (r, s)               # an idle slot's entry is untouched
        assert counts[1] == 0
        for s, (w, last) in push.items():
            ref, ref_p = one[s].encode({0: (w, last)}, packed=True)
            assert same(res[s][0], ref[0][0]) and same(res[s][1], ref[0][1]), (r, s)
            k = counts[s]
            assert packets[s][4] == k and packets[s] == ref_p[0], (r, s)
            assert (s == 3 and r >= 3) or k == one[s].last_n_q_rows[0], (r, s)      # (a session without any floor writes no count)
            assert k == cap or int(res[s][0][k:].abs().max()) == 0
            if s == 4:
                assert k == cap                                      # NaN audio: what the plain push gives it
            elif s == 3 and r >= 3:
                assert k == 4                                        # no floor: the slot's fixed n_q
            else:
                seen.add(k)
    assert len(seen) >= 2, seen
    m.engine.check_status()


# ---- 4. graph replay ----------------------------------------------------------------------------------------------------------------
def test_graphed_slots_replay_when_a_floor_changes():
    m = _matched("tinywn")
    hop, cap, D = m.engine.hop_length, m.arch.num_quantizers, m.arch.codebook_dim
    wav = audio(3, 40 * hop, 830, "tones")
    p1 = m.open_slots(1)                                             # the floors: around the crossing of slot 0's first push
    enc = p1.encode({0: wav[0:1, :max(p1.min_first_samples // hop, p1.min_first_frames) * hop]}, want_enc_out=True)[0][2]
    db0 = crossing_db(_push_errors(m, enc[None], [cap])[0], enc.shape[0], D)[0]

    def run(ss):
        out, stats = [], []
        first = max(ss.min_first_samples // hop, ss.min_first_frames)
        out.append(ss.encode({s: wav[s:s + 1, :first * hop] for s in range(3)}))
        pos = first
        for i in range(14):
            if i >= 6:                                               # from here on a floor changes before every push
                ss.set_noise_floor(i % 3, db0 + 1.5 * (i % 5 - 2))
            if i == 10:
                ss.set_noise_floor(1, None)
            out.append(ss.encode({s: wav[s:s + 1, pos * hop:(pos + 1) * hop] for s in range(3)}))
            out[-1]["k"] = ss.last_n_q_rows
            stats.append(ss.graph_stats())
            pos += 1
        return out, stats
    dbs = [db0, db0 + 3.0, db0 - 3.0]
    eo, _ = run(m.open_slots(3, noise_floor_db=dbs))
    sg = m.open_slots(3, noise_floor_db=dbs, graph=True)
    go, stats = run(sg)
    for a, b in zip(eo, go):
        assert a.keys() == b.keys()
        assert a.get("k") == b.get("k")
        for s in range(3):
            assert torch.equal(a[s][0], b[s][0]) and torch.equal(a[s][1], b[s][1])
    assert len({tuple(o["k"].values()) for o in go[1:]}) > 1, "the floors moved no count"
    assert stats[-1]["fallbacks"] == 0
    assert stats[-1]["captures"] == stats[5]["captures"], "a floor that changes is device data: no further capture"
    assert stats[-1]["replays"] >= stats[5]["replays"] + 8
    m.engine.check_status()


# ---- 5. the search over the stages ---------------------------------------------------------------------------------------------------
def test_beam_rows_keep_the_first_k_codes_of_the_full_depth_path():
    m = engine_for("tinyss", 5, DECAY)
    hop, cap = m.engine.hop_length, m.arch.num_quantizers
    st = m.open_stream(3, rvq_beam=4, noise_floor_db=[-INF, -22.0, 60.0])
    full = m.open_stream(3, rvq_beam=4)
    sched = _schedule(st, hop)
    wav = _stream_rows(m, 840, sum(sched))
    pos, seen = 0, set()
    for p, n in enumerate(sched):
        last = p == len(sched) - 1
        codes = st.encode(wav[..., pos:pos + n], final=last)[0]
        fc = full.encode(wav[..., pos:pos + n], final=last)[0]
        ks = st.last_n_q_rows.tolist()
        for b, k in enumerate(ks):
            assert torch.equal(codes[:k, b], fc[:k, b]) and (k == cap or int(codes[k:, b].abs().max()) == 0), (p, b, k)
        assert ks[2] == 1                                           # a floor of +60 dB: always min_n_q
        seen.update(ks)
        pos += n
    print(f"counts under the search: {sorted(seen)}")
    m.engine.check_status()


# ---- 6. a session with a key / value cache -----------------------------------------------------------------------------------------
def test_seqstream_session_equals_its_twin():
    from test_seqstream_gpu import _tiny
    m0, sd = _tiny()
    m = _matched_model(m0.arch, sd)
    hop, cap, D = m.engine.hop_length, m.arch.num_quantizers, m.arch.codebook_dim
    caps = [cap, 4, 2]
    probe = m.open_stream(3, max_frames=24)
    sched = _schedule(probe, hop)
    wav = _stream_rows(m, 850, sum(sched))
    enc = probe.encode(wav[..., :sched[0]], want_enc_out=True)[2]
    db, _ = crossing_db(_push_errors(m, enc, [cap] * 3)[0], enc.shape[1], D)
    st, twin, out = _twin_pushes(m, lambda **kw: m.open_stream(3, max_frames=24, **kw), wav, caps, [db, db, db + 6.0])
    for p, (codes, quant, enc, packets, ks, tc, tq, te) in enumerate(out):
        assert torch.equal(codes, tc) and torch.equal(quant, tq) and torch.equal(enc, te), p
        assert all(1 <= k <= c for k, c in zip(ks, caps)) and [pk[4] for pk in packets] == ks
    m.engine.check_status()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_first_launch_and_change_nothing():
    m = engine_for("tinyss", 5, DECAY)
    eng, hop, cap, D = m.engine, m.engine.hop_length, m.arch.num_quantizers, m.arch.codebook_dim
    st, twin = m.open_stream(3), m.open_stream(3)
    sched = _schedule(st, hop)
    wav = _stream_rows(m, 860, sched[0] + 8 * hop)
    table = torch.zeros(3, dtype=torch.int32, device=eng.device)
    pos = [sched[0]]

    def plain_push_equals_the_twins():
        x = wav[..., pos[0]:pos[0] + hop]
        a, b = st.encode(x), twin.encode(x)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        pos[0] += hop
    a, b = st.encode(wav[..., :sched[0]]), twin.encode(wav[..., :sched[0]])
    assert torch.equal(a[0], b[0])
    # an offline call while a floor is set
    with eng._floor([1.0] * 3, 1, table):
        with pytest.raises(EngineError, match="session pushes only"):
            m.inference(wav[..., :sched[0]])
    plain_push_equals_the_twins()
    # a floor together with a rate: on the host, and by either setter
    x = torch.randn(6, D)
    with pytest.raises(EngineError, match="noise_floor_db and target_snr_db"):
        eng.rvq_encode(x, cap, target_snr_db=[10.0] * 3, noise_floor_db=[-20.0] * 3)
    with eng._floor([1.0] * 3, 1, table):
        with pytest.raises(EngineError, match="fc_engine_set_rate: a noise floor is set"):
            with eng._rate(_Ratios([0.1] * 3), 1, cap, 2):
                pass
    with eng._rate(_Ratios([0.1] * 3), 1, cap, 2):
        with pytest.raises(EngineError, match="fc_engine_set_floor: a rate is set"):
            with eng._floor([1.0] * 3, 1, table):
                pass
    plain_push_equals_the_twins()
    # a floor of another B
    with eng._floor([1.0] * 2, 1, table):
        with pytest.raises(EngineError, match="a noise floor is set for 2 rows .*this push has 3"):
            st.encode(wav[..., pos[0]:pos[0] + hop])
    plain_push_equals_the_twins()
    # min_n_q above a cap, a NaN floor, a negative one: the library's own words
    st.set_n_q([cap, 2, cap])
    st.min_n_q = 3
    st.set_noise_floor(-20.0)
    with pytest.raises(EngineError, match="min_n_q = 3 lies above the cap of row 1"):
        st.encode(wav[..., pos[0]:pos[0] + hop])
    st.set_noise_floor(None)
    st.min_n_q = 1
    st.set_n_q([cap] * 3)
    for bad in (NAN, -1.0):
        with pytest.raises(EngineError, match="neither negative nor NaN"):
            with eng._floor([1.0, bad, 1.0], 1, table):
                pass
    with pytest.raises(EngineError, match="min_nq lies in"):
        with eng._floor([1.0] * 3, cap + 1, table):
            pass
    plain_push_equals_the_twins()
    # the existing refusal of a push under a rate stays
    with eng._rate(_Ratios([0.1] * 3), 1, cap, 1):
        with pytest.raises(EngineError, match="offline calls only"):
            st.encode(wav[..., pos[0]:pos[0] + hop])
    plain_push_equals_the_twins()
    eng.check_status()
