"""Graph replay of stream and slot pushes (open_stream / open_slots with graph=True; fc_graphstream_set, fc_graphslots_set): a graphed session gives the eager
session's bits, replays what it has captured, and falls back or fails exactly as the header says."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import audio, engine_for, golden, manifest, state_for
from test_slots_gpu import Utt, drive
from test_stream_gpu import check_against_reference, stream_decode, stream_encode

pytestmark = pytest.mark.gpu
MAN = manifest()
NAN = float("nan")
NETS = ["tinyss", "tinywn", "tinystwn"]


def chunks_1_3(T, hop):
    """pushes of 1, 1 and 3 frames in turn, then the ragged rest (a FINAL push of a non-hop length)"""
    out, left, i = [], T // hop, 0
    while left > 0:
        f = min((1, 1, 3)[i % 3], left)
        out.append(f * hop)
        left, i = left - f, i + 1
    if T % hop:
        out.append(T % hop)
    return out


def spy(st, log):
    """log (side, width, parity of the side's push count) of every push the session hands to the library: the key of a graphed twin"""
    enc, dec, n = st._encode_call, st._decode_call, {"enc": 0, "dec": 0}

    def encode_call(rows, want):
        log.append(("enc", max(w.shape[-1] for w, f in rows.values()), n["enc"] & 1))
        n["enc"] += 1
        return enc(rows, want)

    def decode_call(rows, use_scale, emb):
        log.append(("dec", max(t.shape[0] for t, f in rows.values()), n["dec"] & 1))
        n["dec"] += 1
        return dec(rows, use_scale, emb)
    st._encode_call, st._decode_call = encode_call, decode_call


def timeline(m):
    """S = 4: staggered STARTs, idle pushes inside utterances, slot 0 reused after FINAL, slot 2 reused by a START that abandons"""
    hop, ch = m.engine.hop_length, m.engine.channels

    def utt(T, seed, idle_at=()):
        wav = audio(1, T, seed, "tones", ch)
        return Utt(wav[0] if wav.dim() == 3 else wav, 0.5 + 0.125 * (seed % 4), chunks_1_3(T, hop), idle_at)
    us = [utt(22 * hop + 5, 601, (9,)), utt(20 * hop + hop - 1, 602), utt(21 * hop + 1, 603), utt(19 * hop + 3, 604, (8,)), utt(16 * hop + 2, 605),
          utt(18 * hop + 1, 606)]
    dropped = utt(24 * hop, 607)
    return us + [dropped], [[(us[0], None), (us[4], None)], [3, (us[1], None)], [5, (dropped, 9), (us[2], None)], [(us[3], None), 2, (us[5], None)]]


def same_lists(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. slots, twin sessions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", NETS)
def test_a_graphed_slot_session_gives_the_eager_sessions_bits_and_replays(cfg_name):
    m = engine_for(cfg_name, 5)
    log = []
    eager, graphed = m.open_slots(4), m.open_slots(4, graph=True)
    assert graphed.graph and not eager.graph and eager._g is None
    eager.pad_value = graphed.pad_value = NAN                       # behind every row's count and in idle rows
    spy(eager, log)
    ue, tle = timeline(m)
    ug, tlg = timeline(m)
    drive(eager, tle)
    drive(graphed, tlg)
    for a, b in zip(ue, ug):
        assert a.codes and same_lists(a.codes, b.codes) and same_lists(a.quant, b.quant) and same_lists(a.enc, b.enc) and same_lists(a.rec, b.rec)
    n = graphed.graph_stats()
    keys = set(log)
    print(f"{cfg_name}: {len(log)} pushes, {len(keys)} keys, {n}")
    assert min(sum(1 for k in log if k[0] == side) for side in ("enc", "dec")) >= 12
    assert {k[2] for k in keys if k[0] == "enc"} == {0, 1} and {k[2] for k in keys if k[0] == "dec"} == {0, 1}
    assert n["fallbacks"] == 0 and n["evictions"] == 0
    assert n["captures"] == len(keys)
    assert n["replays"] == len(log) - len(keys) > 0
    assert eager.graph_stats() == dict(replays=0, captures=0, evictions=0, fallbacks=0)
    m.engine.check_status()


# ---- 2. stream against the reference ------------------------------------------------------------------------------------------------
class Graphed:
    """the model with open_stream(graph=True): what check_against_reference opens its sessions from"""

    def __init__(self, m):
        self.m, self.engine, self.arch, self.opened = m, m.engine, m.arch, []

    def open_stream(self, *a, **kw):
        self.opened.append(self.m.open_stream(*a, graph=True, **kw))
        return self.opened[-1]


@pytest.mark.parametrize("how", ["frames1", "mixed"])
@pytest.mark.parametrize("name", ["tinywn_b2_t777", "tinystwn_b2_t777"])
def test_a_graphed_stream_against_the_reference_golden_and_the_eager_stream(name, how):
    c = MAN["cases"][name]
    m = engine_for(c["config"], c["weight_seed"], c["codebook_decay"])
    cfg, arch, sd = state_for(c["config"], c["weight_seed"], c["codebook_decay"])
    wav = audio(c["batch"], c["samples"], c["audio_seed"], c["audio_kind"], c.get("channels", 1))
    g = golden(name)
    scale = torch.from_numpy(g["scale"]) if "scale" in g else None
    args = (arch, sd, c["n_q"], wav, g["indices"].astype(np.int64), g.get("encoder_out"), g["quantized"], g["recon"], scale, how)
    gm = Graphed(m)
    codes, recon = check_against_reference(name + " graphed", gm, *args)
    codes_e, recon_e = check_against_reference(name, m, *args)
    assert torch.equal(codes, codes_e) and torch.equal(recon, recon_e)
    stats = gm.opened[0].graph_stats()
    print(f"{name} [{how}]: {stats}")
    assert stats["replays"] > 0 and stats["fallbacks"] == 0
    # every output of the encoder side, and what the one-off pushes do to the counts
    from test_stream_gpu import pushes
    hop = m.engine.hop_length
    chunks = pushes(wav.shape[-1], hop, how)
    sg, se = m.open_stream(c["batch"], n_q=c["n_q"], scale=scale, graph=True), m.open_stream(c["batch"], n_q=c["n_q"], scale=scale)
    outs_e = stream_encode(se, wav, chunks)
    pos, parts, seen_first = 0, [], False
    for i, n in enumerate(chunks):
        before = sg.graph_stats()
        parts.append(sg.encode(wav[..., pos:pos + n], final=i == len(chunks) - 1, want_enc_out=True))
        pos += n
        after = sg.graph_stats()
        if parts[-1][0].shape[-1] and not seen_first:             # the push that ends the start-up is the library's first push
            seen_first = True
            assert after == before, "the first push of an utterance is a one-off"
        if i == len(chunks) - 1:
            assert after == before, "the final push is a one-off"
    assert seen_first and sg.graph_stats()["replays"] > 0
    for k in range(3):
        assert torch.equal(torch.cat([p[k] for p in parts], -1 if k == 0 else 1), outs_e[k])
    m.engine.check_status()


# ---- 3. row bit rates -----------------------------------------------------------------------------------------------------------------
def test_stage_counts_set_between_pushes_and_the_tables_presence_is_part_of_the_key():
    m = engine_for("tinywn", 5)
    hop, B, nq = m.engine.hop_length, 2, m.arch.num_quantizers
    wav = audio(B, 30 * hop, 91, "tones")
    first = 12 * hop

    def run(st):
        c0, q0 = st.encode(wav[..., :first])
        out, stats = [(c0, q0, st.decode(c0.permute(1, 2, 0).contiguous()))], []      # the first push of either side: a one-off
        for i in range(12, 30):
            if i == 16:
                st.set_n_q([1, nq - 1])
            if i == 22:
                st.set_n_q([nq, nq])                               # all stages: no table is set on the engine for these pushes
            c, q = st.encode(wav[..., i * hop:(i + 1) * hop])
            out.append((c, q, st.decode(c.permute(1, 2, 0).contiguous())))
            stats.append(st.graph_stats())
        return out, stats
    (e0, *eo), _ = run(m.open_stream(B))
    (g0, *go), stats = run(m.open_stream(B, graph=True))
    for a, b in zip([e0] + eo, [g0] + go):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert int((go[5][0][1:, 0] != 0).sum()) == 0 and int((go[3][0][1:, 0] != 0).sum()) > 0      # the counts did reach the pushes
    caps = [s["captures"] for s in stats]
    # pushes 12 .. 15 without a table: encode and decode, two parities -> 4 captures; 16 .. 21 with it: 4 more; 22 on without: none
    assert caps[3] == 4 and caps[5] == 8 and caps[9] == 8, caps
    assert caps[-1] == 8 and stats[-1]["replays"] == 2 * len(stats) - 8 and stats[-1]["fallbacks"] == 0
    # a slot session: the slot's count changed in the middle of its utterance
    w = audio(1, 24 * hop, 92, "tones")

    def slots(st):
        out = []
        for i, (a, b) in enumerate([(0, 12), (12, 13), (13, 14), (14, 15), (15, 16), (16, 17), (17, 24)]):
            if i == 3:
                st.set_n_q(1, 2)
            res = st.encode({1: (w[..., a * hop:b * hop], b == 24)})
            out.append(res[1])
        return out
    sg = m.open_slots(3, graph=True)
    for a, b in zip(slots(m.open_slots(3)), slots(sg)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert sg.graph_stats()["replays"] > 0 and sg.graph_stats()["fallbacks"] == 0
    m.engine.check_status()


# ---- 4. slots with a key / value cache --------------------------------------------------------------------------------------------
def test_graphed_slots_of_a_transformer_net_at_their_own_cache_positions():
    from test_seq_transformer_gpu import MAN as MAN_TF, _engine
    c = MAN_TF["cases"]["ss320tfc_b2_t16000"]
    m, sd = _engine(c["config"], c["weight_seed"])
    hop, nq = m.engine.hop_length, c["n_q"]
    wav = audio(3, 40 * hop, 93, "tones")

    def run(st):
        out = []

        def step(push):                                                             # every emitted frame decoded by the same slot
            res = st.encode(push)
            dec = st.decode({s: r[0].t().contiguous() for s, r in res.items()})
            out.append({s: (r[0], r[1], dec.get(s)) for s, r in res.items()})
        first = st.min_first_samples // hop
        assert first + 23 <= 40
        step({0: wav[0:1, :first * hop]})                                           # START push of slot 0 alone
        step({0: wav[0:1, first * hop:(first + 1) * hop], 2: wav[2:3, :(first + 2) * hop]})
        pos = [first + 1, 0, first + 2]
        for i in range(20):                                                         # one-frame pushes, the slots at different positions
            push = {0: wav[0:1, pos[0] * hop:(pos[0] + 1) * hop], 2: wav[2:3, pos[2] * hop:(pos[2] + 1) * hop]}
            if i == 4:
                push[1] = wav[1:2, :first * hop]                                     # a START in the middle
                pos[1] = first - 1
            elif i > 4 and i % 3:
                push[1] = wav[1:2, pos[1] * hop:(pos[1] + 1) * hop]
            step(push)
            for s in push:
                pos[s] += 1
        return out
    same = lambda x, y: (x is None and y is None) or torch.equal(x, y)
    eo = run(m.open_slots(3, n_q=nq, max_frames=64))
    sg = m.open_slots(3, n_q=nq, max_frames=64, graph=True)
    go = run(sg)
    assert len(eo) == len(go) == 22
    for a, b in zip(eo, go):
        assert a.keys() == b.keys()
        for s in a:
            assert all(same(x, y) for x, y in zip(a[s], b[s])), s
    assert any(v[2] is not None for v in go[-1].values())
    n = sg.graph_stats()
    print(f"ss320tfc slots: {n}")
    assert n["replays"] >= 30 and n["fallbacks"] == 0
    m.engine.check_status()


# ---- 5. refusal -----------------------------------------------------------------------------------------------------------------------
def test_a_lock_step_session_with_max_frames_refuses_graph_replay_in_the_librarys_words():
    from funcodec_amd.engine import EngineError
    from funcodec_amd.stream import GRAPH_MAX_FRAMES_REFUSAL
    from test_seqstream_gpu import _tiny
    m, _ = _tiny()
    with pytest.raises(EngineError, match="max_frames") as ei:
        m.open_stream(1, max_frames=64, graph=True)
    assert str(ei.value) == GRAPH_MAX_FRAMES_REFUSAL
    st = m.open_stream(1, max_frames=64)
    assert m.engine.lib.fc_graphstream_set(st._h, 1) != 0
    from funcodec_amd import _lib
    assert _lib.last_error() == GRAPH_MAX_FRAMES_REFUSAL and not m.engine.lib.fc_graphstream_enabled(st._h)
    assert m.engine.lib.fc_graphstream_set(st._h, 0) == 0


# ---- 6. / 7. the key and the cache, through the C ABI -----------------------------------------------------------------------------
class RawStream:
    """fc_stream_* with the caller's own pointers: a running utterance of B = 1 behind its first push, on a stream that can be captured"""

    def __init__(self, m, graph, frames=24):
        from funcodec_amd.engine import _ptr
        self.m, self.lib, self.hop, self._ptr = m, m.engine.lib, m.engine.hop_length, _ptr
        self.st = m.open_stream(1, max_chunk=frames * self.hop)
        self.h, self.nq, self.D = self.st._h, self.st.n_q, m.arch.dimension
        self.stream = torch.cuda.Stream()
        self.ws = torch.empty(self.st._ws_bytes, dtype=torch.uint8, device=m.device)
        if graph:
            m.engine._check(self.lib.fc_graphstream_set(self.h, 1))
        self.wav = audio(1, 400 * self.hop, 95, "tones").to(m.device).reshape(1, 1, -1).contiguous()
        self.pos = 0
        self.push(self.st.min_first_samples // self.hop)           # the first push: a one-off

    def push(self, frames, codes=None, quant=None):
        n = frames * self.hop
        x = self.wav[..., self.pos:self.pos + n].contiguous() if codes is None else self.fixed_in[..., :n]
        if codes is not None:
            x.copy_(self.wav[..., self.pos:self.pos + n])
        self.pos += n
        codes = torch.empty(self.nq, 1, frames, dtype=torch.int64, device=self.m.device) if codes is None else codes
        quant = torch.empty(1, frames, self.D, device=self.m.device) if quant is None else quant
        nf = C.c_int(0)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            self.m.engine._check(self.lib.fc_stream_encode(self.h, self._ptr(x), n, 0, self._ptr(codes), self._ptr(quant), None, C.byref(nf),
                                                           self._ptr(self.ws), self.ws.numel(), C.c_void_p(self.stream.cuda_stream)))
        torch.cuda.synchronize()
        assert nf.value == frames
        return codes, quant

    @property
    def fixed_in(self):
        if not hasattr(self, "_in"):
            self._in = torch.empty(1, 1, 32 * self.hop, device=self.m.device)
        return self._in.view(-1)[None, None]

    def stats(self):
        return self.st.graph_stats()


def test_a_pointer_change_is_a_miss():
    m = engine_for("tinywn", 5)
    e, g = RawStream(m, False), RawStream(m, True)
    dev = m.device
    outs = [(torch.empty(g.nq, 1, 1, dtype=torch.int64, device=dev), torch.empty(1, 1, g.D, device=dev)) for _ in range(2)]
    g.fixed_in
    want = [e.push(1) for _ in range(6)]
    got, stats = [], []
    for i in range(6):                                             # pushes 0 .. 3 into buffer pair 0 (both parities), then pair 1
        c, q = g.push(1, *outs[0 if i < 4 else 1])
        got.append((c.clone(), q.clone()))
        stats.append(g.stats())
    assert [s["captures"] for s in stats] == [1, 2, 2, 2, 3, 4] and [s["replays"] for s in stats] == [0, 0, 1, 2, 2, 2], stats
    assert stats[-1]["fallbacks"] == 0
    for a, b in zip(want, got):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    m.engine.check_status()


def test_the_least_recently_used_graph_is_evicted_and_a_width_seen_again_is_captured_afresh():
    m = engine_for("tinywn", 5)
    e, g = RawStream(m, False), RawStream(m, True)
    dev = m.device
    codes, quant = torch.empty(g.nq * 24, dtype=torch.int64, device=dev), torch.empty(24 * g.D, device=dev)
    g.fixed_in
    widths = list(range(1, 19)) + [1]                              # 18 distinct widths, then the first one again
    for i, w in enumerate(widths):
        want = e.push(w)
        before = g.stats()
        got = g.push(w, codes[:g.nq * w].view(g.nq, 1, w), quant[:w * g.D].view(1, w, g.D))
        after = g.stats()
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]), w
        assert after["captures"] == before["captures"] + 1 and after["replays"] == before["replays"], (i, w, after)
    n = g.stats()
    assert n["evictions"] == len(widths) - 16 and n["fallbacks"] == 0, n
    m.engine._check(g.lib.fc_graphstream_set(g.h, 0))              # off: the graphs go, the pushes go on eagerly
    want, got = e.push(2), g.push(2, codes[:g.nq * 2].view(g.nq, 1, 2), quant[:2 * g.D].view(1, 2, g.D))
    assert torch.equal(want[0], got[0]) and g.stats() == n
    m.engine.check_status()


# ---- 8. a failing push ----------------------------------------------------------------------------------------------------------------
def test_a_graphed_push_that_fails_poisons_every_slot_and_stores_no_graph():
    from funcodec_amd.engine import EngineError
    m = engine_for("tinywn", 5)
    hop, S = m.engine.hop_length, 2
    T = 20 * hop
    wavs = [audio(1, T, 71 + i, "tones") for i in range(S)]
    good = m.open_slots(S).encode({i: (w, True) for i, w in enumerate(wavs)})
    st = m.open_slots(S, graph=True)
    st.encode({0: wavs[0][..., :10 * hop], 1: wavs[1][..., :10 * hop]})
    before = st.graph_stats()
    keep = st._g.ws
    st._g.ws = torch.empty(8192, dtype=torch.uint8, device=m.device)          # a host-side failure behind the validation, inside the capture
    with pytest.raises(EngineError, match="workspace too small"):
        st.encode({0: wavs[0][..., 10 * hop:11 * hop]})
    st._g.ws = keep
    assert st.graph_stats() == before, "a failed push stores no graph and is no fallback"
    with pytest.raises(EngineError, match=r"start\(1\)"):
        st.encode({1: wavs[1][..., 10 * hop:11 * hop]})
    counts, ws = (C.c_int32 * S)(hop, hop), st._g.ws
    buf, codes = torch.zeros(S, 1, hop, device=m.device), torch.empty(st.n_q, S, 1, dtype=torch.int64, device=m.device)
    from funcodec_amd.engine import _ptr
    with pytest.raises(EngineError, match="restarted with START"):
        m.engine._check(m.engine.lib.fc_slots_encode(st._h, _ptr(buf), hop, counts, (C.c_int32 * S)(), None, _ptr(codes), None, None, _ptr(ws), ws.numel(),
                                                     m.engine._stream()))
    st.start(0)
    st.start(1)
    again = st.encode({i: (w, True) for i, w in enumerate(wavs)})
    for i in range(S):
        assert torch.equal(again[i][0], good[i][0]) and torch.equal(again[i][1], good[i][1])
    # and it replays afterwards
    st.start(0)
    for k in range(6):
        st.encode({0: wavs[0][..., (k + 9 if k else 0) * hop:(k + 10) * hop]})
    assert st.graph_stats()["replays"] > 0
    m.engine.check_status()


# ---- 9. neighbours --------------------------------------------------------------------------------------------------------------------
def test_a_graphed_session_an_eager_session_and_offline_calls_do_not_disturb_each_other():
    m = engine_for("tinywn", 5)
    hop, B, nfr = m.engine.hop_length, 2, 26
    a, b = audio(B, hop * nfr, 51, "tones"), audio(B, hop * nfr, 52, "noise")
    chunks = [12 * hop] + [hop] * (nfr - 12)

    def alone(wav, graph):
        st = m.open_stream(B, graph=graph)
        codes, quant, enc, _ = stream_encode(st, wav, chunks)
        return codes, quant, stream_decode(st, codes.permute(1, 2, 0).contiguous(), [12] + [1] * (nfr - 12))
    ra, rb = alone(a, True), alone(b, False)
    off_ref = m.engine.encode_decode(a, m.arch.num_quantizers)
    sg, se = m.open_stream(B, graph=True), m.open_stream(B)
    og, oe, pos = [], [], 0
    for i, n in enumerate(chunks):
        final = i == len(chunks) - 1
        cg, qg = sg.encode(a[..., pos:pos + n], final=final)
        off = m.engine.encode_decode(a, m.arch.num_quantizers)
        ce, qe = se.encode(b[..., pos:pos + n], final=final)
        wg = sg.decode(cg.permute(1, 2, 0).contiguous())
        we = se.decode(ce.permute(1, 2, 0).contiguous())
        assert torch.equal(off["codes"], off_ref["codes"]) and torch.equal(off["recon"], off_ref["recon"])
        og.append((cg, qg, wg)); oe.append((ce, qe, we))
        pos += n
    for outs, ref in ((og, ra), (oe, rb)):
        assert torch.equal(torch.cat([o[0] for o in outs], -1), ref[0]) and torch.equal(torch.cat([o[1] for o in outs], 1), ref[1])
        assert torch.equal(torch.cat([o[2] for o in outs], -1), ref[2])
    assert sg.graph_stats()["replays"] > 0 and sg.graph_stats()["fallbacks"] == 0
    m.engine.check_status()


# ---- 10. the process switch -----------------------------------------------------------------------------------------------------------
CHILD = """
import sys, torch
sys.path.insert(0, {tests!r})
from helpers import audio, engine_for
m = engine_for("tinywn", 5)
hop = m.engine.hop_length
wav = audio(1, 20 * hop, 97, "tones")
def run(st):
    return [st.encode(wav[..., :12 * hop])] + [st.encode(wav[..., i * hop:(i + 1) * hop]) for i in range(12, 20)]
sg = m.open_stream(1, graph=True)
eq = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(run(m.open_stream(1)), run(sg)))
sl = m.open_slots(2, graph=True)
for i in range(12, 18):
    sl.encode({{1: wav[0, (0 if i == 12 else i) * hop:(i + 1) * hop]}})
print("RESULT", int(sg.graph), int(sl.graph), eq, sg.graph_stats(), sl.graph_stats())
"""


def test_the_process_switch_keeps_graphed_sessions_eager():
    env = dict(os.environ, FC_SESSION_GRAPH="0")
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", CHILD.format(tests=here)], env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1]
    zero = "{'replays': 0, 'captures': 0, 'evictions': 0, 'fallbacks': 0}"
    assert line == f"RESULT 0 0 True {zero} {zero}", line
