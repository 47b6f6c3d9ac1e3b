"""CPU tests of the slot session (fc_slots_*, funcodec_amd.stream.StreamSlots): its C-ABI surface, what it refuses, the per-row staging
rule of a push restated in Python and checked against float64 torch on every conv of the causal tiny nets, and the wrapper's per-slot
hold-back logic against a stub library."""
import ctypes
import dataclasses
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from funcodec_amd import _lib
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.engine import EngineError
from funcodec_amd.stream import (FC_SLOT_FINAL, FC_SLOT_START, StreamSlots, conv_layers, min_first, slot_staged_width, stage_slot_row,
                                 stream_refusal)
from torch_oracle import sconv1d, sconvtr1d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT_CALLS = {"fc_slots_state_bytes", "fc_slots_create", "fc_slots_destroy", "fc_slots_min_first", "fc_slots_workspace_bytes",
              "fc_slots_encode", "fc_slots_decode_codes", "fc_slots_decode_emb", "fc_slots_lstm_forward"}


def test_slot_calls_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    declared = {n for n in re.findall(r"\b(fc_slots_[a-z_0-9]+)\s*\(", hdr)}
    bound = {n for n in _lib.SYMBOLS if n.startswith("fc_slots_")}
    assert declared == bound == SLOT_CALLS
    lib = ctypes.CDLL(_lib.lib_path())
    for name in SLOT_CALLS:
        assert hasattr(lib, name), name
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in SLOT_CALLS:       # one C parameter per ctypes argument
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, flat).group(1)
        assert len([p for p in params.split(",") if p.strip()]) == len(_lib.SYMBOLS[name][1]), name
    assert _lib.FC_ABI_VERSION == 7 and "#define FC_ABI_VERSION 7 " in hdr and _lib.load().fc_abi_version() == 7
    assert "#define FC_SLOT_START %d\n" % FC_SLOT_START in hdr and "#define FC_SLOT_FINAL %d\n" % FC_SLOT_FINAL in hdr


@pytest.mark.parametrize("name, change, key", [
    ("ds320", {}, "causal"),
    ("ss320tfc", {}, "seq_model: transformer"),
    ("ss320", {"model_type": "freq_codec"}, "freq_codec"),
    ("ss320", {"segment_dur": 0.5}, "model_conf.segment_dur"),
    ("ss320", {"q0_ds_ratio": 2}, "quantizer_conf.q0_ds_ratio"),
])
def test_a_slot_session_refuses_what_a_stream_refuses_and_names_the_key(name, change, key):
    arch = dataclasses.replace(arch_from_config(recipe_config(name)), **change)
    assert key in stream_refusal(arch)
    with pytest.raises(EngineError, match=re.escape(key)):
        StreamSlots(types.SimpleNamespace(arch=arch, engine=None), 4)      # refused before any engine call


def test_slots_of_a_non_causal_engine_are_refused_by_the_library_too():
    from funcodec_amd.engine import CodecEngine
    eng = CodecEngine(arch_from_config(recipe_config("tiny")))
    assert eng.lib.fc_slots_state_bytes(eng._h, 4) == 0


# ---- the per-row staging rule ------------------------------------------------------------------------------------------------------
def _schedule(n_first, cpf, tail):
    """Pushes of a 4-slot session at one layer, in columns of that layer.  Per push and slot: None (idle) or (utterance, columns, START, FINAL).
    Slot 0: one utterance with an idle push in its middle.  Slot 1: starts two pushes late, ends on a whole frame, and is reused after
    FINAL.  Slot 2: starts one push late and abandons its first utterance with START.  Slot 3: idle for long, then a whole utterance in
    one push.  `tail`: columns of the last push of the utterances that end ragged."""
    f = lambda frames: frames * cpf
    s0 = [("A", f(n_first), 1, 0), ("A", f(1), 0, 0), None, ("A", f(1), 0, 0), ("A", f(2), 0, 0), ("A", tail, 0, 1), None, None]
    s1 = [None, None, ("B", f(n_first + 2), 1, 0), ("B", f(3), 0, 0), ("B", f(1), 0, 1), ("C", f(n_first), 1, 0), None, ("C", tail, 0, 1)]
    s2 = [None, ("D", f(n_first), 1, 0), ("D", f(1), 0, 0), ("E", f(n_first + 1), 1, 0), None, ("E", f(1), 0, 0), ("E", tail, 0, 1), None]
    s3 = [None, None, None, None, None, None, ("F", f(n_first) + tail, 1, 1), None]
    return [list(p) for p in zip(s0, s1, s2, s3)]


@pytest.mark.parametrize("name", ["tinyss", "tinywn"])
def test_staged_rows_of_a_slot_push_equal_each_utterance_alone_in_float64(name):
    """Every conv and transposed conv of the net: the reference's causal layer on each whole utterance alone (torch_oracle.sconv1d /
    sconvtr1d in float64) against the same torch conv WITHOUT padding over the [S][cin][Tp] buffer that stage_slot_row builds push by
    push, rows START / continuing / FINAL (utterances of frames * columns-per-frame + {0, 1, cpf - 1} columns) / idle side by side.
    The abandoned utterance is checked up to where it was abandoned.  Channel counts are capped at 4 x 3 (the rule does not depend on
    them).  Bound: float64 rounding of sums of <= 64 products of O(1) values, 1e-12."""
    arch = arch_from_config(recipe_config(name))
    enc_first, dec_first = min_first(arch)
    hop = arch.hop_length
    gen = torch.Generator().manual_seed(13)
    checked = 0
    for L in conv_layers(arch):
        cin, cout, k, s, d, pt, cpf = min(L["cin"], 4), min(L["cout"], 3), L["k"], L["stride"], L["dil"], L["carry"], L["cols_per_frame"]
        tr = L["kind"] == "convtr"
        n_first = enc_first // hop if L["side"] == "encoder" else dec_first
        w = torch.randn((cin, cout, k) if tr else (cout, cin, k), generator=gen, dtype=torch.float64)
        b = torch.randn(cout, generator=gen, dtype=torch.float64)
        for tail in sorted({cpf, 1, max(1, cpf - 1)}):
            if L["side"] == "decoder" and tail % cpf:
                continue                                     # the decoder sees whole frames only
            sched = _schedule(n_first, cpf, tail)
            total = {}
            for push in sched:
                for op in push:
                    if op:
                        total[op[0]] = total.get(op[0], 0) + op[1]
            utt = {u: torch.randn(cin, n, generator=gen, dtype=torch.float64) for u, n in total.items()}
            pos, got = {u: 0 for u in utt}, {u: [] for u in utt}
            carry = [torch.full((cin, pt), float("nan"), dtype=torch.float64) for _ in range(4)]     # a START row must not read it
            for push in sched:
                T = max(op[1] for op in push if op)
                tp = slot_staged_width(L, T)
                rows = []
                for slot, op in enumerate(push):
                    row = utt[op[0]][:, pos[op[0]]:pos[op[0]] + op[1]] if op else torch.zeros(cin, 0, dtype=torch.float64)
                    staged, carry[slot] = stage_slot_row(L, carry[slot], row, bool(op and op[2]), bool(op and op[3]), tp)
                    assert staged.shape == (cin, tp)
                    rows.append(staged)
                buf = torch.stack(rows)
                assert bool(torch.isfinite(buf).all())
                y = F.conv_transpose1d(buf, w, b, stride=s)[..., s:s + T * s] if tr else F.conv1d(buf, w, b, stride=s, dilation=d)
                assert y.shape[-1] == (T * s if tr else -(-T // s))
                for slot, op in enumerate(push):
                    if not op:
                        assert float(buf[slot].abs().max()) == 0.0                # an idle row stages zeros
                        continue
                    u, n, start, final = op
                    n_out = n * s if tr else (-(-n // s) if final else n // s)
                    assert final or tr or n % s == 0
                    got[u].append(y[slot, :, :n_out])
                    pos[u] += n
            for u, x in utt.items():
                out = torch.cat(got[u], -1)
                seen = x[None, :, :pos[u]]
                want = (sconvtr1d(seen, w, b, None, None, s, 0.0, True) if tr else sconv1d(seen, w, b, None, None, s, 0.0, True, d))[0]
                if u == "D":                                 # abandoned: whole pushes only, so the reference's end padding is empty
                    assert pos[u] < total[u] + 1 and want.shape == out.shape
                assert out.shape == want.shape, (L, u, tail)
                assert float((out - want).abs().max()) < 1e-12, (L, u, tail)
                checked += 1
    assert checked >= 6 * len(conv_layers(arch))


# ---- the wrapper's per-slot logic against a stub library --------------------------------------------------------------------------------
class _StubLib:
    """records every fc_slots_* push (counts and flags per slot); computes nothing"""

    def __init__(self, enc_first, dec_first):
        self.first, self.pushes, self.fail_next, self.error = (enc_first, dec_first), [], [], ""

    def fc_slots_state_bytes(self, e, S): return 64 * S
    def fc_slots_create(self, e, S, max_chunk, n_q, state, nbytes, out): return 0
    def fc_slots_destroy(self, h): return None
    def fc_slots_min_first(self, h, decode): return self.first[decode]
    def fc_slots_workspace_bytes(self, h): return 256

    def fc_slots_encode(self, h, wav, Tc, counts, flags, scale, codes, quant, enc, ws, ws_bytes, stream):
        self.pushes.append(("encode", Tc, list(counts), list(flags), scale is not None))
        return 0

    def fc_slots_decode_codes(self, h, x, Tf, counts, flags, use_scale, wav, emb, ws, ws_bytes, stream):
        self.pushes.append(("decode", Tf, list(counts), list(flags), False))
        return 0

    def fc_slots_decode_emb(self, h, x, Tf, counts, flags, use_scale, wav, ws, ws_bytes, stream):
        self.pushes.append(("decode_emb", Tf, list(counts), list(flags), False))
        return self.fail_next.pop() if self.fail_next else 0


def _raise(msg):
    raise EngineError(msg)


def _stub_session(slots, max_chunk=None):
    arch = arch_from_config(recipe_config("tinywn"))
    hop = arch.hop_length
    lib = _StubLib(*min_first(arch))
    eng = types.SimpleNamespace(lib=lib, device=torch.device("cpu"), hop_length=hop, _h=None, _ws=None, channels=1,
                                _check=lambda rc: _raise(lib.error) if rc else None, _stream=lambda: None, frames=lambda n: -(-n // hop),
                                _dev=lambda t, dtype: t.to(dtype).contiguous())
    return StreamSlots(types.SimpleNamespace(arch=arch, engine=eng), slots, max_chunk=max_chunk), lib, hop


def test_each_slot_is_held_back_until_its_own_start_up_has_arrived_then_emits_everything_held():
    st, lib, hop = _stub_session(3)
    need = st.min_first_samples // hop
    assert need >= 3, "the test needs a start-up of several frames"
    w = lambda frames: torch.zeros(frames * hop)
    # slot 0 arrives a frame at a time, slot 1 in one push that is long enough, slot 2 two frames at a time starting one call later
    fed, emitted, started = [0, 0, 0], [0, 0, 0], set()
    for call in range(need + 2):
        pushes = {0: w(1)}
        if call == 0:
            pushes[1] = w(need + 1)
        if call >= 1:
            pushes[2] = w(2)
        for slot, x in pushes.items():
            fed[slot] += x.shape[-1] // hop
        n_before = len(lib.pushes)
        out = st.encode(pushes)
        for slot in range(3):
            if fed[slot] < need:
                assert slot not in out, (call, slot)                          # nothing before the start-up is complete
            elif slot in pushes:
                assert out[slot][0].shape[-1] == fed[slot] - emitted[slot]     # then everything held at once, later what was pushed
                emitted[slot] = fed[slot]
        if out:
            _, Tc, counts, flags, scaled = lib.pushes[-1]
            assert len(lib.pushes) == n_before + 1 and Tc == max(counts)
            for slot in range(3):
                assert counts[slot] == (out[slot][0].shape[-1] * hop if slot in out else 0)
                first = slot in out and slot not in started                    # START goes with the push that emits what was held
                assert flags[slot] == (FC_SLOT_START if first else 0), (call, slot)
                if first:
                    assert counts[slot] // hop == fed[slot]
                    started.add(slot)
        else:
            assert len(lib.pushes) == n_before
    assert emitted == fed and all(f >= need for f in fed)
    starts = [sum(1 for p in lib.pushes if p[3][slot] & FC_SLOT_START) for slot in range(3)]
    assert starts == [1, 1, 1]


def test_the_wrapper_splits_long_pushes_ends_and_restarts_slots_and_refuses_a_call_as_a_whole():
    st, lib, hop = _stub_session(2, max_chunk=None)
    st.max_chunk = 20 * hop
    need = st.min_first_samples
    out = st.encode({0: (torch.zeros(45 * hop + 3), True), 1: torch.zeros(need)})
    assert out[0][0].shape[-1] == 46 and out[1][0].shape[-1] == need // hop
    assert [(p[2], p[3]) for p in lib.pushes] == [([20 * hop, need], [FC_SLOT_START, FC_SLOT_START]), ([20 * hop, 0], [0, 0]),
                                                   ([5 * hop + 3, 0], [FC_SLOT_FINAL, 0])]
    n = len(lib.pushes)
    with pytest.raises(EngineError, match="final push"):                      # slot 0 has ended; slot 1's part of the call is not pushed either
        st.encode({1: torch.zeros(hop), 0: torch.zeros(hop)})
    with pytest.raises(EngineError, match="multiple of the hop"):
        st.encode({1: torch.zeros(hop + 1)})
    assert len(lib.pushes) == n
    st.start(0, scale=0.5)
    with pytest.raises(EngineError, match="fewer than"):                      # shorter than the start-up: the offline call's job
        st.encode({0: (torch.zeros(hop), True)})
    out = st.encode({0: (torch.zeros(need + 1), True), 1: torch.zeros(hop)})
    assert lib.pushes[-1][2:] == ([need + 1, hop], [FC_SLOT_START | FC_SLOT_FINAL, 0], True) and len(lib.pushes) == n + 1
    # decode: held back per slot in frames, FINAL passed on
    few = torch.zeros(st.min_first_frames - 1, st.n_q, dtype=torch.long)
    assert st.decode({1: few}) == {}
    with pytest.raises(EngineError, match="fewer than"):
        st.decode({0: (few, True)})
    got = st.decode({1: (torch.zeros(2, st.n_q, dtype=torch.long), True)})
    assert got[1].shape == (1, (st.min_first_frames + 1) * hop)
    assert lib.pushes[-1][:4] == ("decode", st.min_first_frames + 1, [0, st.min_first_frames + 1], [0, FC_SLOT_START | FC_SLOT_FINAL])


def test_decode_emb_goes_the_same_way_and_a_rule_refusal_of_the_library_undoes_the_call_while_a_failure_invalidates_every_slot():
    st, lib, hop = _stub_session(2)
    D, need = st.arch.dimension, st.min_first_frames
    st.start(1, scale=0.25)
    got = st.decode_emb({1: torch.zeros(need, D)})
    assert got[1].shape == (1, need * hop) and lib.pushes[-1][:4] == ("decode_emb", need, [0, need], [0, FC_SLOT_START])
    assert st.state[:8].view(torch.float32).tolist() == [0.0, 0.25]          # the scale of a slot that only decodes (the stub wrote no ones)
    # refused by a rule before the library's first launch, nothing of the call pushed: the wrapper is where it was
    lib.fail_next, lib.error = [1], "slot decode: slot 0: some rule"
    with pytest.raises(EngineError, match="some rule"):
        st.decode_emb({0: torch.zeros(need, D), 1: torch.zeros(1, D)})
    assert not st._dec[0].started and st._dec[1].started and st._poisoned == [False, False]
    st.decode_emb({0: torch.zeros(need, D), 1: torch.zeros(1, D)})
    assert lib.pushes[-1][2:4] == ([need, 1], [FC_SLOT_START, 0])
    # any other error: every slot must be restarted
    lib.fail_next, lib.error = [1], "workspace too small"
    with pytest.raises(EngineError, match="workspace"):
        st.decode_emb({0: torch.zeros(1, D)})
    with pytest.raises(EngineError, match=r"start\(1\)"):
        st.decode_emb({1: torch.zeros(1, D)})
    st.start(1)
    assert st.decode_emb({1: torch.zeros(need, D)})[1].shape == (1, need * hop)
