"""`-m gpu` tests of the slot record (csrc/slots_kernels.h states it; StreamSlots.export / import_slot / migrate, CodecStream.export,
fc_slotrec_*): a call in flight leaves its session and goes on in another one bit for bit.

The yardstick between sessions is torch.equal against ONE uninterrupted slot session fed the same pushes (computed once per net and
schedule and shared); the uninterrupted bits themselves are held to the oracle on the utterance alone with test_slots_gpu's bars.  For
the transformer net the oracle is oracle/torch_oracle.py's convs and quantiser with test_seq_transformer_gpu's float64 transformer at
the bottleneck.  The nets are the tiny causal ones (hop 8): their first conv carries cin * pt = 6 floats per slot, so odd slots are not
16-byte aligned, and the cache holds 7, 17, 33 frames (no multiple of 16) at pitches 48 and 112 (max_frames 40 against 100)."""
import functools

import pytest
import torch

from helpers import audio, engine_for, oracle_for
from test_seqstream_gpu import _tiny
from test_seqstream_host import causal_tinytf
from test_slots_gpu import Utt, assert_against_reference
from test_stream_gpu import pushes

from funcodec_amd.engine import EngineError
from funcodec_amd.stream import SlotRecord, min_first, slot_record_floats

pytestmark = pytest.mark.gpu
NAN = float("nan")
NETS = ["tinyss", "tinywn", "tinystwn", "tinytf"]
HOP = 8
T = 40 * HOP + 1
CACHE = [7, 10, 16, 7]                    # frames per push: the caches hold 7, 17, 33 and 40 frames


def model(net):
    return _tiny()[0] if net == "tinytf" else engine_for(net, 5)


@functools.lru_cache(maxsize=None)
def oracle(net):
    if net != "tinytf":
        return oracle_for(net, 5)
    from test_seq_transformer_gpu import transformer_f64
    from torch_oracle import Oracle
    m, sd = _tiny()

    class TfOracle(Oracle):
        """the reference's convs and quantiser, with TransformerEncoder (float64, causal, with the skip) where Oracle runs its SLSTM"""

        def _slstm(self, x, prefix):
            return transformer_f64(x.double(), sd, prefix[:-len(".lstm")], m.arch.lstm_layers, True, True).float()

    orc = TfOracle(causal_tinytf(), {k: torch.from_numpy(v) for k, v in sd.items()})
    orc.lstm_layers = m.arch.lstm_layers
    return orc


def slots(net, S, max_frames=48, **kw):
    m = model(net)
    return m.open_slots(S, max_frames=max_frames, **kw) if net == "tinytf" else m.open_slots(S, **kw)


@functools.lru_cache(maxsize=None)
def material(net, seed):
    """(wav [C,T], scale, the oracle's result on the utterance alone), computed once"""
    m = model(net)
    wav = audio(1, T, seed, "tones", m.engine.channels)
    ref = oracle(net).inference(wav, bit_width=None, use_scale=True)
    return (wav[0] if wav.dim() == 3 else wav), ref["scale"], ref


def chunks(how):
    return [f * HOP for f in CACHE] + [1] if how == "cache" else pushes(T, HOP, how)


def utt(net, seed=400, how="mixed"):
    wav, scale, _ = material(net, seed)
    return Utt(wav, scale, chunks(how))


def push(st, items, decode=True):
    """one round: step i of every named utterance {slot: (Utt, i)} in ONE encode push, every emitted frame decoded in the same round"""
    enc = {}
    for slot, (u, i) in items.items():
        n = u.steps[i]
        enc[slot] = (u.wav[..., u.pos:u.pos + n], i == len(u.steps) - 1)
        u.pos += n
    out = st.encode(enc, want_enc_out=True)
    dec = {}
    for slot, (c, q, e) in out.items():
        u = items[slot][0]
        u.codes.append(c); u.quant.append(q); u.enc.append(e)
        dec[slot] = (c.t().contiguous(), enc[slot][1])
    if decode and dec:
        for slot, w in st.decode(dec).items():
            items[slot][0].rec.append(w)
    return bool(out)


def run(st, slot, u, lo, hi):
    if lo == 0:
        st.start(slot, u.scale)
    return sum(push(st, {slot: (u, i)}) for i in range(lo, hi))


def fork(u):
    """the utterance as far as it has come, for a second session to continue"""
    v = Utt(u.wav, u.scale, [n for n in u.steps])
    v.pos, v.codes, v.quant, v.enc, v.rec = u.pos, list(u.codes), list(u.quant), list(u.enc), list(u.rec)
    return v


@functools.lru_cache(maxsize=None)
def baseline(net, seed=400, how="mixed"):
    """ONE uninterrupted session fed the utterance's pushes: (codes, quantized, enc_out, wav), held to the oracle here, once"""
    u = utt(net, seed, how)
    run(slots(net, 1), 0, u, 0, len(u.steps))
    ref = material(net, seed)[2]
    assert_against_reference(f"{net} [{how}] uninterrupted", model(net).arch, u, ref["code_indices"][0].numpy(), ref["encoder_out"],
                             ref["code_embeddings"][0][0], ref["recon_speech"])
    return u.cat()


def same(u, base, tag=""):
    got = u.cat()
    for name, a, b in zip(("codes", "quantized", "enc_out", "wav"), got, base):
        assert a.shape == b.shape and torch.equal(a, b), (tag, name)


def first_emitting(net, how="mixed"):
    """index of the push that takes the utterance past its start-up: from there on both sides are Running"""
    need, have = min_first(model(net).arch)[0], 0
    for i, n in enumerate(chunks(how)):
        have += n
        if have >= need:
            return i
    raise AssertionError


def crowd(net, dst, among, parity):
    """the other slots of `dst` mid-utterance: the same filler in every slot of `among`, driven until the session's push counters have
    the parity asked for (one library push per emitting round).  Returns the fillers and the next step of each."""
    fill = {slot: utt(net, 411) for slot in among}
    for slot, f in fill.items():
        dst.start(slot, f.scale)
    i = emitted = 0
    while emitted < 2 or emitted % 2 != parity:
        emitted += push(dst, {slot: (f, i) for slot, f in fill.items()})
        i += 1
    return fill, i


def finish(st, slot, u, lo, fill=None, fi=0):
    """the utterance from step lo to its FINAL push, the fillers going on beside it in the same pushes while they last"""
    for i in range(lo, len(u.steps)):
        items = {slot: (u, i)}
        for s, f in (fill or {}).items():
            if fi < len(f.steps):
                items[s] = (f, fi)
        fi += 1
        push(st, items)
    while fill and fi < len(next(iter(fill.values())).steps):
        push(st, {s: (f, fi) for s, f in fill.items()})
        fi += 1


# ---- 1. continuation, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,where", [(n, "middle") for n in NETS] + [("tinytf", "first"), ("tinytf", "all_but_one")])
def test_a_call_exported_mid_utterance_continues_in_another_session_bit_for_bit(net, where):
    """slot 1 of 3 -> slot 4 of 5 whose other slots are mid-utterance and whose push counters stand at the other parity; the transformer
    net from max_frames 40 (pitch 48) to 100 (pitch 112), after its first push past the start-up (9 frames), in the middle (20) and
    with one push to go (40)"""
    base = baseline(net)
    u = utt(net)
    i0 = first_emitting(net)
    k = {"first": i0 + 1, "middle": i0 + 4, "all_but_one": len(u.steps) - 1}[where]
    src = slots(net, 3, max_frames=40)
    emitted = run(src, 1, u, 0, k)
    assert emitted >= 1 and u.rec
    dst = slots(net, 5, max_frames=100)
    fill, fi = crowd(net, dst, [0, 1, 2, 3], (emitted + 1) % 2)
    rec = src.export(1)
    assert rec.floats is not None and rec.meta[1:3] == (1, 1) and not torch.isnan(rec.floats).any()
    assert rec.floats.numel() == model(net).engine.lib.fc_slotrec_floats(src._h, rec.meta[3], rec.meta[4])
    dst.import_slot(4, rec)
    finish(dst, 4, u, k, fill, fi)
    same(u, base, (net, where))
    for s, f in fill.items():                          # the import touched no other slot's floats
        same(f, baseline(net, 411), (net, where, "filler", s))
    model(net).engine.check_status()


# ---- 2. the record is canonical -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS)
def test_the_record_is_a_function_of_the_pushes_alone(net):
    """the same pushes in slot 1 of 3 (eager, max_frames 40) and in slot 4 of 5 (graph replay, max_frames 100, one push ahead in
    parity, a filler running in slot 0), every float of both states NaN before anything starts: the records after every push -- at 7,
    17, 33 and 40 cached frames -- are equal bit for bit and hold no NaN, and the metas are equal"""
    a, b = slots(net, 3, max_frames=40), slots(net, 5, max_frames=100, graph=True)
    for st in (a, b):
        st.state.view(torch.float32).fill_(NAN)        # every other slot's rows stay NaN: a slot writes what it reads
    ua, ub, f = utt(net, how="cache"), utt(net, how="cache"), utt(net, 411, "cache")
    b.start(0, f.scale)
    push(b, {0: (f, 0)})                               # b's counters are one push ahead: the other parity
    a.start(1, ua.scale)
    b.start(4, ub.scale)
    for i, frames in enumerate([7, 17, 33, 40]):
        push(a, {1: (ua, i)})
        push(b, {4: (ub, i), 0: (f, i + 1)})
        ra, rb = a.export(1), b.export(4)
        assert ra.meta == rb.meta and ra.meta[1:3] == (1, 1), (net, frames)
        assert ra.meta[3:] == ((frames, frames) if net == "tinytf" else (0, 0))
        assert not torch.isnan(ra.floats).any() and torch.equal(ra.floats, rb.floats), (net, frames)
        assert ra.floats.numel() == slot_record_floats(model(net).arch, *ra.meta[3:], net == "tinytf")
    assert b.graph_stats()["fallbacks"] == 0
    model(net).engine.check_status()


# ---- 3. the source is undisturbed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["tinywn", "tinytf"])
def test_after_an_export_the_source_and_the_copy_both_run_on_to_the_same_bits(net):
    base = baseline(net)
    u = utt(net)
    k = first_emitting(net) + 3
    src, dst = slots(net, 2), slots(net, 3, max_frames=64)
    run(src, 1, u, 0, k)
    rec = src.export(1)
    v = fork(u)
    dst.import_slot(2, rec)
    for i in range(k, len(u.steps)):                   # alternating, so that neither waits for the other
        push(src, {1: (u, i)})
        push(dst, {2: (v, i)})
    same(u, base, (net, "source"))
    same(v, base, (net, "copy"))
    model(net).engine.check_status()


# ---- 4. through host bytes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["tinyss", "tinytf"])
def test_a_record_through_host_bytes_continues_bit_for_bit(net):
    base = baseline(net, how="cache")
    u = utt(net, how="cache")
    src = slots(net, 2, max_frames=40)
    run(src, 0, u, 0, 1)
    short = src.export(0).to_bytes()                   # 7 frames
    run(src, 0, u, 1, 3)
    blob = src.export(0).to_bytes()                    # 33 frames
    rec = SlotRecord.from_bytes(blob, device=model(net).device)
    dst = slots(net, 2, max_frames=100)
    dst.import_slot(1, rec)
    finish(dst, 1, u, 3)
    same(u, base, net)
    if net == "tinytf":                                # the bytes follow the frames held, not max_frames
        wide = slots(net, 1, max_frames=100)
        w = utt(net, how="cache")
        run(wide, 0, w, 0, 1)
        assert len(wide.export(0).to_bytes()) == len(short)
        planes = 2 * 2 * 2 * 64                        # sides x blocks x (K, V) x C floats per cached frame column
        assert rec.floats.numel() - SlotRecord.from_bytes(short).floats.numel() == planes * (48 - 16)
        assert 0 <= len(blob) - len(short) - 4 * planes * (48 - 16) < 16          # the header names the frames: a few digits more
    else:
        assert rec.floats.numel() == SlotRecord.from_bytes(short).floats.numel() and abs(len(blob) - len(short)) < 16
    model(net).engine.check_status()


# ---- 5. many slots in one launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["tinywn", "tinytf"])
def test_migrate_moves_every_running_slot_into_permuted_slots_and_one_slot_alone(net):
    base = baseline(net)
    i0 = first_emitting(net)
    src, dst = slots(net, 4, max_frames=40), slots(net, 8, max_frames=100)
    us = [utt(net) for _ in range(4)]
    at = [0, 0, 0, 0]                                  # the next step of each: slot j starts j rounds late, so the four states differ
    for r in range(i0 + 5):
        items = {}
        for j in range(4):
            if r >= j:
                if r == j:
                    src.start(j, us[j].scale)
                items[j] = (us[j], at[j])
                at[j] += 1
        push(src, items)
    assert all(u.rec for u in us)
    perm = {0: 5, 1: 2, 2: 7, 3: 0}
    src.migrate(dst, perm)
    for step in range(len(us[0].steps)):
        items = {perm[j]: (us[j], at[j] + step) for j in range(4) if at[j] + step < len(us[j].steps)}
        if items:
            push(dst, items)
    for j, u in enumerate(us):
        same(u, base, (net, "migrate 4", j))
    # n = 1: one running slot of a fresh pair
    one = utt(net)
    src2, dst2 = slots(net, 3, max_frames=40), slots(net, 4, max_frames=100)
    run(src2, 2, one, 0, i0 + 2)
    src2.migrate(dst2, {2: 3})
    finish(dst2, 3, one, i0 + 2)
    same(one, base, (net, "migrate 1"))
    model(net).engine.check_status()


# ---- 6. start-up held, an ended encoder, a slot that only decodes --------------------------------------------------------------------
@pytest.mark.parametrize("net", ["tinywn", "tinytf"])
def test_a_slot_still_gathering_its_start_up_travels_as_its_held_pieces(net):
    base = baseline(net, how="frames1")
    u = utt(net, how="frames1")
    src, dst = slots(net, 2), slots(net, 3)
    assert run(src, 1, u, 0, 3) == 0                   # 3 of the 7 start-up frames: nothing has reached the library
    rec = src.export(1)
    assert rec.floats is None and rec.meta is None and len(rec.enc.head) == 3 and not rec.enc.started
    dst.import_slot(0, SlotRecord.from_bytes(rec.to_bytes(), device=model(net).device))
    finish(dst, 0, u, 3)
    same(u, base, net)
    model(net).engine.check_status()


@pytest.mark.parametrize("net", ["tinywn", "tinytf"])
def test_an_ended_encoder_beside_a_running_decoder_and_a_slot_that_only_decodes(net):
    """the decoder side alone is Running: after the encoder's FINAL push (phase ended), and in a slot whose encoder never started
    (phase idle); the encoder side of both records holds 0 frames and zeros"""
    codes, _, _, wav = baseline(net)
    u = utt(net)
    tokens = codes.t().contiguous()                    # [Tf, n_q]
    cut, Tf = 20, codes.shape[-1]
    # a: encode everything, decode the first 20 frames, move, decode the rest
    src, dst = slots(net, 2), slots(net, 3, max_frames=64)
    src.start(0, u.scale)
    for i in range(len(u.steps)):
        push(src, {0: (u, i)}, decode=False)
    head = src.decode({0: tokens[:cut]})[0]
    rec = src.export(0)
    assert rec.meta[1:3] == (2, 1) and rec.meta[3] == 0 and rec.enc.ended
    dst.import_slot(2, rec)
    tail = dst.decode({2: (tokens[cut:], True)})[2]
    # b: a session that only decodes, the scale given at start
    only, other = slots(net, 2), slots(net, 2, max_frames=64)
    only.start(1, u.scale)
    head_b = only.decode({1: tokens[:cut]})[1]
    rec_b = only.export(1)
    assert rec_b.meta[1:3] == (0, 1) and rec_b.meta[3] == 0
    other.import_slot(0, rec_b)
    tail_b = other.decode({0: (tokens[cut:], True)})[0]
    # the yardstick: ONE session decoding the same two pushes
    ref = slots(net, 1)
    ref.start(0, u.scale)
    want = torch.cat([ref.decode({0: tokens[:cut]})[0], ref.decode({0: (tokens[cut:], True)})[0]], -1)
    assert want.shape == wav.shape
    assert torch.equal(torch.cat([head, tail], -1), want) and torch.equal(torch.cat([head_b, tail_b], -1), want)
    n_enc = {"tinywn": 326 + 128, "tinytf": 646}[net]  # the encoder side's floats (test_slot_record_host counts them): zeros in both records
    assert not rec.floats[1:1 + n_enc].any() and not rec_b.floats[1:1 + n_enc].any() and rec.floats[1 + n_enc:].any()
    assert torch.equal(rec.floats[1:], rec_b.floats[1:])
    assert torch.equal(rec.floats[:1].cpu(), torch.tensor([float(torch.as_tensor(u.scale).reshape(-1)[0])], dtype=torch.float32))
    model(net).engine.check_status()


# ---- 7. into a session that replays graphs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["tinywn", "tinytf"])
def test_an_import_into_a_replaying_session_keeps_it_replaying(net):
    base = baseline(net, how="frames1")
    u, f = utt(net, how="frames1"), utt(net, 411, "frames1")
    k = first_emitting(net, "frames1") + 6
    src = slots(net, 2, max_frames=40)
    run(src, 0, u, 0, k)
    dst = slots(net, 3, max_frames=100, graph=True)
    assert dst.graph
    dst.start(1, f.scale)
    fi = 0
    for fi in range(first_emitting(net, "frames1") + 5):   # one-frame pushes at both parities: their graphs are captured and replay
        push(dst, {1: (f, fi)})
    fi += 1
    before = dst.graph_stats()
    assert before["replays"] >= 2
    dst.import_slot(2, src.export(0))
    for i in range(k, len(u.steps) - 1):               # the steady pushes: the FINAL one has a width of its own
        push(dst, {2: (u, i), 1: (f, fi)})
        fi += 1
    after = dst.graph_stats()
    assert after["captures"] - before["captures"] <= 2 and after["fallbacks"] == 0, (before, after)
    assert after["replays"] - before["replays"] >= 2 * (len(u.steps) - 1 - k) - 2, (before, after)
    push(dst, {2: (u, len(u.steps) - 1)})
    same(u, base, net)
    model(net).engine.check_status()


# ---- 8. the stage count and the noise floor travel ------------------------------------------------------------------------------------------
def test_a_slots_stage_count_and_noise_floor_travel_and_more_stages_than_the_session_are_refused():
    net = "tinywn"
    m = model(net)
    wav, scale, _ = material(net, 400)
    steps = chunks("mixed")

    def packets(move_at):
        st = slots(net, 2)
        st.start(1, scale, n_q=2, noise_floor_db=-12.0)
        slot, pos, out = 1, 0, []
        for i, n in enumerate(steps):
            if i == move_at:
                rec = st.export(1)
                assert rec.n_q == 2 and rec.noise_floor_db == -12.0
                st, slot = slots(net, 3), 2
                st.import_slot(slot, rec)
                assert st._row_nq[slot] == 2 and st._floor_db[slot] == -12.0 and st.n_q == 6
            res, pk = st.encode({slot: (wav[..., pos:pos + n], i == len(steps) - 1)}, packed=True)
            pos += n
            out.append((pk.get(slot), res[slot][0] if slot in res else None))
        return out

    want, got = packets(None), packets(first_emitting(net) + 2)
    assert len(want) == len(got) and any(p for p, _ in want)
    for (p0, c0), (p1, c1) in zip(want, got):
        assert p0 == p1 and (c0 is None) == (c1 is None) and (c0 is None or torch.equal(c0, c1))
    narrow = m.open_slots(2, n_q=1)
    src = slots(net, 1)
    u = utt(net)
    src.start(0, u.scale, n_q=2)
    for i in range(first_emitting(net) + 2):
        push(src, {0: (u, i)})
    with pytest.raises(EngineError, match=r"slot 1: the record's n_q = 2 exceeds this session's n_q = 1"):
        narrow.import_slot(1, src.export(0))
    m.engine.check_status()


# ---- 9. refusals change nothing -------------------------------------------------------------------------------------------------------
def _record_of(net, steps, **kw):
    st = slots(net, 2, **kw)
    u = utt(net)
    run(st, 1, u, 0, steps)
    return st, st.export(1)


def test_a_refused_import_or_export_names_its_rule_and_changes_nothing():
    i0 = first_emitting("tinyss")
    assert i0 == first_emitting("tinytf") == first_emitting("tinywn") == 2
    _, rec_wn = _record_of("tinywn", 5)
    _, rec_ss = _record_of("tinyss", 5)
    _, rec_tf = _record_of("tinytf", 6, max_frames=40)                       # 20 frames
    assert rec_tf.meta[3:] == (20, 20)
    for net, dst_kw, calls in [
            ("tinyss", {}, [(rec_wn, r"slot 1: .*layout"), (rec_tf, r"slot 1: the record holds a key / value cache and this session has none")]),
            ("tinytf", {"max_frames": 16}, [(rec_tf, r"slot 1: .*20 frames, past the session's max_frames = 16"),
                                            (rec_ss, r"slot 1: the record holds no key / value cache and this session has one")])]:
        codes, quant, enc, wav = baseline(net)
        dst = slots(net, 3, **dst_kw)
        u = utt(net)
        run(dst, 0, u, 0, 3)                           # slot 0 is running (9 frames)
        own = dst.export(0)
        for rec, pattern in calls:
            with pytest.raises(EngineError, match=pattern):
                dst.import_slot(1, rec)
        buf = own.floats.reshape(1, -1)
        two = torch.cat([buf, buf], 0)
        with pytest.raises(EngineError, match=r"slot import: slot 1: named twice"):
            dst._import_rows([1, 1], two, [own.meta, own.meta])
        with pytest.raises(EngineError, match=r"slot import: slot 2: pitch_floats = \d+ is too small"):
            dst._import_rows([2], buf[:, :-4].contiguous(), [own.meta])
        with pytest.raises(EngineError, match=r"slot import: slot 3: out of range"):
            dst._import_rows([3], buf, [own.meta])
        with pytest.raises(EngineError, match=r"names 1 \.\. 3 slots"):
            dst._import_rows([0, 1, 2, 1], torch.cat([two, two], 0), [own.meta] * 4)
        assert not any(dst._poisoned) and not dst._enc[1].started and not dst._enc[2].started
        push(dst, {0: (u, 3)})
        push(dst, {0: (u, 4)})                         # the running slot goes on bit for bit: its pushes 3 and 4 are the uninterrupted ones
        got = u.cat()
        n = got[0].shape[-1]
        assert n == 12 and torch.equal(got[0], codes[:, :n]) and torch.equal(got[1], quant[:n]) and torch.equal(got[2], enc[:n])
        assert torch.equal(got[3], wav[..., :n * HOP])
        model(net).engine.check_status()


def test_a_slot_that_a_failed_push_invalidated_is_not_exported():
    m = model("tinywn")
    st = slots("tinywn", 2)
    u, v = utt("tinywn"), utt("tinywn", 411)
    st.start(0, u.scale)
    st.start(1, v.scale)
    for i in range(3):
        push(st, {0: (u, i), 1: (v, i)})
    rec = st.export(0)                                 # while it is sound
    w = fork(u)
    keep_ws, keep_need = m.engine._ws, st._ws_bytes
    m.engine._ws, st._ws_bytes = torch.empty(8192, dtype=torch.uint8, device=m.device), 8192
    with pytest.raises(EngineError, match="workspace too small"):            # a host-side failure behind the validation (test_slots_gpu)
        push(st, {0: (u, 3)})
    m.engine._ws, st._ws_bytes = keep_ws, keep_need
    with pytest.raises(EngineError, match=r"slot 1: .*not exported"):          # the wrapper
        st.export(1)
    with pytest.raises(EngineError, match=r"slot export: slot 1: .*not exported"):      # the library
        st._export_rows(m.engine.lib.fc_slotrec_export, [1], [(st._enc[1], st._dec[1])])
    with pytest.raises(EngineError, match="takes no record"):
        st.import_slot(1, rec)
    st.start(0)
    st.start(1)
    st.import_slot(1, rec)                             # restarted, the session takes records again
    finish(st, 1, w, 3)
    same(w, baseline("tinywn"), "after the restart")
    m.engine.check_status()


# ---- 10. a lock-step row as a slot record ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["tinystwn", "tinytf"])
def test_a_row_of_a_lock_step_stream_continues_in_a_slot(net):
    m = model(net)
    wavs = [material(net, seed) for seed in (400, 411)]
    x = torch.stack([w for w, _, _ in wavs])           # [2, C, T]
    scale = torch.tensor([float(torch.as_tensor(s).reshape(-1)[0]) for _, s, _ in wavs])
    steps = chunks("mixed")
    k = first_emitting(net) + 3

    def lockstep(stop):
        st = m.open_stream(2, scale=scale, max_frames=48) if net == "tinytf" else m.open_stream(2, scale=scale)
        out, pos = [], 0
        for i, n in enumerate(steps[:stop]):
            c, q, e = st.encode(x[..., pos:pos + n], final=i == len(steps) - 1, want_enc_out=True)
            pos += n
            w = st.decode(c.permute(1, 2, 0).contiguous()) if c.shape[-1] else None
            out.append((c, q, e, w))
        return st, out, pos

    _, whole, _ = lockstep(len(steps))
    st, part, pos = lockstep(k)
    rec = st.export(1)
    assert rec.meta[1:3] == (1, 1) and rec.scale == float(scale[1])
    dst = slots(net, 3, max_frames=100)
    dst.import_slot(2, rec)
    u = Utt(wavs[1][0], wavs[1][1], steps)
    u.pos = pos
    finish(dst, 2, u, k)
    got = u.cat()
    cat = lambda outs, j, dim: torch.cat([o[j][:, 1] if j == 0 else o[j][1] for o in outs if o[3] is not None], dim)
    # against the uninterrupted stream, every output bit for bit: the record carries the row's state whole, and a slot push runs the
    # lock-step push's kernels in the same form on it
    for j, (name, dim) in enumerate((("codes", -1), ("quantized", 0), ("enc_out", 0), ("wav", -1))):
        assert torch.equal(got[j], cat(whole[k:], j, dim)), (net, name)
    # the whole utterance, its first pushes from the stream and the rest from the slot, against the oracle on the utterance alone
    v = Utt(wavs[1][0], wavs[1][1], steps)
    v.codes, v.quant, v.enc, v.rec = [cat(part, 0, -1), got[0]], [cat(part, 1, 0), got[1]], [cat(part, 2, 0), got[2]], [cat(part, 3, -1), got[3]]
    ref = wavs[1][2]
    assert_against_reference(f"{net} stream row -> slot", m.arch, v, ref["code_indices"][0].numpy(), ref["encoder_out"], ref["code_embeddings"][0][0],
                             ref["recon_speech"])
    assert torch.equal(torch.cat(v.codes, -1), baseline(net, 411)[0])
    m.engine.check_status()


def test_a_lock_step_row_still_gathering_its_start_up_travels_as_its_own_pieces():
    """CodecStream.export of a row before anything has reached the library: the record is the ROW's slice of the held pieces, its scale
    and its stage count; continued in a slot it is the uninterrupted slot session's utterance bit for bit"""
    net = "tinystwn"
    m = model(net)
    wavs = [material(net, seed) for seed in (400, 411)]
    x = torch.stack([w for w, _, _ in wavs])
    scale = torch.tensor([float(torch.as_tensor(s).reshape(-1)[0]) for _, s, _ in wavs])
    steps = chunks("frames1")
    st = m.open_stream(2, scale=scale, n_q=[6, 3])
    for i in range(3):                                 # 3 of the 7 start-up frames
        assert st.encode(x[..., i * HOP:(i + 1) * HOP])[0].shape[-1] == 0
    rec = st.export(1)
    assert rec.floats is None and rec.meta is None and rec.n_q == 3 and rec.scale == float(scale[1])
    assert len(rec.enc.head) == 3 and all(torch.equal(p.cpu(), wavs[1][0][..., i * HOP:(i + 1) * HOP]) for i, p in enumerate(rec.enc.head))
    dst = slots(net, 2)
    dst.import_slot(1, rec)
    dst.set_n_q(1, 6)                                  # the count travelled (asserted above); the yardstick runs all six stages
    u = Utt(wavs[1][0], wavs[1][1], steps)
    u.pos = 3 * HOP
    finish(dst, 1, u, 3)
    same(u, baseline(net, 411, "frames1"), net)
    m.engine.check_status()


@pytest.mark.parametrize("net", ["tinywn", "tinytf"])
def test_migrate_inside_one_session_exchanges_two_running_slots(net):
    """dst is the session itself and each destination is the other pair's source: every record is exported before any is imported and
    the wrapper's state is taken before any slot adopts, so the two calls change places and go on bit for bit"""
    base = baseline(net)
    i0 = first_emitting(net)
    ss = slots(net, 3, max_frames=48)
    a, b = utt(net), utt(net)
    run(ss, 0, a, 0, i0 + 1)
    ss.start(2, b.scale)
    for i in range(i0 + 3):                            # b runs beside a, two pushes behind
        push(ss, {0: (a, i0 + 1 + i), 2: (b, i)} if i0 + 1 + i < len(a.steps) else {2: (b, i)})
    na, nb = 2 * i0 + 4, i0 + 3
    assert ss._enc[0].frames != ss._enc[2].frames
    ss.migrate(ss, {0: 2, 2: 0})
    assert (ss._enc[2].frames, ss._enc[0].frames) == (sum(a.steps[:na]) // HOP, sum(b.steps[:nb]) // HOP)
    for step in range(len(b.steps) - nb):
        items = {0: (b, nb + step)}
        if na + step < len(a.steps):
            items[2] = (a, na + step)
        push(ss, items)
    same(a, base, (net, "a, now in slot 2"))
    same(b, base, (net, "b, now in slot 0"))
    model(net).engine.check_status()
