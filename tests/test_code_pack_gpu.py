"""The codec's bit stream on the MI355X (csrc/code_pack_kernels.h states the packet): fc_codes_pack / fc_codes_unpack against a
restatement in Python integers over every tile edge, then the packets of the offline calls, both session kinds and the CLI against the
codes and the decode calls there are.  Every comparison is exact."""
import ctypes as C
import functools
import os
import struct

import numpy as np
import pytest
import torch

from funcodec_amd import _lib, io as fio
from funcodec_amd.engine import EngineError
from helpers import audio, engine_for

pytestmark = pytest.mark.gpu
BITS = (1, 6, 7, 8, 10, 16)
COUNTS = (1, 3, 8, 32)
FRAMES = (1, 2, 31, 32, 33, 63, 64, 65, 130)
NAN_BITS = 0x7FF8000000000000
GARBAGE = (-1, (1 << 40) + 5)
BW = 12000.0          # one stage of the tiny quantisers: log2(64) bits x 16000 / 8 frames per second


# ---- the restatement and the two calls ---------------------------------------------------------------------------------------------------
def payload_int(codes, b, frames, k, bits):
    mask = (1 << bits) - 1
    return sum((int(codes[i, b, t]) & mask) << ((t * k + i) * bits) for t in range(frames) for i in range(k))


def restate_row(codes, b, frames, k, bits, pitch=None):
    """the packet of row b of codes [n_q, B, Tf] (numpy) in Python integers, zero-filled to the pitch if one is given"""
    p = struct.pack("<IBBBB", frames, k, bits, 0, 0) + payload_int(codes, b, frames, k, bits).to_bytes((frames * k * bits + 7) // 8, "little")
    return p if pitch is None else p + bytes(pitch - len(p))


def restate(codes, frames_rows, n_q_rows, bits, pitch):
    return np.frombuffer(b"".join(restate_row(codes, b, f, k, bits, pitch) for b, (f, k) in enumerate(zip(frames_rows, n_q_rows))),
                         dtype=np.uint8).reshape(len(frames_rows), pitch)


def _i32(rows):
    return None if rows is None else torch.tensor(rows, dtype=torch.int32, device="cuda")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def pack(codes, bits, frames_rows=None, n_q_rows=None, fill=0xFF):
    """fc_codes_pack of codes [n_q, B, Tf] (a device tensor) into a buffer pre-filled with `fill` -> uint8 [B, pitch] on the host"""
    lib = _lib.load()
    n_q, B, Tf = codes.shape
    pitch = lib.fc_code_packet_pitch(Tf, n_q, bits)
    out = torch.full((B, pitch), fill, dtype=torch.uint8, device="cuda")
    fr, nq = _i32(frames_rows), _i32(n_q_rows)
    rc = lib.fc_codes_pack(_p(codes), B, Tf, n_q, bits, _p(fr), _p(nq), _p(out), pitch, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def unpack(packets, Tf, n_q, bits, guard=4096):
    """fc_codes_unpack of uint8 [B, pitch] (numpy) into a buffer pre-filled with -1 with a guard region behind it, which must stay -1"""
    lib = _lib.load()
    dev = torch.from_numpy(np.ascontiguousarray(packets)).cuda()
    B, pitch = dev.shape
    n = B * Tf * n_q
    flat = torch.full((n + guard,), -1, dtype=torch.int64, device="cuda")
    rc = lib.fc_codes_unpack(_p(dev), pitch, B, Tf, n_q, bits, _p(flat), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    flat = flat.cpu()
    assert bool((flat[n:] == -1).all()), "the guard region behind the tokens was written"
    return flat[:n].view(B, Tf, n_q)


def tokens_of(codes, frames_rows, n_q_rows):
    """codes [n_q, B, Tf] -> [B, Tf, n_q] with zeros behind every row's count and frames"""
    tok = torch.as_tensor(codes).permute(1, 2, 0).clone()
    for b, (f, k) in enumerate(zip(frames_rows, n_q_rows)):
        tok[b, f:] = 0
        tok[b, :, k:] = 0
    return tok


def seeded(bits, n_q, B, Tf, seed=0):
    return np.random.default_rng(100000 * bits + 1000 * n_q + 10 * Tf + B + seed).integers(0, 1 << bits, (n_q, B, Tf), dtype=np.int64)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_pack_and_unpack_against_python_integers_over_every_tile_edge(bits):
    for n_q in COUNTS:
        for Tf in FRAMES:
            for B in (1, 3):
                codes = seeded(bits, n_q, B, Tf)
                dev = torch.from_numpy(codes).cuda()
                # rows with frames 1 and Tf and counts 1 and n_q in one batch; B = 1: the whole row
                frames = [Tf] if B == 1 else [1, Tf, (Tf + 1) // 2]
                counts = [n_q] if B == 1 else [n_q, 1, (n_q + 1) // 2]
                got = pack(dev, bits, frames, counts)
                want = restate(codes, frames, counts, bits, got.shape[1])
                assert got.shape[1] % 16 == 0 and np.array_equal(got, want), (bits, n_q, Tf, B)      # the whole buffer, zero tail included
                if B == 1:                      # null and given rows agree when they say the same
                    assert np.array_equal(pack(dev, bits), got) and np.array_equal(pack(dev, bits, frames, None), got)
                    assert np.array_equal(pack(dev, bits, None, counts), got)
                tok = unpack(got, Tf, n_q, bits)
                assert torch.equal(tok, tokens_of(codes, frames, counts)), (bits, n_q, Tf, B)


@pytest.mark.parametrize("bits,n_q,Tf", [(10, 32, 130), (7, 3, 65), (16, 8, 64), (1, 32, 33)])
def test_garbage_behind_frames_and_count_does_not_reach_a_byte(bits, n_q, Tf):
    clean = seeded(bits, n_q, 3, Tf)
    frames, counts = [Tf - 1, 0, (Tf + 1) // 2], [max(1, n_q - 1), n_q, (n_q + 1) // 2]
    want = pack(torch.from_numpy(clean).cuda(), bits, frames, counts)
    assert np.array_equal(want, restate(clean, frames, counts, bits, want.shape[1]))
    for g in GARBAGE:
        dirty = clean.copy()
        for b in (0, 2):
            dirty[:, b, frames[b]:] = g
            dirty[counts[b]:, b, :] = g
        dirty[:, 1, :] = NAN_BITS             # the neighbour row has no frames: nothing of it may be read into a packet
        got = pack(torch.from_numpy(dirty).cuda(), bits, frames, counts)
        assert np.array_equal(got, want), g
    # inside a row's frames and count the same values are codes, taken modulo 2^bits
    wild = clean.copy()
    wild[0, 0, 0], wild[0, 2, 0] = GARBAGE
    got = pack(torch.from_numpy(wild).cuda(), bits, frames, counts)
    assert np.array_equal(got, restate(wild, frames, counts, bits, got.shape[1]))
    # counts and frames outside their range are clamped on the device: frames to [0, Tf], k to [1, n_q]
    got = pack(torch.from_numpy(clean).cuda(), bits, [Tf + 7, -3, 1 << 30], [n_q + 1, 0, -5])
    assert np.array_equal(got, restate(clean, [Tf, 0, Tf], [n_q, 1, 1], bits, got.shape[1]))


@pytest.mark.parametrize("bits,n_q", [(10, 32), (6, 6), (7, 3)])
def test_a_row_packet_does_not_depend_on_its_batch(bits, n_q):
    codes = seeded(bits, n_q, 3, 130)
    frames, counts = [130, 64, 77], [n_q, 1, (n_q + 1) // 2]
    batch = pack(torch.from_numpy(codes).cuda(), bits, frames, counts)
    for b in range(3):
        alone = pack(torch.from_numpy(np.ascontiguousarray(codes[:, b:b + 1, :frames[b]])).cuda(), bits, None, [counts[b]])
        n = fio.packet_bytes(frames[b], counts[b], bits)
        assert alone[0, :n].tobytes() == batch[b, :n].tobytes() == restate_row(codes, b, frames[b], counts[b], bits)
        assert not alone[0, n:].any() and not batch[b, n:].any()


@pytest.mark.parametrize("bits,n_q,Tf", [(10, 32, 65), (7, 3, 130), (16, 8, 33), (1, 1, 64), (6, 6, 31)])
def test_unpack_of_random_payloads_and_clamped_headers(bits, n_q, Tf):
    rng = np.random.default_rng(bits * 1000 + n_q * 10 + Tf)
    pitch = fio.packet_pitch(Tf, n_q, bits)
    frames, counts = [Tf, 1, (Tf + 1) // 2, Tf], [n_q, n_q, (n_q + 1) // 2, 1]
    rows = np.zeros((4, pitch), np.uint8)
    want = torch.zeros((4, Tf, n_q), dtype=torch.int64)
    for b, (f, k) in enumerate(zip(frames, counts)):
        packet = struct.pack("<IBBBB", f, k, bits, 0, 0) + rng.integers(0, 256, fio.packet_bytes(f, k, bits) - 8, dtype=np.uint8).tobytes()
        rows[b, :len(packet)] = np.frombuffer(packet, np.uint8)
        tok, kk, _ = fio.unpack_packet(packet)                       # the host unpacker
        want[b, :f, :k] = torch.from_numpy(tok)
    assert torch.equal(unpack(rows, Tf, n_q, bits), want)
    # headers whose frames or k exceed the call's are clamped: the payload is then read as Tf frames of n_q stages, inside the row
    if n_q < 255:
        rows2 = rng.integers(0, 256, (2, pitch), dtype=np.uint8)
        rows2[0, :8] = np.frombuffer(struct.pack("<IBBBB", Tf + 5, n_q, bits, 0, 0), np.uint8)
        rows2[1, :8] = np.frombuffer(struct.pack("<IBBBB", 0xFFFFFFFF, n_q + 1, bits, 0, 0), np.uint8)
        want2 = torch.zeros((2, Tf, n_q), dtype=torch.int64)
        for b in range(2):
            n = int.from_bytes(rows2[b, 8:].tobytes(), "little")
            for t in range(Tf):
                for i in range(n_q):
                    want2[b, t, i] = (n >> ((t * n_q + i) * bits)) & ((1 << bits) - 1)
        assert torch.equal(unpack(rows2, Tf, n_q, bits), want2)


# ---- the offline calls (the tiny net: 6 stages of 64 codes, hop 8) ----------------------------------------------------------------------
T_TINY = 400
LENS = [400, 123, 257]
WIDTHS = [2 * BW, 6 * BW, 4 * BW]


@functools.lru_cache(maxsize=None)
def _tiny_wav():
    return audio(3, T_TINY, 4711, "tones").cuda()


def test_packets_of_an_encoding_call_hold_its_codes():
    m = engine_for("tiny", 0)
    plain = m.inference_encoding(_tiny_wav())
    ret = m.inference_encoding(_tiny_wav(), packed=True)
    codes = ret["code_indices"][0]
    assert torch.equal(codes, plain["code_indices"][0]) and "packets" not in plain
    assert ret["packets"].dtype == torch.uint8 and ret["packets"].is_cuda
    assert ret["packets"].shape == (3, fio.packet_pitch(codes.shape[2], 6, 6)) and m.engine.code_bits == 6
    host = m.engine.packets_to_host(ret["packets"])
    for b, p in enumerate(host):
        tok, k, bits = fio.unpack_packet(p)
        assert (k, bits) == (6, 6) and np.array_equal(tok, codes[:, b].cpu().numpy().T)
    # the engine's own round trip, and the bytes back onto the device
    assert torch.equal(m.engine.unpack_codes(ret["packets"], codes.shape[2], 6), codes.permute(1, 2, 0))
    buf, Tf, counts = m.engine.packets_from_host(host)
    assert Tf == codes.shape[2] and counts == [6, 6, 6] and torch.equal(buf, ret["packets"])
    for field, bad in (("mode", host[1][:6] + b"\2" + host[1][7:]), ("bits", host[1][:5] + b"\7" + host[1][6:]),
                       ("k", host[1][:4] + b"\7" + host[1][5:]), ("length", host[1][:-1])):
        with pytest.raises(EngineError, match=f"row 1.*{field}"):
            m.engine.packets_from_host([host[0], bad, host[2]])


def test_lengths_and_a_bit_width_per_row_equal_the_single_row_calls():
    m = engine_for("tiny", 0)
    wav = _tiny_wav()
    ret = m.inference_encoding(wav, bit_width=WIDTHS, speech_lengths=torch.tensor(LENS), packed=True)
    host = m.engine.packets_to_host(ret["packets"])
    for b, (n, bw) in enumerate(zip(LENS, WIDTHS)):
        one = m.inference_encoding(wav[b:b + 1, :n], bit_width=bw, packed=True)
        alone, = m.engine.packets_to_host(one["packets"])
        assert host[b] == alone, b
        frames, k, bits, nbytes = fio.parse_packet_header(host[b])
        assert (frames, k, bits) == (m.engine.frames(n), int(bw // BW), 6) and nbytes == len(host[b])
    # with rvq_beam the packets hold the search's codes
    beam = m.inference_encoding(wav, bit_width=WIDTHS, speech_lengths=torch.tensor(LENS), rvq_beam=2, packed=True)
    for b, p in enumerate(m.engine.packets_to_host(beam["packets"])):
        tok, k, _ = fio.unpack_packet(p)
        assert np.array_equal(tok, beam["code_indices"][0][:k, b, :tok.shape[0]].cpu().numpy().T)


def test_the_counts_of_a_target_snr_go_into_the_headers_on_the_device():
    m = engine_for("tiny", 0, 0.8)
    wav = _tiny_wav()
    ret = m.inference_encoding(wav, target_snr_db=[0.5, 3.0, float("inf")], speech_lengths=torch.tensor(LENS), packed=True)
    counts = ret["n_q_rows"].tolist()
    host = m.engine.packets_to_host(ret["packets"])
    for b, p in enumerate(host):
        tok, k, _ = fio.unpack_packet(p)
        assert k == counts[b] and tok.shape[0] == m.engine.frames(LENS[b])
        assert np.array_equal(tok, ret["code_indices"][0][:k, b, :tok.shape[0]].cpu().numpy().T)
    dec = m.inference_decoding_packed(ret["packets"])
    assert dec["n_q_rows"] == counts and dec["token_lengths"] == [m.engine.frames(n) for n in LENS]
    ref, _ = m.engine.decode_codes(ret["code_indices"][0].permute(1, 2, 0)[:, :, :max(counts)].contiguous(), lengths=dec["token_lengths"],
                                   n_q_rows=counts if len(set(counts)) > 1 else None)
    assert torch.equal(dec["recon_speech"], ref)


def test_decoding_from_packets_equals_decoding_the_codes():
    m = engine_for("tiny", 0)
    wav = _tiny_wav()
    ret = m.inference_encoding(wav, bit_width=WIDTHS, packed=True)
    tokens = ret["code_indices"][0].permute(1, 2, 0).contiguous()
    want = m.inference_decoding(tokens, bit_width=WIDTHS)
    host = m.engine.packets_to_host(ret["packets"])
    for packets in (host, ret["packets"]):
        got = m.inference_decoding_packed(packets)
        assert torch.equal(got["recon_speech"], want["recon_speech"]) and got["n_q_rows"] == [2, 6, 4]
        assert torch.equal(got["code_embeddings"][0][0], want["code_embeddings"][0][0])
    # rows of their own lengths go through token_lengths
    rag = m.inference_encoding(wav, bit_width=WIDTHS, speech_lengths=torch.tensor(LENS), packed=True)
    frames = [m.engine.frames(n) for n in LENS]
    want = m.inference_decoding(rag["code_indices"][0].permute(1, 2, 0).contiguous(), bit_width=WIDTHS, token_lengths=torch.tensor(frames))
    got = m.inference_decoding_packed(m.engine.packets_to_host(rag["packets"]))
    assert got["token_lengths"] == frames and torch.equal(got["recon_speech"], want["recon_speech"])
    # one bit width for all: the plain decode call
    uni = m.inference_encoding(wav, bit_width=3 * BW, packed=True)
    want = m.inference_decoding(uni["code_indices"][0].permute(1, 2, 0).contiguous())
    assert torch.equal(m.inference_decoding_packed(uni["packets"])["recon_speech"], want["recon_speech"])


@pytest.mark.parametrize("name,word", [("ds320seg", "segment_dur"), ("tinybypass", "bypass_quantizer"), ("tinyq0", "q0_ds_ratio")])
def test_packed_is_refused_by_name(name, word):
    m = engine_for(name, 0)
    wav = audio(1, 8000 if name == "ds320seg" else 400, 1, "tones").cuda()
    with pytest.raises(EngineError, match=word):
        m.inference_encoding(wav, packed=True)
    with pytest.raises(EngineError, match=word):
        m.inference_decoding_packed([fio.pack_codes(np.zeros((1, 4), np.int64), 1, m.engine.code_bits)])


def test_speech2token_keeps_its_tuple_and_the_packets_stand_beside_it():
    from funcodec_amd.bin.codec_inference import Speech2Token
    m = engine_for("tiny", 0)
    s2t = Speech2Token.__new__(Speech2Token)
    s2t.model, s2t.device, s2t.dtype, s2t.check_status = m, "cuda", "float32", True
    out = s2t(_tiny_wav(), run_mod="encode", packed=True)
    assert len(out) == 4 and s2t.last_packets is not None
    want = m.inference_encoding(_tiny_wav(), packed=True)["packets"]
    assert torch.equal(s2t.last_packets, want)
    s2t(_tiny_wav(), run_mod="encode")
    assert s2t.last_packets is None
    with pytest.raises(ValueError, match="packed"):
        s2t(_tiny_wav(), run_mod="decode_emb", packed=True)


# ---- sessions (the small causal SoundStream net) ---------------------------------------------------------------------------------------
def _values(packets, b=None):
    """the payload values of a list of pushes' packets of one row, concatenated: [frames, k]"""
    return np.concatenate([fio.unpack_packet(p)[0] for p in packets], 0)


@pytest.mark.parametrize("graph", [False, True])
def test_stream_pushes_pack_to_the_offline_codes_and_decode_back(graph):
    m = engine_for("tinyss", 0)
    hop, B, T = m.engine.hop_length, 2, 8 * 61 + 3
    wav = audio(B, T, 99, "tones").cuda()
    off = m.engine.encode(wav, 6)
    rows = [6, 3]
    off_rows = m.engine.encode(wav, 6, n_q_rows=rows)
    st = m.open_stream(B, n_q=rows, scale=off["scale"], graph=graph)
    dec = m.open_stream(B, n_q=6, scale=off["scale"], graph=graph)          # the decoder's own counts are all 6: the packets carry theirs
    ref = m.open_stream(B, n_q=rows, scale=off["scale"])
    chunks = [hop * 1, hop * 20, hop * 7, hop * 33, 3]
    pos, per_row, wavs, wavs_ref, codes_all = 0, [[] for _ in range(B)], [], [], []
    for j, n in enumerate(chunks):
        final = j == len(chunks) - 1
        codes, quant, packets = st.encode(wav[..., pos:pos + n], final=final, packed=True)
        pos += n
        if codes.shape[-1] == 0:
            assert packets == []
            continue
        assert len(packets) == B
        for b, p in enumerate(packets):
            frames, k, bits, nbytes = fio.parse_packet_header(p)
            assert (frames, k, bits) == (codes.shape[-1], rows[b], 6)
            per_row[b].append(p)
        codes_all.append(codes)
        wavs.append(dec.decode_packed(packets, final=final))
        wavs_ref.append(ref.decode(codes.permute(1, 2, 0).contiguous(), final=final))
    codes_all = torch.cat(codes_all, -1)
    assert torch.equal(codes_all, off_rows["codes"])
    for b in range(B):
        assert np.array_equal(_values(per_row[b]), off_rows["codes"][:rows[b], b].cpu().numpy().T)
        assert np.array_equal(_values(per_row[b])[:, :3], off["codes"][:3, b].cpu().numpy().T)
    assert torch.equal(torch.cat(wavs, -1), torch.cat(wavs_ref, -1))
    assert dec._row_nq is None                    # untouched by the packets' counts
    with pytest.raises(EngineError, match="lock-step"):
        m.open_stream(B, scale=off["scale"]).decode_packed([per_row[0][0], per_row[1][1]])


@pytest.mark.parametrize("graph", [False, True])
def test_slot_pushes_pack_every_slot_by_its_own_frames_and_count(graph):
    m = engine_for("tinyss", 0)
    hop = m.engine.hop_length
    wav = audio(3, hop * 40, 17, "tones").cuda()
    ss = m.open_slots(4, n_q=6, graph=graph)
    dd = m.open_slots(4, n_q=6, graph=graph)
    rr = m.open_slots(4, n_q=6)
    counts = {0: 6, 2: 2, 3: 4}
    for s in (ss, rr):
        for slot, k in counts.items():
            s.set_n_q(slot, k)
    first = ss.min_first_samples
    plan = [{0: first, 2: first + hop * 3, 3: first}, {0: hop * 5, 3: hop * 1}, {2: hop * 2, 0: hop * 1, 3: hop * 9}]
    pos = {0: 0, 2: 0, 3: 0}
    src = {0: 0, 2: 1, 3: 2}
    for step in plan:
        pushes = {slot: wav[src[slot], pos[slot]:pos[slot] + n] for slot, n in step.items()}
        for slot, n in step.items():
            pos[slot] += n
        res, packets = ss.encode(pushes, packed=True)
        assert sorted(packets) == sorted(res) == sorted(step) and 1 not in packets            # the idle slot gives no packet
        for slot, p in packets.items():
            codes = res[slot][0]
            tok, k, bits = fio.unpack_packet(p)
            assert (k, bits) == (counts[slot], 6) and tok.shape[0] == codes.shape[-1] == step[slot] // hop
            assert np.array_equal(tok, codes[:k].cpu().numpy().T) and not codes[k:].any()
        got = dd.decode_packed(packets)
        want = rr.decode({slot: res[slot][0].t().contiguous() for slot in packets})
        assert sorted(got) == sorted(want)
        for slot in got:
            assert torch.equal(got[slot], want[slot]), slot
    assert dd._row_nq == [6, 6, 6, 6]
    assert ss.encode({}, packed=True) == ({}, {})


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _cli(args):
    from funcodec_amd.bin.codec_inference import main
    main(["--ngpu", "1", "--gpuid_list", "0", "--batch_size", "2", "--sampling_rate", "16000"] + args)


def test_cli_packed_indices_decode_to_the_files_of_the_text_form(tmp_path):
    from funcodec_amd.synth import make_checkpoint
    cfg_path, pth_path = make_checkpoint(str(tmp_path / "model"), "tiny", 0, 0.8)
    lens = [400, 123, 257]
    wavs = audio(3, 400, 77, "tones")
    scp = tmp_path / "wav.scp"
    with open(scp, "wt") as f:
        for i, n in enumerate(lens):
            p = str(tmp_path / f"u{i}.wav")
            fio.save_audio(wavs[i:i + 1, :n], p, 16000, rescale=False)
            f.write(f"u{i} {p}\n")
    model = ["--config_file", cfg_path, "--model_file", pth_path, "--bit_width", str(int(4 * BW))]
    enc = model + ["--need_indices", "true", "--run_mod", "encode", "--length_aware", "true", "--data_path_and_name_and_type", f"{scp},speech,sound"]
    _cli(["--output_dir", str(tmp_path / "text.1"), "--indices_save_type", "text"] + enc)
    _cli(["--output_dir", str(tmp_path / "packed.1"), "--indices_save_type", "packed"] + enc)
    fcb = str(tmp_path / "packed.1" / "codecs.fcb")
    assert os.path.exists(fcb + ".scp") and not os.path.exists(str(tmp_path / "packed.1" / "codecs.txt"))
    head, recs = fio.read_fcb(fcb)
    assert head == dict(bits=6, n_q=4, sample_rate=16000, hop=8) and [(k, n) for k, n, _ in recs] == [(f"u{i}", n) for i, n in enumerate(lens)]
    text = dict(fio.read_scp(str(tmp_path / "text.1" / "codecs.txt")))
    for key, _, packet in recs:
        tok, k, _ = fio.unpack_packet(packet)
        assert k == 4 and np.array_equal(tok, fio.load_codec_json(text[key]))
    dec = model + ["--run_mod", "decode"]
    _cli(["--output_dir", str(tmp_path / "dtext.1"), "--data_path_and_name_and_type", f"{tmp_path / 'text.1' / 'codecs.txt'},speech,codec_json"] + dec)
    _cli(["--output_dir", str(tmp_path / "dpacked.1"), "--data_path_and_name_and_type", f"{fcb}.scp,speech,codec_fcb"] + dec)
    for i in range(3):
        with open(tmp_path / "dtext.1" / f"u{i}.wav", "rb") as a, open(tmp_path / "dpacked.1" / f"u{i}.wav", "rb") as b:
            assert a.read() == b.read(), i

    # a target SNR: every packet carries the count codec_n_q.txt names, and decodes with it
    _cli(["--output_dir", str(tmp_path / "rate.1"), "--indices_save_type", "packed", "--target_snr_db", "2.0", "--min_n_q", "1"] + enc)
    fcb = str(tmp_path / "rate.1" / "codecs.fcb")
    table = {k: int(v.split()[0]) for k, v in fio.read_scp(str(tmp_path / "rate.1" / "codec_n_q.txt"))}
    head, recs = fio.read_fcb(fcb)
    assert {k: fio.parse_packet_header(p)[1] for k, _, p in recs} == table and head["n_q"] == 4
    _cli(["--output_dir", str(tmp_path / "drate.1"), "--batch_size", "1", "--data_path_and_name_and_type", f"{fcb}.scp,speech,codec_fcb"] + dec)
    m = engine_for("tiny", 0, 0.8)
    for key, _, packet in recs:
        tok, k, _ = fio.unpack_packet(packet)
        full = np.zeros((tok.shape[0], 4), np.int64)
        full[:, :k] = tok
        ref = m.inference_decoding(torch.from_numpy(full)[None].cuda(), bit_width=[k * BW])["recon_speech"]
        fio.save_audio(ref[0].cpu(), str(tmp_path / "ref.wav"), 16000, rescale=True)
        with open(tmp_path / "ref.wav", "rb") as a, open(tmp_path / "drate.1" / f"{key}.wav", "rb") as b:
            assert a.read() == b.read(), key
