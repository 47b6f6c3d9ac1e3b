"""The bit stream's mode 1, a stage count per frame, on the MI355X (csrc/code_pack_kernels.h states the packet): fc_codes_pack_frames /
fc_codes_unpack_frames against the numpy restatement of funcodec_amd/io.py over every word edge, garbage and hostile packets, mixed
buffers, then the packets of the offline calls and the CLI.  Every comparison is exact."""
import ctypes as C
import os
import struct

import numpy as np
import pytest
import torch

from funcodec_amd import _lib, io as fio
from funcodec_amd.engine import EngineError
from helpers import audio, engine_for

pytestmark = pytest.mark.gpu
BITS = (1, 6, 10, 16)
KMAX = (1, 3, 32)
FRAMES = (1, 31, 32, 33, 63, 64, 65, 300)
GARBAGE = (-1, (1 << 40) + 5)
FILL, GUARD = 0xA5, 4096
BW = 12000.0          # one stage of the tiny quantisers


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _i32(a):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.int32).cuda()


def pack(codes, counts, bits, frames_rows=None):
    """fc_codes_pack_frames of codes [n_q, B, Tf] and counts [B, Tf] into a buffer pre-filled with 0xA5 with a guard behind it, which
    must stay 0xA5 -> uint8 [B, pitch] on the host"""
    lib = _lib.load()
    codes = torch.as_tensor(codes).cuda()
    n_q, B, Tf = codes.shape
    pitch = lib.fc_frame_packet_pitch(Tf, n_q, bits)
    assert pitch == fio.frame_packet_pitch(Tf, n_q, bits)
    out = torch.full((B * pitch + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    nws = lib.fc_frame_pack_workspace_bytes(B, Tf)
    assert nws == 4 * B * (Tf + 1)
    ws = torch.full((nws + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    kf, fr = _i32(counts), _i32(frames_rows)
    rc = lib.fc_codes_pack_frames(_p(codes), B, Tf, n_q, bits, _p(fr), _p(kf), _p(out), pitch, _p(ws), nws, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    out, ws = out.cpu().numpy(), ws.cpu().numpy()
    assert (out[B * pitch:] == FILL).all() and (ws[nws:] == FILL).all(), "a guard region was written"
    return out[:B * pitch].reshape(B, pitch)


def unpack(packets, Tf, n_q, bits):
    """fc_codes_unpack_frames of uint8 [B, pitch] (numpy) into buffers pre-filled with -1 with guards behind them -> (tokens, counts)"""
    lib = _lib.load()
    dev = torch.from_numpy(np.ascontiguousarray(packets)).cuda()
    B, pitch = dev.shape
    n = B * Tf * n_q
    tok = torch.full((n + GUARD,), -1, dtype=torch.int64, device="cuda")
    kf = torch.full((B * Tf + GUARD,), -1, dtype=torch.int32, device="cuda")
    nws = lib.fc_frame_pack_workspace_bytes(B, Tf)
    ws = torch.full((nws + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    rc = lib.fc_codes_unpack_frames(_p(dev), pitch, B, Tf, n_q, bits, _p(tok), _p(kf), _p(ws), nws, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    tok, kf, ws = tok.cpu(), kf.cpu(), ws.cpu().numpy()
    assert bool((tok[n:] == -1).all()) and bool((kf[B * Tf:] == -1).all()) and (ws[nws:] == FILL).all(), "a guard region was written"
    return tok[:n].view(B, Tf, n_q).numpy(), kf[:B * Tf].view(B, Tf).numpy()


def restate(codes, counts, bits, frames_rows, pitch):
    """the whole pitched buffer by the numpy packer: counts clamped to [0, n_q], frames to [0, Tf], zeros up to the pitch"""
    n_q, B, Tf = codes.shape
    rows = []
    for b in range(B):
        f = Tf if frames_rows is None else min(max(int(frames_rows[b]), 0), Tf)
        p = fio.pack_frame_codes(codes[:, b], np.clip(counts[b], 0, n_q), bits=bits, frames=f)
        rows.append(p + bytes(pitch - len(p)))
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(B, pitch)


def tokens_of(codes, counts, frames_rows=None):
    n_q, B, Tf = codes.shape
    tok = np.transpose(codes, (1, 2, 0)).copy()
    k = np.clip(counts, 0, n_q).copy()
    if frames_rows is not None:
        for b, f in enumerate(frames_rows):
            k[b, max(min(int(f), Tf), 0):] = 0
    tok[np.arange(n_q)[None, None, :] >= k[:, :, None]] = 0
    return tok, k


def case(bits, n_q, Tf, seed=0):
    """three rows: random counts (and its own frames), all 0, all n_q"""
    rng = np.random.default_rng(100000 * bits + 1000 * n_q + 10 * Tf + seed)
    codes = rng.integers(0, 1 << bits, (n_q, 3, Tf), dtype=np.int64)
    counts = np.stack([rng.integers(0, n_q + 1, Tf), np.zeros(Tf, np.int64), np.full(Tf, n_q)]).astype(np.int32)
    frames = [int(rng.integers(0, Tf + 1)), Tf, Tf]
    return codes, counts, frames


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_pack_and_unpack_against_the_numpy_restatement_over_every_word_edge(bits):
    for n_q in KMAX:
        for Tf in FRAMES:
            codes, counts, frames = case(bits, n_q, Tf)
            for fr in (None, frames):
                got = pack(codes, counts, bits, fr)
                want = restate(codes, counts, bits, fr, got.shape[1])
                assert np.array_equal(got, want), (n_q, Tf, fr, np.argwhere(got != want)[:4].tolist())
                tok, kf = unpack(got, Tf, n_q, bits)
                wtok, wk = tokens_of(codes, counts, fr)
                assert np.array_equal(kf, wk) and np.array_equal(tok, wtok), (n_q, Tf, fr)


@pytest.mark.parametrize("bits,n_q,Tf", [(6, 3, 33), (10, 32, 65), (16, 32, 300)])
def test_garbage_behind_counts_and_frames_does_not_reach_a_byte(bits, n_q, Tf):
    codes, counts, frames = case(bits, n_q, Tf, 1)
    frames[2] = Tf - 1
    clean = pack(codes, counts, bits, frames)
    _, k = tokens_of(codes, counts, frames)
    behind = np.arange(n_q)[:, None, None] >= k[None]
    for g in GARBAGE:
        dirty = np.where(behind, g, codes)
        dc = counts.copy()
        for b, f in enumerate(frames):
            dc[b, f:] = 200 + b                                        # counts behind a row's frames are not looked at
        assert np.array_equal(pack(dirty, dc, bits, frames), clean)
    # counts outside [0, n_q] are clamped
    wild = counts.copy()
    wild[0, ::2] = -3
    wild[2, ::3] = n_q + 9
    assert np.array_equal(pack(codes, wild, bits, frames), restate(codes, wild, bits, frames, clean.shape[1]))


@pytest.mark.parametrize("bits,n_q,Tf", [(6, 3, 31), (10, 32, 64)])
def test_unpack_of_buffers_that_mix_both_modes(bits, n_q, Tf):
    codes, counts, frames = case(bits, n_q, Tf, 2)
    pitch = fio.frame_packet_pitch(Tf, n_q, bits)
    k0 = max(n_q - 1, 1)
    rows = [fio.pack_frame_codes(codes[:, 0], counts[0], bits=bits, frames=frames[0]), fio.pack_codes(codes[:, 1], k0, bits, Tf - 1),
            fio.pack_frame_codes(codes[:, 2], counts[2], bits=bits)]
    buf = np.frombuffer(b"".join(r + bytes(pitch - len(r)) for r in rows), dtype=np.uint8).reshape(3, pitch)
    tok, kf = unpack(buf, Tf, n_q, bits)
    c = counts.copy()
    c[1] = k0
    wtok, wk = tokens_of(codes, c, [frames[0], Tf - 1, Tf])
    assert np.array_equal(kf, wk) and np.array_equal(tok, wtok)


def restate_unpack(row, Tf, n_q, bits):
    """one row of fc_codes_unpack_frames in Python integers, with the clamps of csrc/code_pack_kernels.h: frames to [0, Tf], kmax to
    [1, n_q], a count to [0, kmax]; the codes section where the header's own frames put it; bits behind the pitch are 0"""
    big = int.from_bytes(bytes(row), "little")                        # (bits behind the pitch read as 0)
    f, kb, _, mode, _ = struct.unpack_from("<IBBBB", bytes(row), 0)
    frames, kb = min(f, Tf), min(max(kb, 1), n_q)
    cbits = kb.bit_length()
    tok, k = np.zeros((Tf, n_q), np.int64), np.zeros(Tf, np.int32)
    base, s = 64, 0
    if mode == 1:
        base += 32 * ((f * cbits + 31) // 32)
    nbits = 8 * len(row)
    for t in range(frames):
        k[t] = min((big >> (64 + t * cbits)) & ((1 << cbits) - 1), kb) if mode == 1 else kb
        for i in range(k[t]):
            P = base + (s + i) * bits
            w = P // 32
            inside = w * 32 + 32 <= nbits and ((P % 32) + bits <= 32 or w * 32 + 64 <= nbits)
            tok[t, i] = (big >> P) & ((1 << bits) - 1) if inside else 0
        s += int(k[t])
    return tok, k


@pytest.mark.parametrize("bits,n_q,Tf", [(6, 3, 33), (10, 5, 64), (16, 32, 31)])
def test_unpack_of_hostile_packets_stays_inside_its_row(bits, n_q, Tf):
    rng = np.random.default_rng(5 + bits + n_q + Tf)
    pitch = fio.frame_packet_pitch(Tf, n_q, bits)
    buf = rng.integers(0, 256, (4, pitch), dtype=np.uint8)            # random payloads: counts above kmax, codes anywhere
    heads = [(Tf, n_q, 1), (Tf + 1000, 255, 1), (0xFFFFFFFF, 0, 1), (Tf - 1, 200, 0)]      # frames above Tf, kmax outside 1..n_q
    for b, (f, kb, mode) in enumerate(heads):
        buf[b, :8] = np.frombuffer(struct.pack("<IBBBB", f, kb, bits, mode, 0), dtype=np.uint8)
    tok, kf = unpack(buf, Tf, n_q, bits)
    for b in range(4):
        wtok, wk = restate_unpack(buf[b], Tf, n_q, bits)
        assert np.array_equal(kf[b], wk) and np.array_equal(tok[b], wtok), b
    assert kf.max() <= n_q and tok.max() < (1 << bits) and tok.min() >= 0


# ---- the offline calls -----------------------------------------------------------------------------------------------------------------
def _round_trip(m, wav, targets, lens=None, **kw):
    """inference(per_frame, packed) -> packets_to_host -> inference_decoding_packed, held to what the mode-0 round trip is held to: the
    packets hold the call's codes and counts, and decoding them equals decoding the codes"""
    sl = {} if lens is None else dict(speech_lengths=torch.tensor(lens))
    ret = m.inference_encoding(wav, target_snr_db=targets, per_frame=True, packed=True, **sl, **dict(dict(min_n_q=0), **kw))
    codes, kf = ret["code_indices"][0], ret["n_q_frames"]
    n_q, Bn, Tf = codes.shape
    assert ret["packets"].dtype == torch.uint8 and ret["packets"].is_cuda and ret["packets"].shape == (Bn, fio.frame_packet_pitch(Tf, n_q, m.engine.code_bits))
    host = m.engine.packets_to_host(ret["packets"])
    frames = [Tf] * Bn if lens is None else [m.engine.frames(n) for n in lens]
    for b, p in enumerate(host):
        assert fio.packet_mode(p) == 1 and len(p) == fio.frame_packet_bytes(frames[b], max(int(ret["n_q_rows"][b]), 1), int(ret["n_codes_rows"][b]), m.engine.code_bits)
        tok, counts, bits = fio.unpack_frame_packet(p)
        assert bits == m.engine.code_bits and np.array_equal(counts, kf[b, :frames[b]].cpu().numpy())
        assert np.array_equal(tok, codes[:tok.shape[1], b, :frames[b]].cpu().numpy().T)
    tokens = codes.permute(1, 2, 0).contiguous()
    want = m.inference_decoding(tokens, n_q_frames=kf, token_lengths=None if lens is None or len(set(frames)) == 1 else torch.tensor(frames))
    for packets in (host, ret["packets"]):
        got = m.inference_decoding_packed(packets)
        assert got["token_lengths"] == frames and got["n_q_rows"] == [max(k, 1) for k in ret["n_q_rows"].tolist()]
        top = got["n_q_frames"].shape[1]
        assert torch.equal(got["n_q_frames"], kf[:, :top])
        assert torch.equal(got["recon_speech"], want["recon_speech"][..., :got["recon_speech"].shape[-1]])
        assert torch.equal(got["code_embeddings"][0][0], ret["code_embeddings"][0][0][:, :top])
    return ret, host


def test_tiny_round_trip_with_lengths_caps_and_the_search():
    m = engine_for("tiny", 0, 0.8)
    T = 3003
    wav = audio(3, T, 4711, "tones").cuda()
    ret, host = _round_trip(m, wav, [2.0, 6.0, 4.0])
    assert len(set(ret["n_q_frames"].reshape(-1).tolist())) > 1
    lens = [T, T - 59, 1201]
    _round_trip(m, wav, [2.0, 6.0, 4.0], lens)
    _round_trip(m, wav, [2.0, 6.0, float("inf")], lens, bit_width=[2 * BW, 6 * BW, 4 * BW], rvq_beam=2, min_n_q=1)
    # a bad packet names the row and the field
    bad_count = bytearray(fio.pack_frame_codes(np.array([[5, 1, 3], [6, 2, 4]]), [2, 0, 1], bits=6))
    bad_count[8] |= 0x0C                                               # frame 1: a count of 3 under kmax = 2
    for field, bad in (("mode", host[1][:6] + b"\2" + host[1][7:]), ("bits", host[1][:5] + b"\7" + host[1][6:]),
                       ("k", host[1][:4] + b"\7" + host[1][5:]), ("length", host[1][:-1]), ("count", bytes(bad_count))):
        with pytest.raises(EngineError, match=f"row 1.*{field}"):
            m.engine.packets_from_host([host[0], bad, host[2]])
    m.engine.check_status()


def test_freq_codec_round_trip():
    from helpers import freq_engine_for
    m = freq_engine_for("tinyfreq", 3)
    wav = audio(3, 1777, 762, "tones").cuda()
    _round_trip(m, wav, [1.0, float("inf"), 3.0])
    m.engine.check_status()


def test_speech2token_keeps_the_counts():
    from funcodec_amd.bin.codec_inference import Speech2Token
    from funcodec_amd.synth import make_checkpoint
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        cfg_path, pth_path = make_checkpoint(os.path.join(d, "model"), "tiny", 0, 0.8)
        s2t = Speech2Token(cfg_path, pth_path, device="cuda")
        wav = audio(2, 1603, 5, "tones")
        out = s2t(wav, run_mod="encode", target_snr_db=3.0, per_frame=True, packed=True)
        assert len(out) == 4 and s2t.last_n_q_frames.shape == (2, out[0][0].shape[-1]) and s2t.last_n_q_frames.dtype == torch.int32
        assert [fio.packet_mode(p) for p in s2t.model.engine.packets_to_host(s2t.last_packets)] == [1, 1]
        s2t(wav, run_mod="encode")
        assert s2t.last_n_q_frames is None and s2t.last_packets is None
        with pytest.raises(Exception, match="target"):
            s2t(wav, run_mod="encode", per_frame=True)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _cli(args):
    from funcodec_amd.bin.codec_inference import main
    main(["--ngpu", "1", "--gpuid_list", "0", "--batch_size", "2", "--sampling_rate", "16000"] + args)


def test_cli_per_frame_writes_mode_1_packets_and_decodes_them(tmp_path):
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
    enc = model + ["--need_indices", "true", "--run_mod", "encode", "--length_aware", "true", "--data_path_and_name_and_type", f"{scp},speech,sound",
                   "--target_snr_db", "2.0", "--per_frame", "true", "--min_n_q", "0"]
    with pytest.raises(Exception, match="indices_save_type"):          # the text form has no place for the counts
        _cli(["--output_dir", str(tmp_path / "text.1"), "--indices_save_type", "text"] + enc)
    _cli(["--output_dir", str(tmp_path / "frames.1"), "--indices_save_type", "packed"] + enc)
    fcb = str(tmp_path / "frames.1" / "codecs.fcb")
    head, recs = fio.read_fcb(fcb)
    assert head["n_q"] == 4 and [(k, n) for k, n, _ in recs] == [(f"u{i}", n) for i, n in enumerate(lens)]
    table = {k: v.split() for k, v in fio.read_scp(str(tmp_path / "frames.1" / "codec_n_q.txt"))}
    m = engine_for("tiny", 0, 0.8)
    _cli(["--output_dir", str(tmp_path / "dframes.1"), "--data_path_and_name_and_type", f"{fcb}.scp,speech,codec_fcb", "--batch_size", "1"] + model + ["--run_mod", "decode"])
    for key, _, packet in recs:
        assert fio.packet_mode(packet) == 1
        tok, counts, _ = fio.unpack_frame_packet(packet)
        assert len(table[key]) == 3 and int(table[key][0]) == max(int(counts.max()), 1) and abs(float(table[key][2]) - counts.mean()) < 1e-3
        full = np.zeros((tok.shape[0], 4), np.int64)
        full[:, :tok.shape[1]] = tok
        ref = m.inference_decoding(torch.from_numpy(full)[None].cuda(), n_q_frames=torch.from_numpy(counts.astype(np.int32))[None])["recon_speech"]
        fio.save_audio(ref[0].cpu(), str(tmp_path / "ref.wav"), 16000, rescale=True)
        with open(tmp_path / "ref.wav", "rb") as a, open(tmp_path / "dframes.1" / f"{key}.wav", "rb") as b:
            assert a.read() == b.read(), key
