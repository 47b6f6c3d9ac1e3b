"""The bit stream's mode 1, a stage count per frame, on the host (csrc/code_pack_kernels.h states the packet): the numpy packer of
funcodec_amd/io.py round trip over every combination, one packet written out byte by byte, the length formula, every refusal by field,
the library's arithmetic and refusals, the container with both modes, a committed fixture and the C header's wording.  No GPU is needed."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

from funcodec_amd import _lib, io as fio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BITS = (1, 6, 7, 8, 10, 16)
KMAX = (1, 3, 8, 32, 255)
FRAMES = (0, 1, 5, 31, 32, 33, 64, 65)
NEW = ("fc_frame_packet_pitch", "fc_frame_packet_bytes", "fc_frame_pack_workspace_bytes", "fc_codes_pack_frames", "fc_codes_unpack_frames")


def _case(bits, kmax, frames, kind, seed=0):
    rng = np.random.default_rng(100000 * bits + 1000 * kmax + 10 * frames + kind + seed)
    counts = (rng.integers(0, kmax + 1, frames), np.zeros(frames, np.int64), np.full(frames, kmax, np.int64))[kind]
    return rng.integers(0, 1 << bits, (kmax, frames), dtype=np.int64), counts


def _restate_int(codes, counts, bits):
    """the packet in Python integers: header, the counts at cbits bits each padded to a word, the kept codes frame-major"""
    frames = len(counts)
    kmax = max(int(max(counts, default=0)), 1)
    cbits = kmax.bit_length()
    cint = sum(int(k) << (t * cbits) for t, k in enumerate(counts))
    vals = [int(codes[i, t]) & ((1 << bits) - 1) for t in range(frames) for i in range(int(counts[t]))]
    vint = sum(v << (j * bits) for j, v in enumerate(vals))
    return (struct.pack("<IBBBB", frames, kmax, bits, 1, 0) + cint.to_bytes(4 * ((frames * cbits + 31) // 32), "little") +
            vint.to_bytes((len(vals) * bits + 7) // 8, "little"))


@pytest.mark.parametrize("bits", BITS)
def test_numpy_round_trip_over_every_combination(bits):
    for kmax in KMAX:
        for frames in FRAMES:
            for kind in range(3):
                codes, counts = _case(bits, kmax, frames, kind)
                p = fio.pack_frame_codes(codes, counts, bits=bits)
                assert p == _restate_int(codes, counts, bits), (kmax, frames, kind)
                top = max(int(counts.max()) if frames else 0, 1)
                assert len(p) == fio.frame_packet_bytes(frames, top, int(counts.sum()), bits)
                assert fio.packet_mode(p) == 1
                tok, got, b = fio.unpack_frame_packet(p)
                assert b == bits and np.array_equal(got, counts) and tok.shape == (frames, top) and tok.dtype == np.int64
                want = np.where(np.arange(top)[None, :] < counts[:, None], codes.T[:, :top], 0)
                assert np.array_equal(tok, want)
                assert fio.pack_frame_codes(tok, got, bits=b, layout="tq") == p
                f, k, b2, c2, need = fio.parse_frame_packet(p + b"tail", exact=False)
                assert (f, k, b2, need) == (frames, top, bits, len(p)) and np.array_equal(c2, counts)


def test_one_packet_byte_by_byte():
    """frames 3, kmax 2, bits 3, counts [2, 0, 1]; codes[i][t]: frame 0 holds 5, 6, frame 2 holds 3 (what lies behind a count is not packed)"""
    codes = np.array([[5, 1, 3], [6, 2, 4]])
    p = fio.pack_frame_codes(codes, [2, 0, 1], bits=3)
    assert p == bytes([3, 0, 0, 0,      # frames, u32 little-endian
                       2,               # kmax
                       3,               # bits
                       1,               # mode
                       0,
                       # counts, cbits = 2, LSB first: 2 -> bits 0..1 = (0, 1), 0 -> (0, 0), 1 -> bits 4..5 = (1, 0): 0b010010; padded to a word
                       0x12, 0, 0, 0,
                       # codes, 3 bits each: 5 = 0b101 at bits 0..2, 6 = 0b110 at 3..5, 3 = 0b011 at 6..8: byte 0 = 0b11110101, byte 1 = 0
                       0xF5, 0x00])
    assert len(p) == fio.frame_packet_bytes(3, 2, 3, 3) == 8 + 4 + 2
    tok, counts, bits = fio.unpack_frame_packet(p)
    assert tok.tolist() == [[5, 6], [0, 0], [3, 0]] and counts.tolist() == [2, 0, 1] and bits == 3


def test_the_length_formula_and_the_library():
    lib = _lib.load()
    for bits in BITS:
        for kmax in KMAX:
            cbits = kmax.bit_length()
            for T in FRAMES + (300, 7500):
                for n_codes in (0, T, T * kmax):
                    n = 8 + 4 * -(-T * cbits // 32) + -(-n_codes * bits // 8)
                    assert lib.fc_frame_packet_bytes(T, kmax, n_codes, bits) == n == fio.frame_packet_bytes(T, kmax, n_codes, bits)
                pitch = lib.fc_frame_packet_pitch(T, kmax, bits)
                assert pitch == fio.frame_packet_pitch(T, kmax, bits) == -(-lib.fc_frame_packet_bytes(T, kmax, T * kmax, bits) // 16) * 16
                assert pitch >= lib.fc_code_packet_pitch(T, kmax, bits)          # a mixed buffer holds rows of mode 0 too
    for bad in ((-1, 3, 0, 10), (5, 0, 0, 10), (5, 256, 0, 10), (5, 3, 0, 0), (5, 3, 0, 17), (5, 3, 16, 10), (5, 3, -1, 10)):
        assert lib.fc_frame_packet_bytes(*bad) == 0
    for bad in ((-1, 3, 10), (5, 0, 10), (5, 256, 10), (5, 3, 0), (5, 3, 17)):
        assert lib.fc_frame_packet_pitch(*bad) == 0
    assert lib.fc_frame_pack_workspace_bytes(3, 7) == 3 * 8 * 4 and lib.fc_frame_pack_workspace_bytes(0, 7) == 0 == lib.fc_frame_pack_workspace_bytes(3, 0)


def test_every_refusal_names_its_field():
    codes = np.arange(12).reshape(3, 4)
    good = fio.pack_frame_codes(codes, [3, 0, 1, 2], bits=6)

    def refused(field, fn, *a, **kw):
        with pytest.raises(fio.PacketError) as e:
            fn(*a, **kw)
        assert e.value.field == field and str(e.value).startswith(field), str(e.value)

    refused("bits", fio.pack_frame_codes, codes, [1] * 4, bits=0)
    refused("bits", fio.pack_frame_codes, codes, [1] * 4, bits=17)
    refused("frames", fio.pack_frame_codes, codes, [1] * 4, bits=6, frames=5)
    refused("count", fio.pack_frame_codes, codes, [1, 4, 1, 1], bits=6)          # above the stages there are
    refused("count", fio.pack_frame_codes, codes, [1, -1, 1, 1], bits=6)
    refused("count", fio.pack_frame_codes, codes, [1, 1], bits=6)                # fewer counts than frames
    with pytest.raises(fio.PacketError, match=r"^count: frame 1"):
        fio.pack_frame_codes(codes, [1, 4, 1, 1], bits=6)
    refused("length", fio.parse_frame_packet, good[:7])
    refused("length", fio.parse_frame_packet, good[:9])                          # inside the counts section
    refused("length", fio.parse_frame_packet, good[:-1])
    refused("length", fio.parse_frame_packet, good + b"\0")
    refused("length", fio.packet_mode, good[:5])
    refused("mode", fio.parse_frame_packet, good[:6] + b"\0" + good[7:])
    refused("mode", fio.packet_mode, good[:6] + b"\2" + good[7:])
    refused("bits", fio.parse_frame_packet, good[:5] + b"\0" + good[6:])
    refused("bits", fio.parse_frame_packet, good, bits=10)
    refused("k", fio.parse_frame_packet, good[:4] + b"\0" + good[5:])
    refused("k", fio.parse_frame_packet, good, n_q=2)
    two = fio.pack_frame_codes(codes, [2, 0, 1, 2], bits=6)
    refused("k", fio.parse_frame_packet, two[:4] + b"\3" + two[5:])              # a header's kmax that is not the largest count
    over = bytearray(fio.pack_frame_codes(codes[:2], [2, 0, 1, 2], bits=6))      # kmax 2, cbits 2: frame 1's count made 3
    over[8] |= 0x0C
    with pytest.raises(fio.PacketError, match=r"^count: frame 1"):
        fio.parse_frame_packet(bytes(over))
    # the mode-0 functions stay mode-0 functions
    refused("mode", fio.parse_packet_header, good)
    refused("mode", fio.unpack_packet, good)
    # the header alone
    assert fio.parse_frame_packet(good[:8], exact=None) == (4, 3, 6, None, None)
    mode, f, k, b, counts, need = fio.parse_any_packet(good)
    assert (mode, f, k, b, need) == (1, 4, 3, 6, len(good)) and counts.tolist() == [3, 0, 1, 2]
    mode, f, k, b, counts, need = fio.parse_any_packet(fio.pack_codes(codes, 2, 6))
    assert (mode, f, k, b) == (0, 4, 2, 6) and counts.tolist() == [2] * 4


def test_refusals_of_the_library_calls_need_no_gpu():
    """refused before any launch, the argument named: the pointers here are host memory that no kernel ever sees"""
    lib = _lib.load()
    B, Tf, n_q, bits = 2, 5, 3, 10
    pitch = lib.fc_frame_packet_pitch(Tf, n_q, bits)
    nws = lib.fc_frame_pack_workspace_bytes(B, Tf)
    codes = torch.zeros((n_q, B, Tf), dtype=torch.int64)
    out = torch.zeros((B, pitch), dtype=torch.uint8)
    tok = torch.zeros((B, Tf, n_q), dtype=torch.int64)
    kf = torch.zeros((B, Tf), dtype=torch.int32)
    ws = torch.zeros((nws,), dtype=torch.uint8)
    cp, op, tp, kp, wp = (C.c_void_p(t.data_ptr()) for t in (codes, out, tok, kf, ws))

    def pack(codes=cp, B=B, Tf=Tf, n_q=n_q, bits=bits, kf=kp, out=op, pitch=pitch, ws=wp, nws=nws):
        return lib.fc_codes_pack_frames(codes, B, Tf, n_q, bits, None, kf, out, pitch, ws, nws, None)

    def unpack(inp=op, pitch=pitch, B=B, Tf=Tf, n_q=n_q, bits=bits, tok=tp, kf=kp, ws=wp, nws=nws):
        return lib.fc_codes_unpack_frames(inp, pitch, B, Tf, n_q, bits, tok, kf, ws, nws, None)

    def refused(rc, word):
        assert rc != 0
        assert word in _lib.last_error(), _lib.last_error()

    for fn in (pack, unpack):
        for b in (0, 17):
            refused(fn(bits=b), "bits")
        for q in (0, 256):
            refused(fn(n_q=q), "n_q")
        refused(fn(B=0), "B")
        refused(fn(Tf=0), "Tf")
        refused(fn(pitch=4), "pitch")
        refused(fn(pitch=pitch + 2), "pitch")
        refused(fn(kf=None), "n_q_frames")
        refused(fn(ws=None), "workspace")
        refused(fn(nws=nws - 4), "workspace")
        refused(fn(Tf=2 ** 31 // 3 + 1, pitch=2 ** 40), "int32 scan")     # Tf * n_q does not fit an i32
    refused(pack(pitch=pitch - 16), "fc_frame_packet_pitch")
    refused(pack(codes=None), "codes")
    refused(pack(out=None), "packets")
    refused(unpack(inp=None), "packets")
    refused(unpack(tok=None), "tokens")
    assert not out.any() and not tok.any() and not ws.any()


# ---- the container ---------------------------------------------------------------------------------------------------------------------
KEYS = ("utt_b", "utt_a", "früh_語_0", "utt_c")


def write_frames_fcb(path):
    """four seeded utterances of the tiny recipe's format (6 bits, 6 stages, 16 kHz, hop 8): three packets of mode 1 (random counts, all
    0, all 6) and one of mode 0 in one file"""
    records = []
    with fio.FcbWriter(path, 6, 6, 16000, 8) as w:
        for j, (key, T) in enumerate(zip(KEYS, (5, 1, 33, 12))):
            codes, counts = _case(6, 6, T, j % 3, seed=7)
            if j == 3:
                counts = np.full(T, 4)
                packet = fio.pack_codes(codes, 4, 6)
            else:
                packet = fio.pack_frame_codes(codes, counts, bits=6)
            w(key, packet, T * 8 - j)
            records.append((key, T * 8 - j, packet, codes, counts))
    return records


def test_fcb_holds_both_modes(tmp_path):
    path = str(tmp_path / "codecs.fcb")
    records = write_frames_fcb(path)
    head, got = fio.read_fcb(path)
    assert head == dict(bits=6, n_q=6, sample_rate=16000, hop=8) and [(k, n, p) for k, n, p, _, _ in records] == got
    assert [fio.packet_mode(p) for _, _, p in got] == [1, 1, 1, 0]
    for (key, spec), (_, samples, packet, codes, counts) in zip(fio.read_scp(path + ".scp"), records):
        assert fio.load_fcb_record(spec) == (head, samples, packet)
        tok, top, c, mode = fio.load_fcb_frames(spec)
        assert tok.shape == (codes.shape[1], 6) and np.array_equal(c, counts) and mode == fio.packet_mode(packet)
        assert np.array_equal(tok, np.where(np.arange(6)[None, :] < counts[:, None], codes.T, 0))
        assert np.array_equal(fio._load_item(spec, "codec_fcb"), tok) and fio.load_fcb_item(spec)[1] == top
    with pytest.raises(fio.PacketError, match="^k"):                     # a count above the file's n_q
        with fio.FcbWriter(str(tmp_path / "bad.fcb"), 6, 2, 16000, 8) as w:
            w("x", records[2][2], 1)
    # a batch that holds a mode-1 packet carries a count per frame, zeros behind a row's frames; a mode-0 row counts its k
    batches = list(fio.iter_batches([(path + ".scp", "speech", "codec_fcb")], 2))
    for (keys, batch), recs in zip(batches, (records[:2], records[2:])):
        assert sorted(batch) == ["speech", "speech_lengths", "speech_n_q", "speech_n_q_frames"]
        assert batch["speech_n_q_frames"].dtype == torch.int32 and batch["speech_n_q_frames"].shape == batch["speech"].shape[:2]
        for i, (_, _, _, codes, counts) in enumerate(recs):
            T = codes.shape[1]
            assert batch["speech_n_q_frames"][i, :T].tolist() == counts.tolist() and not batch["speech_n_q_frames"][i, T:].any()


def test_the_committed_fixture_is_what_the_packer_writes_today(tmp_path):
    """the format cannot drift silently: tests/golden/fcb_frames.fcb was made by write_frames_fcb and committed"""
    path = str(tmp_path / "codecs.fcb")
    write_frames_fcb(path)
    with open(path, "rb") as f, open(os.path.join(GOLD, "fcb_frames.fcb"), "rb") as g:
        made, kept = f.read(), g.read()
    assert len(kept) < 1024 and made == kept
    head, recs = fio.read_fcb(os.path.join(GOLD, "fcb_frames.fcb"))
    assert [k for k, _, _ in recs] == list(KEYS) and head["bits"] == 6
    for key, _, packet in recs[:3]:
        tok, counts, bits = fio.unpack_frame_packet(packet)
        assert fio.pack_frame_codes(tok, counts, bits=bits, layout="tq") == packet


def test_the_header_documents_the_entry_points_and_the_abi_stays():
    with open(os.path.join(ROOT, "include", "funcodec_amd.h")) as f:
        text = f.read()
    assert re.search(r"#define FC_ABI_VERSION 7\b", text) and _lib.FC_ABI_VERSION == 7 and _lib.load().fc_abi_version() == 7
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:size_t|int) " + name + r"\(", text, re.S)
        assert m and "csrc/code_pack_kernels.h" in m.group(1), name          # each entry states the rule by reference to the kernel header
    with open(os.path.join(ROOT, "funcodec_amd", "csrc", "code_pack_kernels.h")) as f:
        rule = f.read()
    for word in ("mode = 1", "kmax", "cbits", "frame-major", "LSB first", "rounded up to 16", "exactly one writer"):
        assert word in rule, word
    from funcodec_amd import build
    assert "code_pack_frames_kernels.hip" in build.sources()
