"""The codec's bit stream on the host (csrc/code_pack_kernels.h states the packet): the numpy packer of funcodec_amd/io.py against a
restatement in Python integers, every header field and refusal, the pitch / length arithmetic of the library, the ``codecs.fcb``
container with its index, the ``codec_fcb`` input type, a committed fixture, and the C header's wording.  No GPU is needed."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

from funcodec_amd import _lib, io as fio
from funcodec_amd.config import arch_from_config, recipe_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BITS = (1, 6, 7, 8, 10, 16)
COUNTS = (1, 3, 8, 32)
FRAMES = (1, 2, 31, 33, 64, 65)


def restate(codes, k, bits, frames=None):
    """the packet of codes [n_q, T] in Python integers: value j = t k + i at stream bits [j bits, (j + 1) bits), LSB first"""
    frames = codes.shape[1] if frames is None else frames
    n = sum((int(codes[i, t]) % (1 << bits)) << ((t * k + i) * bits) for t in range(frames) for i in range(k))
    return struct.pack("<IBBBB", frames, k, bits, 0, 0) + n.to_bytes((frames * k * bits + 7) // 8, "little")


def seeded_codes(bits, T, seed=0, n_q=32):
    return np.random.default_rng(1000 * bits + 7 * T + seed).integers(0, 1 << bits, (n_q, T), dtype=np.int64)


@pytest.mark.parametrize("bits", BITS)
def test_pack_and_unpack_against_python_integers(bits):
    for k in COUNTS:
        for T in FRAMES:
            codes = seeded_codes(bits, T)
            want = restate(codes, k, bits)
            got = fio.pack_codes(codes, k, bits)
            assert got == want, (bits, k, T)
            assert got == fio.pack_codes(codes.T, k, bits, layout="tq")
            assert len(got) == fio.packet_bytes(T, k, bits) == 8 + -(-T * k * bits // 8)
            tok, kk, bb = fio.unpack_packet(got)
            assert (kk, bb) == (k, bits) and tok.dtype == np.int64 and np.array_equal(tok, codes[:k].T)
            pad = 8 * (len(got) - 8) - T * k * bits                         # pad bits are zero
            assert 0 <= pad < 8 and (pad == 0 or got[-1] >> (8 - pad) == 0)
            # a frame count below the array's: nothing behind it reaches the packet
            if T > 1:
                assert fio.pack_codes(codes, k, bits, frames=T - 1) == restate(codes, k, bits, T - 1)


def test_a_code_is_taken_modulo_two_to_the_bits():
    codes = np.array([[-1, (1 << 40) + 5, 64, 63]], dtype=np.int64)
    assert fio.pack_codes(codes, 1, 6) == restate(np.array([[63, 5, 0, 63]]), 1, 6)


def test_every_header_field_and_refusal_names_its_field():
    codes = seeded_codes(10, 5)
    p = fio.pack_codes(codes, 3, 10)
    assert struct.unpack("<IBBBB", p[:8]) == (5, 3, 10, 0, 0)
    assert fio.parse_packet_header(p) == (5, 3, 10, len(p))
    assert fio.parse_packet_header(p, n_q=3, bits=10) == (5, 3, 10, len(p))
    assert fio.parse_packet_header(p + b"\0\0", exact=False)[3] == len(p)
    bad = {"mode": p[:6] + b"\1" + p[7:], "bits": p[:5] + b"\x11" + p[6:], "k": p[:4] + b"\0" + p[5:], "length": p + b"\0"}
    for field, q in bad.items():
        with pytest.raises(fio.PacketError, match="^" + field) as err:
            fio.parse_packet_header(q)
        assert err.value.field == field
        with pytest.raises(fio.PacketError):
            fio.unpack_packet(q)
    for kw, field in ((dict(n_q=2), "k"), (dict(bits=8), "bits")):
        with pytest.raises(fio.PacketError, match="^" + field):
            fio.parse_packet_header(p, **kw)
    with pytest.raises(fio.PacketError, match="^length"):
        fio.parse_packet_header(p[:-1])
    with pytest.raises(fio.PacketError, match="^length"):
        fio.parse_packet_header(p[:5])
    with pytest.raises(fio.PacketError, match="^k"):
        fio.pack_codes(codes, 33, 10)
    with pytest.raises(fio.PacketError, match="^bits"):
        fio.pack_codes(codes, 3, 17)
    with pytest.raises(fio.PacketError, match="^frames"):
        fio.pack_codes(codes, 3, 10, frames=6)
    assert [fio.code_bits(n) for n in (2, 64, 65, 128, 256, 1024, 1025)] == [1, 6, 7, 7, 8, 10, 11]


def test_pitch_and_bytes_of_the_library_follow_the_formula():
    lib = _lib.load()
    for bits in BITS:
        for n_q in COUNTS + (255,):
            for T in (0,) + FRAMES + (130, 7500):
                nbytes = 8 + -(-T * n_q * bits // 8)
                assert lib.fc_code_packet_bytes(T, n_q, bits) == nbytes == fio.packet_bytes(T, n_q, bits)
                pitch = lib.fc_code_packet_pitch(T, n_q, bits)
                assert pitch == fio.packet_pitch(T, n_q, bits) == -(-nbytes // 16) * 16
                assert pitch % 16 == 0 and pitch >= nbytes >= max(lib.fc_code_packet_bytes(T, k, bits) for k in range(1, n_q + 1))
    for bad in ((-1, 3, 10), (5, 0, 10), (5, 256, 10), (5, 3, 0), (5, 3, 17)):
        assert lib.fc_code_packet_bytes(*bad) == 0 and lib.fc_code_packet_pitch(*bad) == 0


def test_refusals_of_the_pack_and_unpack_calls_need_no_gpu():
    """refused before any launch, the argument named: the pointers here are host memory that no kernel ever sees"""
    lib = _lib.load()
    B, Tf, n_q, bits = 2, 5, 3, 10
    pitch = lib.fc_code_packet_pitch(Tf, n_q, bits)
    codes = torch.zeros((n_q, B, Tf), dtype=torch.int64)
    out = torch.zeros((B, pitch), dtype=torch.uint8)
    tok = torch.zeros((B, Tf, n_q), dtype=torch.int64)
    cp, op, tp = (C.c_void_p(t.data_ptr()) for t in (codes, out, tok))

    def refused(rc, word):
        assert rc != 0
        assert word in _lib.last_error(), _lib.last_error()

    for b in (0, 17):
        refused(lib.fc_codes_pack(cp, B, Tf, n_q, b, None, None, op, pitch, None), "bits")
        refused(lib.fc_codes_unpack(op, pitch, B, Tf, n_q, b, tp, None), "bits")
    for q in (0, 256):
        refused(lib.fc_codes_pack(cp, B, Tf, q, bits, None, None, op, pitch, None), "n_q")
        refused(lib.fc_codes_unpack(op, pitch, B, Tf, q, bits, tp, None), "n_q")
    refused(lib.fc_codes_pack(cp, B, Tf, n_q, bits, None, None, op, pitch - 16, None), "pitch")
    refused(lib.fc_codes_unpack(op, pitch - 16, B, Tf, n_q, bits, tp, None), "pitch")
    refused(lib.fc_codes_pack(None, B, Tf, n_q, bits, None, None, op, pitch, None), "codes")
    refused(lib.fc_codes_pack(cp, B, Tf, n_q, bits, None, None, None, pitch, None), "packets")
    refused(lib.fc_codes_unpack(None, pitch, B, Tf, n_q, bits, tp, None), "packets")
    refused(lib.fc_codes_unpack(op, pitch, B, Tf, n_q, bits, None, None), "tokens")
    assert not out.any()


# ---- the container ---------------------------------------------------------------------------------------------------------------------
KEYS = ("utt_b", "utt_a", "früh_語_0", "utt_c")          # deliberately not sorted: the file keeps the order of writing


def write_tiny_fcb(path):
    """four seeded utterances of the tiny recipe's format (6 bits, 6 stages, 16 kHz, hop 8): different frames and stage counts"""
    records = []
    with fio.FcbWriter(path, 6, 6, 16000, 8) as w:
        for j, (key, T, k) in enumerate(zip(KEYS, (5, 1, 33, 12), (6, 1, 3, 4))):
            codes = seeded_codes(6, T, seed=j, n_q=6)
            packet = fio.pack_codes(codes, k, 6)
            w(key, packet, T * 8 - j)
            records.append((key, T * 8 - j, packet, codes, k))
    return records


def test_fcb_write_read_and_index_round_trip(tmp_path):
    path = str(tmp_path / "codecs.fcb")
    records = write_tiny_fcb(path)
    head, got = fio.read_fcb(path)
    assert head == dict(bits=6, n_q=6, sample_rate=16000, hop=8)
    assert [(k, n, p) for k, n, p, _, _ in records] == got             # file order = writing order, whatever the keys sort to
    index = fio.read_scp(path + ".scp")
    assert [k for k, _ in index] == list(KEYS)
    offsets = [int(v.rpartition(":")[2]) for _, v in index]
    assert offsets == sorted(offsets) and all(v.rpartition(":")[0] == path for _, v in index)
    for (key, spec), (_, samples, packet, codes, k) in zip(index, records):
        h, n, p = fio.load_fcb_record(spec)
        assert (h, n, p) == (head, samples, packet)
        tok = fio._load_item(spec, "codec_fcb")
        assert tok.shape == (codes.shape[1], 6) and tok.dtype == np.int64
        assert np.array_equal(tok[:, :k], codes[:k].T) and not tok[:, k:].any()
    with pytest.raises(fio.PacketError, match="^k"):
        with fio.FcbWriter(str(tmp_path / "bad.fcb"), 6, 2, 16000, 8) as w:
            w("x", records[0][2], 1)
    with open(str(tmp_path / "not.fcb"), "wb") as f:
        f.write(b"RIFF" + bytes(12))
    with pytest.raises(ValueError, match="FCB1"):
        fio.read_fcb(str(tmp_path / "not.fcb"))


def test_iter_batches_adds_the_stage_counts_for_codec_fcb_only(tmp_path):
    path = str(tmp_path / "codecs.fcb")
    records = write_tiny_fcb(path)
    batches = list(fio.iter_batches([(path + ".scp", "speech", "codec_fcb")], 2))
    assert [keys for keys, _ in batches] == [list(KEYS[:2]), list(KEYS[2:])]
    for (keys, batch), recs in zip(batches, (records[:2], records[2:])):
        assert sorted(batch) == ["speech", "speech_lengths", "speech_n_q"]
        assert batch["speech_n_q"].tolist() == [r[4] for r in recs]
        assert batch["speech_lengths"].tolist() == [r[3].shape[1] for r in recs]
        for i, (_, _, _, codes, k) in enumerate(recs):
            T = codes.shape[1]
            assert np.array_equal(batch["speech"][i, :T, :k].numpy(), codes[:k].T) and not batch["speech"][i, :T, k:].any()
    # any other type keeps its two entries
    txt = tmp_path / "codecs.txt"
    txt.write_text("u0 [[[1, 2, 3], [4, 5, 6]]]\n")
    (_, batch), = fio.iter_batches([(str(txt), "speech", "codec_json")], 1)
    assert sorted(batch) == ["speech", "speech_lengths"]


def test_the_committed_fixture_is_what_the_packer_writes_today(tmp_path):
    """the format cannot drift silently: tests/golden/fcb_tiny.fcb was made by write_tiny_fcb and committed"""
    path = str(tmp_path / "codecs.fcb")
    write_tiny_fcb(path)
    with open(path, "rb") as f, open(os.path.join(GOLD, "fcb_tiny.fcb"), "rb") as g:
        made, kept = f.read(), g.read()
    assert len(kept) < 1024 and made == kept
    head, recs = fio.read_fcb(os.path.join(GOLD, "fcb_tiny.fcb"))
    assert [k for k, _, _ in recs] == list(KEYS) and head["bits"] == 6
    for key, _, packet in recs:
        tok, k, bits = fio.unpack_packet(packet)
        assert fio.pack_codes(tok, k, bits, layout="tq") == packet


def test_the_header_documents_the_entry_points_and_the_abi_stays():
    with open(os.path.join(ROOT, "include", "funcodec_amd.h")) as f:
        text = f.read()
    assert re.search(r"#define FC_ABI_VERSION 7\b", text) and _lib.FC_ABI_VERSION == 7
    assert _lib.load().fc_abi_version() == 7
    for name in ("fc_code_packet_pitch", "fc_code_packet_bytes", "fc_codes_pack", "fc_codes_unpack"):
        assert name in _lib.SYMBOLS
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:size_t|int) " + name + r"\(", text, re.S)
        assert m and "csrc/code_pack_kernels.h" in m.group(1), name          # each entry states the rule by reference to the kernel header
    with open(os.path.join(ROOT, "funcodec_amd", "csrc", "code_pack_kernels.h")) as f:
        rule = f.read()
    for word in ("frames (u32)", "mode = 0", "LSB first", "pad bits are 0", "rounded up to 16"):
        assert word in rule, word
    from funcodec_amd import build
    assert "code_pack_kernels.h" in build.HEADERS and "code_pack_kernels.hip" in build.sources()


def test_the_bit_rate_of_a_packet_is_the_bit_width_asked_for():
    """ds640 at bit_width = 6000: 25 frames a second, 10 bits a code -> 24 stages, and the payload is those bits rounded up to a byte"""
    arch = arch_from_config(recipe_config("ds640"))
    bits = fio.code_bits(arch.codebook_size)
    k = arch.num_quantizers_for_bandwidth(6000)
    assert bits == 10 and k == 6000 // (bits * arch.sample_rate // arch.encoder_hop_length) == 24
    for seconds in (1, 10, 7):
        frames = -(-seconds * arch.sample_rate // arch.encoder_hop_length)
        packet = fio.pack_codes(seeded_codes(bits, frames, n_q=arch.num_quantizers), k, bits)
        payload = len(packet) - 8
        assert payload == -(-k * bits * frames // 8)
        assert 8 * payload / seconds == 8 * -(-k * bits * frames // 8) / seconds
        if seconds == 10:
            assert 8 * payload / seconds == 6000.0          # 250 frames x 24 stages x 10 bits: a whole number of bytes
