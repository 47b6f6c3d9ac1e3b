"""Batch I/O and wire formats around the hot path: what
`funcodec/bin/codec_inference.py:227-378` reads and writes, without torchaudio / kaldiio / librosa.

* wav in:  first channel as float32 in [-1, 1)  (``torchaudio.load(x)[0][0]``, iterable_dataset.py:84)
* scp in:  ``<uttid> <path>`` lines; ``codec_json`` lines ``<uttid> [[[...] x n_q]]`` (iterable_dataset.py:54-58)
* batches: shorter items are WRAP-padded with ``np.pad(mode="wrap")`` (nets_utils.py:65-98, codec_inference.py:257-261)
* out:     ``codecs.txt`` jsonl (codec_inference.py:288-299), Kaldi ``ark,scp`` float matrices (:292-294, :301-311),
           PCM16 wav with peak rescale to 0.99 (``save_audio`` :153-161)
* packets: the codec's own bit stream, ``codecs.fcb`` (not in the reference; csrc/code_pack_kernels.h states the packet)
"""
from __future__ import annotations

import json
import os
import struct
import wave
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import ctypes as C

import numpy as np
import torch

_NATIVE = False


def _native():
    """The engine library's host-side wire-format helpers (fc_format_codec_json, fc_write_wav_pcm16), or None when the library has not
    been built (pure-Python formatting then; the compute path has no such fallback)."""
    global _NATIVE
    if _NATIVE is False:
        try:
            from . import _lib
            _NATIVE = _lib.load()
        except Exception:                      # noqa: BLE001 -- I/O helpers only
            _NATIVE = None
    return _NATIVE


# ------------------------------------------------------------------------------------------------
# wav
# ------------------------------------------------------------------------------------------------
def read_wav(path: str) -> Tuple[np.ndarray, int]:
    """First channel of a RIFF wav as float32 (PCM16/32 scaled by 2^15 / 2^31, float passed through)."""
    try:                                   # plain PCM: the stdlib reader is ~25x faster than scipy's chunk walker (0.13 vs 3.5 ms per 10 s)
        with wave.open(path, "rb") as f:
            ch, width, sr, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
            if width in (2, 4):
                data = np.frombuffer(f.readframes(n), dtype=np.int16 if width == 2 else np.int32).reshape(-1, ch)[:, 0]
                scale = 32768.0 if width == 2 else 2147483648.0
                x = data.astype(np.float32) / np.float32(scale) if width == 2 else (data.astype(np.float64) / scale).astype(np.float32)
                return np.ascontiguousarray(x), int(sr)
    except (wave.Error, EOFError):         # float / extensible / 8-bit files: scipy
        pass
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.ndim > 1:
        data = data[:, 0]
    if data.dtype == np.int16:
        x = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        x = (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    else:
        x = data.astype(np.float32)
    return np.ascontiguousarray(x), int(sr)


def save_audio(wav: torch.Tensor, path: str, sample_rate: int, rescale: bool = False) -> None:
    """codec_inference.py:153-161: peak-rescale to 0.99 (or clamp), then 16-bit PCM.  Mono float32 goes through the library's
    fc_write_wav_pcm16 (same arithmetic, one pass in C; byte-identical files, tests/test_io.py)."""
    limit = 0.99
    wav = torch.as_tensor(wav).detach().float().cpu()
    if wav.dim() == 1:
        wav = wav[None]
    if wav.shape[0] == 1 and _native() is not None:
        x = wav[0].contiguous()
        if _native().fc_write_wav_pcm16(os.fsencode(path), x.data_ptr(), x.numel(), int(sample_rate), int(bool(rescale))) != 0:
            raise OSError(_native().fc_last_error().decode("utf-8", "replace"))
        return
    mx = wav.abs().max()
    if rescale:
        wav = wav * min(limit / mx, 1) if mx > 0 else wav
    else:
        wav = wav.clamp(-limit, limit)
    pcm = torch.clamp((wav * 32768.0).round(), -32768, 32767).to(torch.int16).numpy()
    with wave.open(path, "wb") as f:
        f.setnchannels(pcm.shape[0])
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(np.ascontiguousarray(pcm.T).tobytes())


# ------------------------------------------------------------------------------------------------
# sample-rate conversion (reference: torchaudio.functional.resample, codec_inference.py:318-322,352-356)
# ------------------------------------------------------------------------------------------------
def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6,
             rolloff: float = 0.99) -> torch.Tensor:
    """Band-limited sinc interpolation with a Hann window: the algorithm torchaudio publishes as
    ``torchaudio.functional.resample(..., resampling_method="sinc_interp_hann")`` with its default width / roll-off
    (torchaudio is not installed here, so this is a restatement of that algorithm, not a golden-pinned copy:
    polyphase kernel bank [new/gcd, 1, 2*width + orig/gcd], conv1d with stride orig/gcd, output length
    ceil(new * T / orig)).  Runs wherever `waveform` lives (torch ops: plumbing, not the hot path)."""
    import math
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("sample rates must be positive")
    if orig_freq == new_freq:
        return waveform
    g = math.gcd(orig_freq, new_freq)
    of, nf = orig_freq // g, new_freq // g
    base = min(of, nf) * rolloff
    width = math.ceil(lowpass_filter_width * of / base)
    dt = torch.float64
    idx = torch.arange(-width, width + of, dtype=dt)[None, None] / of
    t = torch.arange(0, -nf, -1, dtype=dt)[:, None, None] / nf + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / of)
    kern = kern.to(dtype=waveform.dtype, device=waveform.device)
    shape = waveform.shape
    x = waveform.reshape(-1, shape[-1])
    n, length = x.shape
    x = torch.nn.functional.pad(x, (width, width + of))
    y = torch.nn.functional.conv1d(x[:, None], kern, stride=of).transpose(1, 2).reshape(n, -1)
    target = int(math.ceil(nf * length / of))
    return y[..., :target].reshape(shape[:-1] + (target,))


# ------------------------------------------------------------------------------------------------
# Kaldi ark / scp (binary float matrices only: what the reference writes with kaldiio "ark,scp,f:")
# ------------------------------------------------------------------------------------------------
class KaldiMatrixWriter:
    """``kaldiio.WriteHelper("ark,scp,f:<prefix>.ark,<prefix>.scp")`` for float32 matrices."""

    def __init__(self, prefix: str):
        self.ark_path = prefix + ".ark"
        self._ark = open(self.ark_path, "wb")
        self._scp = open(prefix + ".scp", "wt")

    def __call__(self, key: str, mat: np.ndarray) -> None:
        mat = np.ascontiguousarray(mat, dtype=np.float32)
        assert mat.ndim == 2
        self._ark.write(key.encode() + b" ")
        off = self._ark.tell()
        self._ark.write(b"\0BFM " + b"\4" + struct.pack("<i", mat.shape[0]) + b"\4" + struct.pack("<i", mat.shape[1]))
        self._ark.write(mat.tobytes())
        self._scp.write(f"{key} {self.ark_path}:{off}\n")

    def close(self) -> None:
        self._ark.close()
        self._scp.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def load_kaldi_mat(spec: str) -> np.ndarray:
    """``<ark path>:<offset>`` -> float32 matrix (kaldiio.load_mat for the binary FM / DM case)."""
    path, _, off = spec.rpartition(":")
    with open(path, "rb") as f:
        f.seek(int(off))
        if f.read(2) != b"\0B":
            raise ValueError(f"{spec}: not a binary Kaldi object")
        tok = f.read(3)
        if tok not in (b"FM ", b"DM "):
            raise ValueError(f"{spec}: unsupported Kaldi type {tok!r}")
        assert f.read(1) == b"\4"
        rows = struct.unpack("<i", f.read(4))[0]
        assert f.read(1) == b"\4"
        cols = struct.unpack("<i", f.read(4))[0]
        dt = np.float32 if tok == b"FM " else np.float64
        data = np.frombuffer(f.read(rows * cols * np.dtype(dt).itemsize), dtype=dt)
    return data.reshape(rows, cols).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# codec index text format
# ------------------------------------------------------------------------------------------------
def format_codec_line(key: str, indices: Sequence[torch.Tensor], batch_id: int, length: int) -> str:
    """codec_inference.py:295-299: ``<key> [[[T ints] x n_q]]`` (n_frame x n_q x T, n_frame always 1).  One frame of int64 codes on
    the host goes through the library's fc_format_codec_json (byte-identical to json.dumps, ~50x faster; tests/test_io.py)."""
    if len(indices) == 1 and _native() is not None:
        x = indices[0]
        if isinstance(x, torch.Tensor) and x.dtype == torch.int64 and x.device.type == "cpu" and x.dim() == 3 and x.is_contiguous():
            lib = _native()
            n_q, B, T = x.shape
            cap = lib.fc_codec_json_bound(n_q, int(length))
            buf = C.create_string_buffer(cap)
            written = C.c_size_t(0)
            if lib.fc_format_codec_json(x.data_ptr(), n_q, B, T, int(batch_id), int(length), buf, cap, C.byref(written)) == 0:
                return key + " " + buf.raw[:written.value].decode("ascii") + "\n"
    to_write = [x[:, batch_id, :length].cpu().numpy().tolist() for x in indices]
    return key + " " + json.dumps(to_write) + "\n"


def load_codec_json(json_str: str) -> np.ndarray:
    """iterable_dataset.py:54-58 -> [T, n_q] int64."""
    array = np.array(json.loads(json_str))
    if array.ndim == 3:
        array = array[0]
    return array.T


# ------------------------------------------------------------------------------------------------
# the bit stream: one packet per utterance (csrc/code_pack_kernels.h states the packet; this is its numpy restatement, so a machine
# without a GPU reads and writes the format) and the container codecs.fcb
# ------------------------------------------------------------------------------------------------
PACKET_HEADER_BYTES = 8


class PacketError(ValueError):
    """a packet that is not one: ``field`` names what is wrong (mode, bits, k, length)"""

    def __init__(self, field: str, msg: str):
        super().__init__(f"{field}: {msg}")
        self.field = field


def code_bits(codebook_size: int) -> int:
    """bits = ceil(log2(codebook_size)), at least 1"""
    return max(1, int(codebook_size - 1).bit_length())


def packet_bytes(frames: int, k: int, bits: int) -> int:
    """8 + ceil(frames k bits / 8) (fc_code_packet_bytes)"""
    return PACKET_HEADER_BYTES + (int(frames) * int(k) * int(bits) + 7) // 8


def packet_pitch(frames: int, n_q: int, bits: int) -> int:
    """the largest packet rounded up to 16 (fc_code_packet_pitch)"""
    return (packet_bytes(frames, n_q, bits) + 15) // 16 * 16


def parse_packet_header(buf, n_q: Optional[int] = None, bits: Optional[int] = None, exact: Optional[bool] = True) -> Tuple[int, int, int, int]:
    """(frames, k, bits, packet length) of the packet at the start of ``buf``, every field checked: mode 0, bits in 1..16 (and the
    expected ``bits`` if given), k in 1..255 (and <= ``n_q`` if given), and a length of exactly (``exact``) or at least the packet's
    8 + ceil(frames k bits / 8) bytes (``exact=None``: ``buf`` is the header alone).  Raises PacketError naming the field."""
    buf = buf if isinstance(buf, (bytes, bytearray)) else bytes(buf)
    if len(buf) < PACKET_HEADER_BYTES:
        raise PacketError("length", f"a packet begins with an {PACKET_HEADER_BYTES}-byte header, got {len(buf)} bytes")
    frames, k, b, mode, zero = struct.unpack_from("<IBBBB", buf, 0)
    if mode != 0:
        raise PacketError("mode", f"only mode 0 (one stage count per packet) is defined, got {mode}")
    if not 1 <= b <= 16 or (bits is not None and b != bits):
        raise PacketError("bits", f"{b} bits per code" + (f", expected {bits}" if bits is not None else " lies outside 1..16"))
    if k < 1 or (n_q is not None and k > n_q):
        raise PacketError("k", f"a stage count lies in 1..{255 if n_q is None else n_q}, got {k}")
    need = packet_bytes(frames, k, b)
    if exact is not None and ((len(buf) != need) if exact else (len(buf) < need)):
        raise PacketError("length", f"{frames} frames of {k} stages at {b} bits are {need} bytes, got {len(buf)}")
    return frames, k, b, need


def pack_codes(codes, k: Optional[int] = None, bits: int = 10, frames: Optional[int] = None, layout: str = "qt") -> bytes:
    """One packet from the codes of one utterance: ``codes`` [n_q, T] (``layout="qt"``, a row of an encode call's codes) or [T, n_q]
    (``"tq"``, the decode calls' tokens); the first ``k`` stages (default: all) of the first ``frames`` frames (default: all), each code
    modulo 2^bits."""
    a = np.asarray(codes)
    if a.ndim != 2:
        raise ValueError(f"pack_codes: codes of one utterance are 2-D, got shape {a.shape}")
    if layout not in ("qt", "tq"):
        raise ValueError(f"pack_codes: layout is 'qt' ([n_q, T]) or 'tq' ([T, n_q]), got {layout!r}")
    a = a.T if layout == "qt" else a                         # [T, n_q]
    k = a.shape[1] if k is None else int(k)
    frames = a.shape[0] if frames is None else int(frames)
    if not 1 <= bits <= 16:
        raise PacketError("bits", f"{bits} bits per code lies outside 1..16")
    if not 1 <= k <= min(a.shape[1], 255):
        raise PacketError("k", f"a stage count lies in 1..{min(a.shape[1], 255)}, got {k}")
    if not 0 <= frames <= a.shape[0]:
        raise PacketError("frames", f"the codes hold {a.shape[0]} frames, got {frames}")
    vals = (a[:frames, :k].astype(np.int64).reshape(-1) & ((1 << bits) - 1)).astype(np.uint32)
    stream = ((vals[:, None] >> np.arange(bits, dtype=np.uint32)[None, :]) & 1).astype(np.uint8).reshape(-1)
    return struct.pack("<IBBBB", frames, k, bits, 0, 0) + np.packbits(stream, bitorder="little").tobytes()


def unpack_packet(packet) -> Tuple[np.ndarray, int, int]:
    """(tokens [T, k] int64, k, bits) of one packet; the inverse of pack_codes"""
    packet = bytes(packet)
    frames, k, bits, _ = parse_packet_header(packet)
    stream = np.unpackbits(np.frombuffer(packet, dtype=np.uint8, offset=PACKET_HEADER_BYTES), bitorder="little")[:frames * k * bits]
    vals = (stream.reshape(frames * k, bits).astype(np.int64) << np.arange(bits, dtype=np.int64)[None, :]).sum(1)
    return vals.reshape(frames, k), k, bits


# ---- mode 1: a stage count per frame (csrc/code_pack_kernels.h, "MODE 1") ----
def count_bits(kmax: int) -> int:
    """cbits: the bit length of kmax (1..8 for kmax in 1..255)"""
    return int(kmax).bit_length()


def frame_packet_bytes(frames: int, kmax: int, n_codes: int, bits: int) -> int:
    """8 + 4 ceil(frames cbits / 32) + ceil(n_codes bits / 8) (fc_frame_packet_bytes)"""
    return PACKET_HEADER_BYTES + 4 * ((int(frames) * count_bits(kmax) + 31) // 32) + (int(n_codes) * int(bits) + 7) // 8


def frame_packet_pitch(frames: int, n_q: int, bits: int) -> int:
    """the largest mode-1 packet (kmax = n_q, every count n_q) rounded up to 16 (fc_frame_packet_pitch)"""
    return (frame_packet_bytes(frames, n_q, int(frames) * int(n_q), bits) + 15) // 16 * 16


def packet_mode(buf) -> int:
    """0 (one count per packet) or 1 (a count per frame) of the packet at the start of ``buf``; anything else raises PacketError("mode")"""
    buf = buf if isinstance(buf, (bytes, bytearray)) else bytes(buf)
    if len(buf) < PACKET_HEADER_BYTES:
        raise PacketError("length", f"a packet begins with an {PACKET_HEADER_BYTES}-byte header, got {len(buf)} bytes")
    if buf[6] not in (0, 1):
        raise PacketError("mode", f"modes 0 (one stage count per packet) and 1 (one per frame) are defined, got {buf[6]}")
    return buf[6]


def _bits_lsb(vals: np.ndarray, width: int) -> np.ndarray:
    """the bit stream of ``vals`` at ``width`` bits each, LSB first, as an array of 0 / 1"""
    vals = np.asarray(vals, dtype=np.uint32).reshape(-1)
    return ((vals[:, None] >> np.arange(width, dtype=np.uint32)[None, :]) & 1).astype(np.uint8).reshape(-1)


def _vals_lsb(stream: np.ndarray, n: int, width: int) -> np.ndarray:
    """the first ``n`` values of ``width`` bits of a stream of 0 / 1 (the inverse of _bits_lsb), int64"""
    return (stream[:n * width].reshape(n, width).astype(np.int64) << np.arange(width, dtype=np.int64)[None, :]).sum(1)


def pack_frame_codes(codes, counts, bits: int = 10, frames: Optional[int] = None, layout: str = "qt") -> bytes:
    """One mode-1 packet from the codes of one utterance: ``codes`` [n_q, T] (``"qt"``) or [T, n_q] (``"tq"``) and ``counts`` [T], the
    stage count of every frame (0 .. min(n_q, 255)); the first ``frames`` frames (default: all).  Frame t contributes its first
    counts[t] codes, each modulo 2^bits; nothing behind a count is looked at."""
    a = np.asarray(codes)
    if a.ndim != 2:
        raise ValueError(f"pack_frame_codes: codes of one utterance are 2-D, got shape {a.shape}")
    if layout not in ("qt", "tq"):
        raise ValueError(f"pack_frame_codes: layout is 'qt' ([n_q, T]) or 'tq' ([T, n_q]), got {layout!r}")
    a = a.T if layout == "qt" else a                         # [T, n_q]
    frames = a.shape[0] if frames is None else int(frames)
    if not 1 <= bits <= 16:
        raise PacketError("bits", f"{bits} bits per code lies outside 1..16")
    if not 0 <= frames <= a.shape[0]:
        raise PacketError("frames", f"the codes hold {a.shape[0]} frames, got {frames}")
    k = np.asarray(counts).reshape(-1)
    if k.shape[0] < frames:
        raise PacketError("count", f"{frames} frames need {frames} counts, got {k.shape[0]}")
    k = k[:frames].astype(np.int64)
    top = min(a.shape[1], 255)
    bad = np.nonzero((k < 0) | (k > top))[0]
    if bad.size:
        raise PacketError("count", f"frame {int(bad[0])}: a stage count lies in 0..{top}, got {int(k[bad[0]])}")
    kmax = max(int(k.max()) if frames else 0, 1)
    cbits = count_bits(kmax)
    cstream = np.zeros(32 * ((frames * cbits + 31) // 32), dtype=np.uint8)
    cstream[:frames * cbits] = _bits_lsb(k, cbits)
    keep = np.arange(a.shape[1])[None, :] < k[:, None]       # [frames, n_q], frame-major
    vals = a[:frames][keep].astype(np.int64) & ((1 << bits) - 1)
    return (struct.pack("<IBBBB", frames, kmax, bits, 1, 0) + np.packbits(cstream, bitorder="little").tobytes() +
            np.packbits(_bits_lsb(vals, bits), bitorder="little").tobytes())


def parse_frame_packet(buf, n_q: Optional[int] = None, bits: Optional[int] = None, exact: Optional[bool] = True):
    """(frames, kmax, bits, counts [frames] int64, packet length) of the mode-1 packet at the start of ``buf``, every field checked:
    mode 1, bits in 1..16 (and the expected ``bits``), kmax in 1..255 (and <= ``n_q``), every count <= kmax and the largest one equal to
    kmax (1 if all are 0), and a length of exactly (``exact``) or at least (``exact=False``) the packet's (``exact=None``: ``buf`` is the
    header alone; counts and length are then None).  Raises PacketError naming the field: mode, bits, k, count (with the frame) or length."""
    buf = buf if isinstance(buf, (bytes, bytearray)) else bytes(buf)
    if len(buf) < PACKET_HEADER_BYTES:
        raise PacketError("length", f"a packet begins with an {PACKET_HEADER_BYTES}-byte header, got {len(buf)} bytes")
    frames, kmax, b, mode, _ = struct.unpack_from("<IBBBB", buf, 0)
    if mode != 1:
        raise PacketError("mode", f"a packet with a stage count per frame has mode 1, got {mode}")
    if not 1 <= b <= 16 or (bits is not None and b != bits):
        raise PacketError("bits", f"{b} bits per code" + (f", expected {bits}" if bits is not None else " lies outside 1..16"))
    if kmax < 1 or (n_q is not None and kmax > n_q):
        raise PacketError("k", f"the largest stage count lies in 1..{255 if n_q is None else n_q}, got {kmax}")
    if exact is None:                                        # ``buf`` is the header alone: no counts, no length
        return frames, kmax, b, None, None
    cbits = count_bits(kmax)
    cbytes = 4 * ((frames * cbits + 31) // 32)
    if len(buf) < PACKET_HEADER_BYTES + cbytes:
        raise PacketError("length", f"{frames} frames at {cbits} count bits need a counts section of {cbytes} bytes, got {len(buf) - PACKET_HEADER_BYTES}")
    cstream = np.unpackbits(np.frombuffer(buf, dtype=np.uint8, offset=PACKET_HEADER_BYTES, count=cbytes), bitorder="little")
    counts = _vals_lsb(cstream, frames, cbits)
    bad = np.nonzero(counts > kmax)[0]
    if bad.size:
        raise PacketError("count", f"frame {int(bad[0])}: {int(counts[bad[0]])} stages, more than the packet's largest count {kmax}")
    if max(int(counts.max()) if frames else 0, 1) != kmax:
        raise PacketError("k", f"the header's largest count is {kmax}, the counts' is {max(int(counts.max()) if frames else 0, 1)}")
    need = frame_packet_bytes(frames, kmax, int(counts.sum()), b)
    if exact is not None and ((len(buf) != need) if exact else (len(buf) < need)):
        raise PacketError("length", f"{frames} frames with {int(counts.sum())} codes at {b} bits are {need} bytes, got {len(buf)}")
    return frames, kmax, b, counts, need


def unpack_frame_packet(packet) -> Tuple[np.ndarray, np.ndarray, int]:
    """(tokens [T, kmax] int64 with zeros behind every frame's count, counts [T] int64, bits) of one mode-1 packet; the inverse of
    pack_frame_codes"""
    packet = bytes(packet)
    frames, kmax, bits, counts, _ = parse_frame_packet(packet)
    off = PACKET_HEADER_BYTES + 4 * ((frames * count_bits(kmax) + 31) // 32)
    n = int(counts.sum())
    vals = _vals_lsb(np.unpackbits(np.frombuffer(packet, dtype=np.uint8, offset=off), bitorder="little"), n, bits)
    tokens = np.zeros((frames, kmax), dtype=np.int64)
    tokens[np.arange(kmax)[None, :] < counts[:, None]] = vals
    return tokens, counts, bits


def parse_any_packet(buf, n_q: Optional[int] = None, bits: Optional[int] = None, exact: Optional[bool] = True):
    """(mode, frames, k or kmax, bits, counts [frames] int64, packet length) of a packet of either mode, checked as its own parser checks it"""
    if packet_mode(buf) == 1:
        frames, kmax, b, counts, need = parse_frame_packet(buf, n_q, bits, exact)
        return 1, frames, kmax, b, counts, need
    frames, k, b, need = parse_packet_header(buf, n_q, bits, exact)
    return 0, frames, k, b, None if exact is None else np.full((frames,), k, dtype=np.int64), need


def unpack_any_packet(packet) -> Tuple[np.ndarray, np.ndarray, int]:
    """(tokens [T, k or kmax], counts [T], bits) of a packet of either mode"""
    if packet_mode(packet) == 1:
        return unpack_frame_packet(packet)
    tok, k, bits = unpack_packet(packet)
    return tok, np.full((tok.shape[0],), k, dtype=np.int64), bits


FCB_MAGIC = b"FCB1"
_FCB_HEADER = struct.Struct("<4sBBHII")      # magic, bits, n_q, 0, sample rate, hop
_FCB_RECORD = struct.Struct("<II")           # valid samples, packet length (behind: u16 key length, key)


class FcbWriter:
    """``codecs.fcb``: the file header (magic b"FCB1", u8 bits, u8 n_q, u16 0, u32 sample rate, u32 hop), then one record per utterance:
    u16 key length, key (UTF-8), u32 valid samples, u32 packet length, packet.  ``<path>.scp`` indexes it with lines ``key path:offset``
    as Kaldi arks are indexed; the offset is that of the record's sample count, behind its key."""

    def __init__(self, path: str, bits: int, n_q: int, sample_rate: int, hop: int):
        if not 1 <= bits <= 16 or not 1 <= n_q <= 255:
            raise ValueError(f"FcbWriter: bits in 1..16 and n_q in 1..255, got {bits}, {n_q}")
        self.path, self.bits, self.n_q = path, int(bits), int(n_q)
        self._f = open(path, "wb")
        self._scp = open(path + ".scp", "wt", encoding="utf-8")
        self._f.write(_FCB_HEADER.pack(FCB_MAGIC, self.bits, self.n_q, 0, int(sample_rate), int(hop)))

    def __call__(self, key: str, packet: bytes, samples: int) -> None:
        packet = bytes(packet)
        parse_any_packet(packet, self.n_q, self.bits)       # either mode
        kb = key.encode("utf-8")
        if not 0 < len(kb) < 65536 or any(c.isspace() for c in key):
            raise ValueError(f"FcbWriter: a key is 1..65535 UTF-8 bytes without white space, got {key!r}")
        self._f.write(struct.pack("<H", len(kb)) + kb)
        self._scp.write(f"{key} {self.path}:{self._f.tell()}\n")
        self._f.write(_FCB_RECORD.pack(int(samples), len(packet)) + packet)

    def close(self) -> None:
        self._f.close()
        self._scp.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _fcb_header(f, path: str) -> Dict[str, int]:
    raw = f.read(_FCB_HEADER.size)
    if len(raw) != _FCB_HEADER.size or raw[:4] != FCB_MAGIC:
        raise ValueError(f"{path}: not an FCB1 file")
    _, bits, n_q, _, sr, hop = _FCB_HEADER.unpack(raw)
    return dict(bits=bits, n_q=n_q, sample_rate=sr, hop=hop)


def read_fcb(path: str):
    """(header dict(bits, n_q, sample_rate, hop), [(key, samples, packet)] in file order); every packet's header is checked"""
    out = []
    with open(path, "rb") as f:
        head = _fcb_header(f, path)
        while True:
            raw = f.read(2)
            if not raw:
                break
            key = f.read(struct.unpack("<H", raw)[0]).decode("utf-8")
            samples, n = _FCB_RECORD.unpack(f.read(_FCB_RECORD.size))
            packet = f.read(n)
            parse_any_packet(packet, head["n_q"], head["bits"])
            out.append((key, samples, packet))
    return head, out


def load_fcb_record(spec: str):
    """``<fcb path>:<offset>`` (a line of codecs.fcb.scp) -> (header dict, samples, packet)"""
    path, _, off = spec.rpartition(":")
    with open(path, "rb") as f:
        head = _fcb_header(f, path)
        f.seek(int(off))
        samples, n = _FCB_RECORD.unpack(f.read(_FCB_RECORD.size))
        packet = f.read(n)
    parse_any_packet(packet, head["n_q"], head["bits"])
    return head, samples, packet


def load_fcb_frames(spec: str) -> Tuple[np.ndarray, int, np.ndarray, int]:
    """``<fcb path>:<offset>`` -> (tokens [T, n_q] int64 with zeros behind every frame's count, the largest count, counts [T] int64,
    the packet's mode); n_q is the file's.  A mode-0 packet counts its k in every frame."""
    head, _, packet = load_fcb_record(spec)
    tok, counts, _ = unpack_any_packet(packet)
    out = np.zeros((tok.shape[0], head["n_q"]), dtype=np.int64)
    out[:, :tok.shape[1]] = tok
    return out, tok.shape[1], counts, packet_mode(packet)


def load_fcb_item(spec: str) -> Tuple[np.ndarray, int]:
    """``<fcb path>:<offset>`` -> (tokens [T, n_q] int64 with zeros behind the packet's k, k); n_q is the file's.  For a mode-1 packet k is
    its largest count (load_fcb_frames also gives the counts)."""
    return load_fcb_frames(spec)[:2]


# ------------------------------------------------------------------------------------------------
# scp-driven batching with the reference's wrap padding
# ------------------------------------------------------------------------------------------------
def read_scp(path: str) -> List[Tuple[str, str]]:
    out = []
    with open(path, "rt", encoding="utf-8") as f:
        for line in f:
            line = line.rstrip("\n")
            if not line.strip():
                continue
            key, _, val = line.partition(" ")
            out.append((key, val.strip()))
    return out


def _load_item(value: str, dtype: str) -> np.ndarray:
    if dtype == "sound":
        return read_wav(value)[0]
    if dtype == "codec_json":
        return load_codec_json(value).astype(np.int64)
    if dtype == "kaldi_ark":
        return load_kaldi_mat(value)
    if dtype == "npy":
        return np.load(value)
    if dtype == "codec_fcb":
        return load_fcb_item(value)[0]
    raise NotImplementedError(f"data type {dtype!r} is not supported by funcodec_amd.io")


def pad_list_with_mod(xs: Sequence[np.ndarray], pad_value=0.0, mode: str = "wrap") -> torch.Tensor:
    """nets_utils.py:65-98."""
    max_len = max(x.shape[0] for x in xs)
    if all(x.shape[0] == max_len for x in xs):       # equal lengths: nothing to pad
        return torch.from_numpy(np.stack(xs, 0))
    kw = {"mode": mode}
    if mode == "constant":
        kw["constant_values"] = pad_value
    out = []
    for x in xs:
        pads = [(0, max_len - x.shape[0])] + [(0, 0)] * (x.ndim - 1)
        out.append(torch.from_numpy(np.pad(x, pads if x.ndim > 1 else pads[0], **kw)))
    return torch.stack(out, 0)


def iter_batches(data_path_and_name_and_type: Sequence[Tuple[str, str, str]], batch_size: int,
                 key_file: Optional[str] = None) -> Iterator[Tuple[List[str], Dict[str, torch.Tensor]]]:
    """What build_streaming_iterator + common_collate_fn(pad_mode="wrap") yield at inference
    (codec_inference.py:250-264, collate_fn.py:55-95): ``(keys, {name, name_lengths})`` in scp order."""
    tables = [(name, dtype, dict(read_scp(path)), [k for k, _ in read_scp(path)]) for path, name, dtype in data_path_and_name_and_type]
    keys = [k for k, _ in read_scp(key_file)] if key_file else tables[0][3]
    for i in range(0, len(keys), batch_size):
        bkeys = keys[i:i + batch_size]
        batch: Dict[str, torch.Tensor] = {}
        for name, dtype, table, _ in tables:
            if dtype == "codec_fcb":       # the packets carry each row's stage count: it travels next to the lengths
                pairs = [load_fcb_frames(table[k]) for k in bkeys]
                items = [p[0] for p in pairs]
                batch[name + "_n_q"] = torch.tensor([p[1] for p in pairs], dtype=torch.long)
                if any(p[3] == 1 for p in pairs):      # a count per frame somewhere in the batch: [B, T] int32, zeros behind a row's frames
                    nqf = np.zeros((len(pairs), max(p[2].shape[0] for p in pairs)), dtype=np.int32)
                    for b, p in enumerate(pairs):
                        nqf[b, :p[2].shape[0]] = p[2]
                    batch[name + "_n_q_frames"] = torch.from_numpy(nqf)
            else:
                items = [_load_item(table[k], dtype) for k in bkeys]
            batch[name] = pad_list_with_mod(items, 0.0 if items[0].dtype.kind == "f" else 0, "wrap")
            batch[name + "_lengths"] = torch.tensor([it.shape[0] for it in items], dtype=torch.long)
        yield bkeys, batch
