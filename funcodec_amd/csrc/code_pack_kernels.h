// The codec's bit stream: one self-describing packet per batch row, written and read on the device (launched by code_pack_kernels.hip).
// The reference has no bit stream to match (funcodec/modules/quantization/binary.py is never imported, and its `push` reinterprets the
// value as float32 bits): this header is the format's specification; funcodec_amd/io.py restates it in numpy for machines without a GPU.
//
// THE PACKET.  bits = ceil(log2(codebook_size)).  A packet is an 8-byte header followed by the payload, all little-endian:
//     bytes 0..3   frames (u32)
//     byte  4      k, the row's stage count (1 .. n_q)
//     byte  5      bits
//     byte  6      mode = 0 (one count per packet); any other mode is refused by name (the place of a later count per frame)
//     byte  7      0
//   Payload: value j = t * k + i is codes[i][b][t] (frame-major, stage-minor: a decoder can start on a prefix), taken modulo 2^bits.
//   Value j occupies stream bits [j * bits, (j + 1) * bits); stream bit p is bit p & 7 of payload byte p >> 3 (LSB first, the order
//   EnCodec's published unpacker reads).  Payload bytes = ceil(frames * k * bits / 8); pad bits are 0.
//   code_packet_bytes(frames, k, bits) = 8 + that.
//
// THE DEVICE ROW.  packets u8 [B][pitch] with pitch >= code_packet_pitch(frames_max, n_q, bits) = the largest packet rounded up to 16.
// Every byte behind a row's packet, up to the pitch, is written as 0: the buffer is a pure function of its inputs, and one copy of
// [B][pitch] carries everything a receiver needs.
//
// Not built: a count per frame (mode 1), entropy coding, a decode that reads packets directly (decoding is unpack, then the row counts
// of the headers, then the decode calls there are).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace fc {

constexpr int kPacketHeaderBytes = 8;
constexpr int kPackTileFrames = 64;      // frames per workgroup of code_pack_kernel: 64 k bits is a multiple of 32, so tiles never share a word

// host arithmetic of the format (0 for arguments outside it: frames < 0, k outside 1..255, bits outside 1..16)
inline size_t code_packet_bytes(long long frames, int k, int bits) {
    if (frames < 0 || k < 1 || k > 255 || bits < 1 || bits > 16) return 0;
    return (size_t)kPacketHeaderBytes + (size_t)(((unsigned long long)frames * (unsigned)k * (unsigned)bits + 7) / 8);
}
inline size_t code_packet_pitch(long long frames, int n_q, int bits) {
    const size_t n = code_packet_bytes(frames, n_q, bits);
    return n ? (n + 15) / 16 * 16 : 0;
}

// codes dev i64 [n_q][B][Tf]; frames_rows, n_q_rows dev i32 [B] or null (all Tf / all n_q), read and clamped on the device (frames to
// [0, Tf], k to [1, n_q]): nothing behind a row's frames or k is read.  packets dev u8 [B][pitch], 4-byte aligned, pitch a multiple of 4
// and >= code_packet_pitch(Tf, n_q, bits).  Every 32-bit word of the buffer is written by exactly one thread; no atomics.
hipError_t launch_code_pack(const int64_t* codes, int B, int Tf, int n_q, int bits, const int32_t* frames_rows, const int32_t* n_q_rows,
                            uint8_t* packets, size_t pitch, hipStream_t st);

// tokens dev i64 [B][Tf][n_q] (the layout every decode call takes): zeros at stages >= k and frames >= frames of the row's header, which
// is read and clamped on the device (frames to [0, Tf], k to [1, n_q]); one thread per token.
hipError_t launch_code_unpack(const uint8_t* packets, size_t pitch, int B, int Tf, int n_q, int bits, int64_t* tokens, hipStream_t st);

}  // namespace fc
