// The codec's bit stream: one self-describing packet per batch row, written and read on the device (launched by code_pack_kernels.hip).
// The reference has no bit stream to match (funcodec/modules/quantization/binary.py is never imported, and its `push` reinterprets the
// value as float32 bits): this header is the format's specification; funcodec_amd/io.py restates it in numpy for machines without a GPU.
//
// THE PACKET.  bits = ceil(log2(codebook_size)).  A packet is an 8-byte header followed by the payload, all little-endian:
//     bytes 0..3   frames (u32)
//     byte  4      k, the row's stage count (1 .. n_q)
//     byte  5      bits
//     byte  6      mode = 0 (one count per packet); mode = 1 is a count per frame (MODE 1 below); any other mode is refused by name
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
// MODE 1, A COUNT PER FRAME (launched by code_pack_frames_kernels.hip; the counts are those of rvq_rate_kernels.h).  Header, 8 bytes:
//     bytes 0..3   frames (u32)
//     byte  4      kmax (1 .. n_q): the row's largest frame count, raised to 1 if it is 0
//     byte  5      bits
//     byte  6      mode = 1
//     byte  7      0
//   Counts section: cbits = the bit length of kmax (1 .. 8).  The count k_t of frame t (0 .. kmax) occupies section bits
//   [t * cbits, (t + 1) * cbits), LSB first as above.  The section is 4 * ceil(frames * cbits / 32) bytes, so the codes start on a 32-bit
//   word; its pad bits are 0.
//   Codes section: with S_t = the sum of k_u over u < t, value j = S_t + i for i < k_t is codes[i][b][t] modulo 2^bits and occupies
//   section bits [j * bits, (j + 1) * bits), LSB first.  The section is ceil(S_frames * bits / 8) bytes; its pad bits are 0.  The layout
//   is frame-major: with the counts section in hand, any prefix of the codes section decodes.
//   frame_packet_bytes(frames, kmax, n_codes, bits) = 8 + the counts section + the codes section with S_frames = n_codes.
//   frame_packet_pitch(frames_max, n_q, bits) = the largest such packet (kmax = n_q, every count n_q) rounded up to 16; every byte behind
//   a row's packet up to the pitch is written as 0, as in mode 0.
//   Packing: the exclusive scan S of the clamped counts (a count to [0, n_q], 0 behind the row's frames clamped to [0, Tf]) lives in a
//   caller-given workspace, one i32 table [B][Tf + 1]; the scan launch also writes the row's header.  Then one thread per 32-bit word
//   behind the header: a counts word gathers its counts; a codes word searches S (binary) for the frame of the first value that touches
//   it and walks the values from there.  Every word of a row has exactly one writer, plain stores from consecutive lanes, no atomics;
//   nothing behind a frame's count or a row's frames is read.
//   Unpacking writes tokens [B][Tf][n_q] (zeros behind counts and frames) and n_q_frames [B][Tf].  A row of mode 0 in the same buffer
//   reads as k_t = k inside its frames (any mode byte other than 1 is read as mode 0: a host validates headers, the device only must
//   not be led astray).  Header and counts are clamped: frames to [0, Tf], kmax (mode 0: k) to [1, n_q], a count to [0, kmax]; the codes section
//   begins where the header's own (unclamped) frames put it, so the first Tf frames of a longer packet decode; a value whose bits would
//   lie behind the row's pitch is 0.  A hostile packet can index nothing outside its row.
//
// Not built: entropy coding, a decode that reads packets directly (decoding is unpack, then the counts per row or frame, then the decode
// calls there are).  Sessions opened per frame write and read mode 1 through these launches (fc_engine_set_floor_frames,
// fc_engine_set_push_frame_nq); a count per frame by target SNR in sessions is not built.
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

// ---- mode 1 (code_pack_frames_kernels.hip) ----
inline int frame_count_bits(int kmax) { int c = 0; while (kmax > 0) { ++c; kmax >>= 1; } return c; }
// host arithmetic of mode 1 (0 for arguments outside the format: frames < 0, kmax outside 1..255, n_codes outside 0..frames kmax, bits outside 1..16)
inline size_t frame_packet_bytes(long long frames, int kmax, long long n_codes, int bits) {
    if (frames < 0 || kmax < 1 || kmax > 255 || bits < 1 || bits > 16 || n_codes < 0 || n_codes > frames * kmax) return 0;
    const unsigned long long cw = ((unsigned long long)frames * (unsigned)frame_count_bits(kmax) + 31) / 32;
    return (size_t)kPacketHeaderBytes + (size_t)(4 * cw) + (size_t)(((unsigned long long)n_codes * (unsigned)bits + 7) / 8);
}
inline size_t frame_packet_pitch(long long frames, int n_q, int bits) {
    const size_t n = frame_packet_bytes(frames, n_q, frames * (long long)n_q, bits);
    return n ? (n + 15) / 16 * 16 : 0;
}
inline size_t frame_pack_workspace_bytes(long long B, long long Tf) { return B < 1 || Tf < 1 ? 0 : (size_t)B * (size_t)(Tf + 1) * sizeof(int32_t); }

// codes dev i64 [n_q][B][Tf]; frames_rows dev i32 [B] or null (all Tf); n_q_frames dev i32 [B][Tf] (never null), both read and clamped on
// the device.  packets dev u8 [B][pitch], 4-byte aligned, pitch a multiple of 4 and >= frame_packet_pitch(Tf, n_q, bits); scan: the
// workspace, i32 [B][Tf + 1].  Tf * n_q fits an i32.  Two launches.
hipError_t launch_code_pack_frames(const int64_t* codes, int B, int Tf, int n_q, int bits, const int32_t* frames_rows, const int32_t* n_q_frames,
                                   uint8_t* packets, size_t pitch, int32_t* scan, hipStream_t st);

// packets of either mode -> tokens dev i64 [B][Tf][n_q] and n_q_frames dev i32 [B][Tf]; scan: the workspace as above.  Two launches.
hipError_t launch_code_unpack_frames(const uint8_t* packets, size_t pitch, int B, int Tf, int n_q, int bits, int64_t* tokens, int32_t* n_q_frames,
                                     int32_t* scan, hipStream_t st);

}  // namespace fc
