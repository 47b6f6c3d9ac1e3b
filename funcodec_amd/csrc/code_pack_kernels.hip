// gfx950 (MI355X / CDNA4) kernels of the codec's bit stream: codes [n_q][B][Tf] -> one packet per row, and back to the token layout of
// the decode calls.  code_pack_kernels.h states the packet.  Integer work only, 64-lane wavefronts; both kernels move about the size of
// the codes once and are bound by their launch.
#include "code_pack_kernels.h"

#include <string>

#include "../../include/funcodec_amd.h"

// the library's thread-local error message (engine.hip)
extern "C" void fc_set_last_error_(const char* msg);

namespace fc {

namespace {
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
}  // namespace

// One workgroup: one row b (blockIdx.y) and one tile of 64 frames (blockIdx.x).  The tile's codes are read coalesced along t, one stage
// after another, and laid into LDS as 16-bit values in stream order (vals[tl * k + i]); values behind the row's frames are 0 and are not
// read.  Then every thread assembles whole 32-bit words from LDS: the tile's 64 k bits bits are 2 k bits words, so a word belongs to one
// tile.  Tile 0 writes the header; the grid's last tile also writes the zeros from the end of its own words to the pitch.  Every word of the
// row therefore has exactly one writer, with plain (vector) dword stores, consecutive lanes on consecutive words.
__global__ __launch_bounds__(256) void code_pack_kernel(const int64_t* __restrict__ codes, int B, int Tf, int n_q, int bits,
                                                        const int32_t* __restrict__ frames_rows, const int32_t* __restrict__ n_q_rows,
                                                        uint32_t* __restrict__ out, unsigned row_words) {
    extern __shared__ uint16_t vals[];      // [64][k]
    const int tid = threadIdx.x, b = blockIdx.y;
    const unsigned ti = blockIdx.x, ntiles = gridDim.x;
    const int frames = clampi(frames_rows ? frames_rows[b] : Tf, 0, Tf);
    const int k = clampi(n_q_rows ? n_q_rows[b] : n_q, 1, n_q);
    const unsigned mask = (1u << bits) - 1u;
    const long long t0 = (long long)ti * kPackTileFrames;
    for (int e = tid; e < k * kPackTileFrames; e += 256) {
        const int i = e >> 6, tl = e & 63;
        const long long t = t0 + tl;
        unsigned v = 0;
        if (t < frames) v = (unsigned)codes[((size_t)i * B + b) * Tf + t] & mask;
        vals[tl * k + i] = (uint16_t)v;
    }
    __syncthreads();
    uint32_t* row = out + (size_t)b * row_words;
    if (ti == 0 && tid == 0) {
        row[0] = (uint32_t)frames;
        row[1] = (uint32_t)k | ((uint32_t)bits << 8);       // mode 0, byte 7 = 0
    }
    const size_t payload_words = row_words - 2;
    const size_t wpt = (size_t)2 * k * bits;                // words of a tile
    const size_t tile_lo = ti * wpt, tile_hi = tile_lo + wpt;
    const size_t w_lo = tile_lo < payload_words ? tile_lo : payload_words;
    const size_t w_hi = (ti == ntiles - 1 || tile_hi > payload_words) ? payload_words : tile_hi;
    for (size_t w = w_lo + tid; w < w_hi; w += 256) {
        uint32_t word = 0;
        if (w < tile_hi) {
            const int P = (int)(w - tile_lo) * 32;          // first bit of the word inside the tile (< 64 * 255 * 16)
            int j = P / bits;
            int shift = j * bits - P;                       // <= 0: value j begins at or in front of the word
            while (shift < 32) {                            // value j begins inside the word, hence inside the tile: j < 64 k
                const uint32_t v = vals[j];
                word |= shift >= 0 ? v << shift : v >> -shift;
                shift += bits;
                ++j;
            }
        }
        row[2 + w] = word;
    }
}

hipError_t launch_code_pack(const int64_t* codes, int B, int Tf, int n_q, int bits, const int32_t* frames_rows, const int32_t* n_q_rows,
                            uint8_t* packets, size_t pitch, hipStream_t st) {
    if (!codes || !packets || B < 1 || B > 65535 || Tf < 1 || n_q < 1 || n_q > 255 || bits < 1 || bits > 16) return hipErrorInvalidValue;
    if (pitch % 4 != 0 || ((uintptr_t)packets & 3) != 0 || pitch < code_packet_pitch(Tf, n_q, bits) || pitch / 4 > 0xffffffffull)
        return hipErrorInvalidValue;
    const unsigned tiles = (unsigned)(((long long)Tf + kPackTileFrames - 1) / kPackTileFrames);
    const size_t lds = (size_t)n_q * kPackTileFrames * sizeof(uint16_t);       // <= 32640 bytes
    hipLaunchKernelGGL(code_pack_kernel, dim3(tiles, B), dim3(256), lds, st, codes, B, Tf, n_q, bits, frames_rows, n_q_rows,
                       reinterpret_cast<uint32_t*>(packets), (unsigned)(pitch / 4));
    return hipGetLastError();
}

// One thread per token (b, t, i).  The row's header is read and clamped here; a token inside the row's frames and count reads the one or
// two payload words that hold its bits (both inside the payload: the value ends in front of the payload's end), any other token is 0.
__global__ __launch_bounds__(256) void code_unpack_kernel(const uint32_t* __restrict__ in, unsigned row_words, size_t total, int Tf, int n_q,
                                                          int bits, int64_t* __restrict__ tokens) {
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= total) return;
    const int i = (int)(n % n_q);
    const size_t bt = n / n_q;
    const int t = (int)(bt % Tf);
    const size_t b = bt / Tf;
    const uint32_t* row = in + b * row_words;
    const uint32_t f = row[0];
    const int frames = f > (uint32_t)Tf ? Tf : (int)f;
    const int k = clampi((int)(row[1] & 0xffu), 1, n_q);
    int64_t v = 0;
    if (t < frames && i < k) {
        const unsigned long long P = ((unsigned long long)t * k + i) * bits;
        const size_t w = (size_t)(P >> 5);
        const int off = (int)(P & 31);
        uint32_t x = row[2 + w] >> off;
        if (off + bits > 32) x |= row[2 + w + 1] << (32 - off);
        v = (int64_t)(x & ((1u << bits) - 1u));
    }
    tokens[n] = v;
}

hipError_t launch_code_unpack(const uint8_t* packets, size_t pitch, int B, int Tf, int n_q, int bits, int64_t* tokens, hipStream_t st) {
    if (!packets || !tokens || B < 1 || Tf < 1 || n_q < 1 || n_q > 255 || bits < 1 || bits > 16) return hipErrorInvalidValue;
    if (pitch % 4 != 0 || ((uintptr_t)packets & 3) != 0 || pitch < code_packet_pitch(Tf, n_q, bits) || pitch / 4 > 0xffffffffull)
        return hipErrorInvalidValue;
    const size_t total = (size_t)B * Tf * n_q;
    const size_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(code_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(packets),
                       (unsigned)(pitch / 4), total, Tf, n_q, bits, tokens);
    return hipGetLastError();
}

}  // namespace fc

// ---- the C ABI of the bit stream (include/funcodec_amd.h): engine-free ------------------------------------------------------------
namespace {
int fail(const std::string& msg) { fc_set_last_error_(msg.c_str()); return 1; }

// what both calls refuse before any launch, naming the argument
int code_pack_check(const char* fn, const void* a, const char* a_name, const void* b, const char* b_name, int B, int Tf, int n_q, int bits,
                    const void* packets, size_t pitch) {
    const std::string f = std::string(fn) + ": ";
    if (bits < 1 || bits > 16) return fail(f + "bits lies in 1..16, got " + std::to_string(bits));
    if (n_q < 1 || n_q > 255) return fail(f + "n_q lies in 1..255 (the header's count is one byte), got " + std::to_string(n_q));
    if (B < 1 || B > 65535) return fail(f + "B lies in 1..65535, got " + std::to_string(B));
    if (Tf < 1) return fail(f + "Tf is at least 1, got " + std::to_string(Tf));
    const size_t need = fc::code_packet_pitch(Tf, n_q, bits);
    if (pitch < need || pitch % 4 != 0 || pitch / 4 > 0xffffffffull)
        return fail(f + "pitch must be a multiple of 4 and at least fc_code_packet_pitch = " + std::to_string(need) + ", got " + std::to_string(pitch));
    if (!a) return fail(f + a_name + " is null");
    if (!b) return fail(f + b_name + " is null");
    if (((uintptr_t)packets & 3) != 0) return fail(f + "packets must be 4-byte aligned");
    return 0;
}

int launched(const char* fn, hipError_t e) { return e == hipSuccess ? 0 : fail(std::string(fn) + ": " + hipGetErrorString(e)); }
}  // namespace

extern "C" {

size_t fc_code_packet_pitch(int frames, int n_q, int bits) { return fc::code_packet_pitch(frames, n_q, bits); }

size_t fc_code_packet_bytes(int frames, int k, int bits) { return fc::code_packet_bytes(frames, k, bits); }

int fc_codes_pack(const int64_t* codes, int B, int Tf, int n_q, int bits, const int32_t* frames_rows, const int32_t* n_q_rows, uint8_t* packets,
                  size_t pitch, void* stream) {
    if (code_pack_check("fc_codes_pack", codes, "codes", packets, "packets", B, Tf, n_q, bits, packets, pitch)) return 1;
    return launched("fc_codes_pack", fc::launch_code_pack(codes, B, Tf, n_q, bits, frames_rows, n_q_rows, packets, pitch, (hipStream_t)stream));
}

int fc_codes_unpack(const uint8_t* packets, size_t pitch, int B, int Tf, int n_q, int bits, int64_t* tokens, void* stream) {
    if (code_pack_check("fc_codes_unpack", packets, "packets", tokens, "tokens", B, Tf, n_q, bits, packets, pitch)) return 1;
    return launched("fc_codes_unpack", fc::launch_code_unpack(packets, pitch, B, Tf, n_q, bits, tokens, (hipStream_t)stream));
}

}  // extern "C"
