// gfx950 (MI355X / CDNA4) kernels of the bit stream's mode 1, a stage count per frame: codes [n_q][B][Tf] and counts [B][Tf] -> one packet
// per row, and packets of either mode back to the token layout of the decode calls with the counts beside them.  code_pack_kernels.h
// states the packet.  Integer work only, 64-lane wavefronts; two launches each way (the scan of the counts, then the words / tokens).
#include "code_pack_kernels.h"

#include <string>

#include "../../include/funcodec_amd.h"

// the library's thread-local error message (engine.hip)
extern "C" void fc_set_last_error_(const char* msg);

namespace fc {

namespace {
__device__ __forceinline__ int fclampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int count_bits_dev(int kmax) { return 32 - __clz(kmax); }      // kmax >= 1

// The exclusive scan of one row's counts by one workgroup of 256 threads: thread j owns the frames [j c, (j + 1) c) with c = ceil(Tf / 256),
// sums them, the 256 sums are scanned in LDS, and the thread walks its frames again writing S.  count(t) is called twice per frame and must
// be pure.  scan_row [Tf + 1]; returns (to every thread) the row's total and its largest count.
template <class Count, class Store>
__device__ __forceinline__ void row_scan(int Tf, int* sh /* [256] */, int* shm /* [256] */, int32_t* scan_row, Count count, Store store, int& total,
                                         int& kmax) {
    const int tid = threadIdx.x;
    const int c = (Tf + 255) / 256;
    const long long t0l = (long long)tid * c;
    const int t0 = t0l < Tf ? (int)t0l : Tf, t1 = t0l + c < Tf ? (int)(t0l + c) : Tf;
    int s = 0, m = 0;
    for (int t = t0; t < t1; ++t) {
        const int k = count(t);
        s += k;
        m = k > m ? k : m;
    }
    sh[tid] = s; shm[tid] = m;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {         // inclusive scan of the sums, running maximum beside it
        const int a = tid >= o ? sh[tid - o] : 0, am = tid >= o ? shm[tid - o] : 0;
        __syncthreads();
        sh[tid] += a;
        shm[tid] = am > shm[tid] ? am : shm[tid];
        __syncthreads();
    }
    int run = sh[tid] - s;
    for (int t = t0; t < t1; ++t) {
        const int k = count(t);
        scan_row[t] = run;
        store(t, k);
        run += k;
    }
    total = sh[255];
    kmax = shm[255];
    if (tid == 0) scan_row[Tf] = total;
}
}  // namespace

// One workgroup per row: S [Tf + 1] of the clamped counts, and the row's header (words 0 and 1).
__global__ __launch_bounds__(256) void frame_pack_scan_kernel(int Tf, int n_q, int bits, const int32_t* __restrict__ frames_rows,
                                                              const int32_t* __restrict__ n_q_frames, int32_t* __restrict__ scan,
                                                              uint32_t* __restrict__ out, unsigned row_words) {
    __shared__ int sh[256], shm[256];
    const int b = blockIdx.x;
    const int frames = fclampi(frames_rows ? frames_rows[b] : Tf, 0, Tf);
    const int32_t* kf = n_q_frames + (size_t)b * Tf;
    int total, kmax;
    row_scan(Tf, sh, shm, scan + (size_t)b * (Tf + 1), [&](int t) { return t < frames ? fclampi(kf[t], 0, n_q) : 0; }, [](int, int) {}, total, kmax);
    if (threadIdx.x == 0) {
        uint32_t* row = out + (size_t)b * row_words;
        row[0] = (uint32_t)frames;
        row[1] = (uint32_t)(kmax < 1 ? 1 : kmax) | ((uint32_t)bits << 8) | (1u << 16);      // mode 1, byte 7 = 0
    }
}

// One thread per 32-bit word behind the header (blockIdx.y: the row).  The header and S were written by frame_pack_scan_kernel, earlier on
// the same stream.  A counts word gathers the counts that touch it; a codes word finds the frame of its first value in S and walks on;
// every other word up to the pitch is 0.
__global__ __launch_bounds__(256) void frame_pack_words_kernel(const int64_t* __restrict__ codes, int B, int Tf, int bits,
                                                               const int32_t* __restrict__ scan, uint32_t* __restrict__ out, unsigned row_words) {
    const int b = blockIdx.y;
    const size_t w = 2 + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= row_words) return;
    uint32_t* row = out + (size_t)b * row_words;
    const int32_t* S = scan + (size_t)b * (Tf + 1);
    const int frames = fclampi((int)row[0], 0, Tf);
    const int cbits = count_bits_dev((int)(row[1] & 0xffu));
    const unsigned long long cw = ((unsigned long long)frames * cbits + 31) / 32;
    const unsigned long long u = w - 2;
    uint32_t word = 0;
    if (u < cw) {
        const unsigned long long P = u * 32;
        int t = (int)(P / cbits);
        int shift = (int)((long long)t * cbits - (long long)P);      // <= 0: count t begins at or in front of the word
        while (shift < 32 && t < frames) {
            const uint32_t c = (uint32_t)(S[t + 1] - S[t]);
            word |= shift >= 0 ? c << shift : c >> -shift;
            shift += cbits;
            ++t;
        }
    } else {
        const unsigned long long P = (u - cw) * 32, total = (unsigned long long)S[frames];
        if (P < total * bits) {
            const uint32_t mask = (1u << bits) - 1u;
            unsigned long long j = P / bits;                          // < total
            int shift = (int)((long long)(j * bits) - (long long)P);
            int lo = 0, hi = frames;                                  // the first m in (0, frames] with S[m] > j; S[frames] = total > j
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if ((unsigned long long)S[mid] > j) hi = mid; else lo = mid;
            }
            int t = lo;                                               // S[t] <= j < S[t + 1]
            int i =(int)(j - (unsigned long long)S[t]), kt = S[t + 1] - S[t];
            while (shift < 32 && j < total) {                         // value j is code i of frame t, t < frames and i < kt
                const uint32_t v = (uint32_t)codes[((size_t)i * B + b) * Tf + t] & mask;
                word |= shift >= 0 ? v << shift : v >> -shift;
                shift += bits;
                ++j;
                if (++i >= kt) {
                    i = 0;
                    do { ++t; } while (t < frames && (kt = S[t + 1] - S[t]) == 0);
                }
            }
        }
    }
    row[w] = word;
}

namespace {
bool frames_args_ok(int B, int Tf, int n_q, int bits, const void* packets, size_t pitch, size_t need) {
    if (B < 1 || B > 65535 || Tf < 1 || n_q < 1 || n_q > 255 || bits < 1 || bits > 16 || (long long)Tf * n_q > 0x7fffffffLL) return false;
    return pitch % 4 == 0 && ((uintptr_t)packets & 3) == 0 && pitch >= need && pitch / 4 <= 0xffffffffull;
}
}  // namespace

hipError_t launch_code_pack_frames(const int64_t* codes, int B, int Tf, int n_q, int bits, const int32_t* frames_rows, const int32_t* n_q_frames,
                                   uint8_t* packets, size_t pitch, int32_t* scan, hipStream_t st) {
    if (!codes || !packets || !n_q_frames || !scan || !frames_args_ok(B, Tf, n_q, bits, packets, pitch, frame_packet_pitch(Tf, n_q, bits)))
        return hipErrorInvalidValue;
    const unsigned row_words = (unsigned)(pitch / 4);
    const size_t blocks = ((size_t)row_words - 2 + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    uint32_t* out = reinterpret_cast<uint32_t*>(packets);
    hipLaunchKernelGGL(frame_pack_scan_kernel, dim3(B), dim3(256), 0, st, Tf, n_q, bits, frames_rows, n_q_frames, scan, out, row_words);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(frame_pack_words_kernel, dim3((unsigned)blocks, B), dim3(256), 0, st, codes, B, Tf, bits, scan, out, row_words);
    return hipGetLastError();
}

// One workgroup per row: the header is read and clamped, every frame's count is read from the counts section (mode 1) or is the header's
// k (any other mode), clamped, and written to n_q_frames; S [Tf + 1] goes to the workspace.  Every read is inside the row's pitch.
__global__ __launch_bounds__(256) void frame_unpack_scan_kernel(const uint32_t* __restrict__ in, unsigned row_words, int Tf, int n_q,
                                                                int32_t* __restrict__ n_q_frames, int32_t* __restrict__ scan) {
    __shared__ int sh[256], shm[256];
    const int b = blockIdx.x;
    const uint32_t* row = in + (size_t)b * row_words;
    const uint32_t f = row[0], h = row[1];
    const int frames = f > (uint32_t)Tf ? Tf : (int)f;
    const int kb = fclampi((int)(h & 0xffu), 1, n_q);
    const bool per_frame = ((h >> 16) & 0xffu) == 1u;
    const int cbits = count_bits_dev(kb);
    int32_t* kf = n_q_frames + (size_t)b * Tf;
    int total, kmax;
    row_scan(Tf, sh, shm, scan + (size_t)b * (Tf + 1),
             [&](int t) {
                 if (t >= frames) return 0;
                 if (!per_frame) return kb;
                 const unsigned long long P = (unsigned long long)t * cbits;
                 const size_t w = 2 + (size_t)(P >> 5);
                 const int off = (int)(P & 31);
                 uint32_t x = w < row_words ? row[w] >> off : 0u;
                 if (off + cbits > 32 && w + 1 < row_words) x |= row[w + 1] << (32 - off);
                 const int k = (int)(x & ((1u << cbits) - 1u));
                 return k > kb ? kb : k;
             },
             [&](int t, int k) { kf[t] = k; }, total, kmax);
}

// One thread per token (b, t, i): inside the frame's count it reads the one or two words that hold value S_t + i of the codes section
// (mode 1: behind the counts section; else: behind the header); a word behind the row's pitch reads as 0.  Any other token is 0.
__global__ __launch_bounds__(256) void frame_unpack_tokens_kernel(const uint32_t* __restrict__ in, unsigned row_words, size_t total, int Tf, int n_q,
                                                                  int bits, const int32_t* __restrict__ n_q_frames, const int32_t* __restrict__ scan,
                                                                  int64_t* __restrict__ tokens) {
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= total) return;
    const int i = (int)(n % n_q);
    const size_t bt = n / n_q;
    const int t = (int)(bt % Tf);
    const size_t b = bt / Tf;
    int64_t v = 0;
    if (i < n_q_frames[bt]) {
        const uint32_t* row = in + b * row_words;
        const uint32_t f = row[0], h = row[1];
        size_t base = 2;
        if (((h >> 16) & 0xffu) == 1u)       // the counts section is as long as the header's own frames say: a prefix of the frames decodes
            base += (size_t)(((unsigned long long)f * count_bits_dev(fclampi((int)(h & 0xffu), 1, n_q)) + 31) / 32);
        const unsigned long long P = ((unsigned long long)scan[b * (Tf + 1) + t] + i) * bits;
        const size_t w = base + (size_t)(P >> 5);
        const int off = (int)(P & 31);
        if (w < row_words && (off + bits <= 32 || w + 1 < row_words)) {
            uint32_t x = row[w] >> off;
            if (off + bits > 32) x |= row[w + 1] << (32 - off);
            v = (int64_t)(x & ((1u << bits) - 1u));
        }
    }
    tokens[n] = v;
}

hipError_t launch_code_unpack_frames(const uint8_t* packets, size_t pitch, int B, int Tf, int n_q, int bits, int64_t* tokens, int32_t* n_q_frames,
                                     int32_t* scan, hipStream_t st) {
    if (!packets || !tokens || !n_q_frames || !scan || !frames_args_ok(B, Tf, n_q, bits, packets, pitch, code_packet_pitch(Tf, n_q, bits)))
        return hipErrorInvalidValue;
    const size_t total = (size_t)B * Tf * n_q;
    const size_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(packets);
    hipLaunchKernelGGL(frame_unpack_scan_kernel, dim3(B), dim3(256), 0, st, in, (unsigned)(pitch / 4), Tf, n_q, n_q_frames, scan);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(frame_unpack_tokens_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in, (unsigned)(pitch / 4), total, Tf, n_q, bits, n_q_frames,
                       scan, tokens);
    return hipGetLastError();
}

}  // namespace fc

// ---- the C ABI of mode 1 (include/funcodec_amd.h): engine-free --------------------------------------------------------------------
namespace {
int fail(const std::string& msg) { fc_set_last_error_(msg.c_str()); return 1; }

// what both calls refuse before any launch, naming the argument
int frame_pack_check(const char* fn, const void* a, const char* a_name, const void* b, const char* b_name, const void* c, const char* c_name, int B,
                     int Tf, int n_q, int bits, const void* packets, size_t pitch, size_t need, const char* need_name, const void* ws, size_t ws_bytes) {
    const std::string f = std::string(fn) + ": ";
    if (bits < 1 || bits > 16) return fail(f + "bits lies in 1..16, got " + std::to_string(bits));
    if (n_q < 1 || n_q > 255) return fail(f + "n_q lies in 1..255 (the header's count is one byte), got " + std::to_string(n_q));
    if (B < 1 || B > 65535) return fail(f + "B lies in 1..65535, got " + std::to_string(B));
    if (Tf < 1) return fail(f + "Tf is at least 1, got " + std::to_string(Tf));
    if ((long long)Tf * n_q > 0x7fffffffLL)
        return fail(f + "Tf * n_q = " + std::to_string((long long)Tf * n_q) + " does not fit the int32 scan of the counts");
    if (pitch < need || pitch % 4 != 0 || pitch / 4 > 0xffffffffull)
        return fail(f + "pitch must be a multiple of 4 and at least " + need_name + " = " + std::to_string(need) + ", got " + std::to_string(pitch));
    if (!a) return fail(f + a_name + " is null");
    if (!b) return fail(f + b_name + " is null");
    if (!c) return fail(f + c_name + " is null");
    if (((uintptr_t)packets & 3) != 0) return fail(f + "packets must be 4-byte aligned");
    const size_t ws_need = fc::frame_pack_workspace_bytes(B, Tf);
    if (!ws || ws_bytes < ws_need || ((uintptr_t)ws & 3) != 0)
        return fail(f + "workspace must be 4-byte aligned and hold fc_frame_pack_workspace_bytes = " + std::to_string(ws_need) + " bytes, got " +
                    std::to_string(ws ? ws_bytes : 0));
    return 0;
}

int launched(const char* fn, hipError_t e) { return e == hipSuccess ? 0 : fail(std::string(fn) + ": " + hipGetErrorString(e)); }
}  // namespace

extern "C" {

size_t fc_frame_packet_pitch(int frames, int n_q, int bits) { return fc::frame_packet_pitch(frames, n_q, bits); }

size_t fc_frame_packet_bytes(int frames, int kmax, long long n_codes, int bits) { return fc::frame_packet_bytes(frames, kmax, n_codes, bits); }

size_t fc_frame_pack_workspace_bytes(int B, int Tf) { return fc::frame_pack_workspace_bytes(B, Tf); }

int fc_codes_pack_frames(const int64_t* codes, int B, int Tf, int n_q, int bits, const int32_t* frames_rows, const int32_t* n_q_frames,
                         uint8_t* packets, size_t pitch, void* workspace, size_t workspace_bytes, void* stream) {
    if (frame_pack_check("fc_codes_pack_frames", codes, "codes", packets, "packets", n_q_frames, "n_q_frames", B, Tf, n_q, bits, packets, pitch,
                         fc::frame_packet_pitch(Tf, n_q, bits), "fc_frame_packet_pitch", workspace, workspace_bytes))
        return 1;
    return launched("fc_codes_pack_frames", fc::launch_code_pack_frames(codes, B, Tf, n_q, bits, frames_rows, n_q_frames, packets, pitch,
                                                                        (int32_t*)workspace, (hipStream_t)stream));
}

int fc_codes_unpack_frames(const uint8_t* packets, size_t pitch, int B, int Tf, int n_q, int bits, int64_t* tokens, int32_t* n_q_frames,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (frame_pack_check("fc_codes_unpack_frames", packets, "packets", tokens, "tokens", n_q_frames, "n_q_frames", B, Tf, n_q, bits, packets, pitch,
                         fc::code_packet_pitch(Tf, n_q, bits), "fc_code_packet_pitch", workspace, workspace_bytes))
        return 1;
    return launched("fc_codes_unpack_frames", fc::launch_code_unpack_frames(packets, pitch, B, Tf, n_q, bits, tokens, n_q_frames, (int32_t*)workspace,
                                                                            (hipStream_t)stream));
}

}  // extern "C"
