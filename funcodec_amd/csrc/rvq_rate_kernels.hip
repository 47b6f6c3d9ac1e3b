// gfx950 (MI355X / CDNA4) kernels of the quantiser's rate control: the residual energy of every frame after every stage, made from the
// codes of a call, the fp64 sums per batch row with the pick of a stage count per row, the pick per frame, and the zeros behind a count;
// and the push rule of a session in one launch (rvq_push_floor_kernel: the same steps, fused per batch row).
// rvq_rate_kernels.h states the rules.  fp32 / fp64 and integers, 64-lane wavefronts.  The encode kernels (rvq_kernels.hip,
// rvq_beam_kernel.h) are not involved: the errors are recomputed from x and the codes, so whoever found the codes is measured by the
// same formula.
#include "device_common.h"
#include "rvq_rate_kernels.h"

namespace fc {

namespace {
constexpr int kRateRows = 16;        // frames per workgroup of rvq_stage_errors_kernel

// The scan of both picks (rvq_rate_kernels.h): the smallest k in [lo, cap] with meets(err(k)), else the k in that range with the smallest
// err(k), first on ties.  The row rule scans fp64 row sums, the frame rule one frame's fp32 errors.
template <typename Err, typename Meets>
__device__ __forceinline__ int rate_pick_scan(int lo, int cap, Err&& err, Meets&& meets) {
    int best = lo;
    auto ebest = err(lo);
    for (int i = lo; i <= cap; ++i) {
        const auto ei = err(i);
        if (meets(ei)) return i;
        if (ei < ebest) { ebest = ei; best = i; }
    }
    return best;
}

// |r|^2 of one residual row by four lanes j = 0 .. 3 (consecutive lanes) in the order rvq_row_norm (device_common.h) states: chain j over
// d in [j D/4, (j + 1) D/4) with the square ROUNDED SEPARATELY, the chains combined (p0 + p1) + (p2 + p3); every lane returns its pair's
// view, lane j = 0 the result.  Stated again here with contraction off: as the encode kernels compile it, rvq_row_norm's square and add
// become one fused multiply-add (hipcc contracts across its __fmul_rn / __fadd_rn, which are plain operators), and those kernels are
// not to be touched.  The errors of this unit are therefore the float32 arithmetic a host can restate operation by operation.
template <int D>
__device__ __forceinline__ float rate_row_norm(const float* row, int j) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll 8
    for (int d = j * (D / 4); d < (j + 1) * (D / 4); ++d) {
        const float v = row[d];
        const float sq = v * v;
        s = s + sq;
    }
    const float s_pair = s + __shfl_xor(s, 1, 64);          // p0+p1 | p2+p3
    return s_pair + __shfl_xor(s_pair, 2, 64);              // (p0+p1)+(p2+p3)
}

// The stage errors of 16 consecutive frame rows from row0, by the 256 threads of a workgroup: the one statement of the first bullet of
// the row rule, shared by rvq_stage_errors_kernel and the fused push kernel.  The residual rows live in LDS (padded by 4 floats like
// rvq_encode_kernel's: the four chains of a row then start in different banks); the selected code rows come through L2.  Stage i:
// wave 0 takes |r_i|^2 of the 16 rows (four lanes a row, rate_row_norm) and its 16 lanes j = 0 hand it to store(i, n, value); then all
// threads subtract the rows' codes of stage i.  cap_of(n): the row's cap, -1 for a row that is not measured (nothing of it is read).
// Every thread of the workgroup calls it (it holds barriers); the caller puts a barrier between two tiles.
template <int D, typename Cap, typename Store>
__device__ __forceinline__ void rvq_stage_errors_tile(float (*R)[D + 4], int* krow, const float* __restrict__ x, const int64_t* __restrict__ codes,
                                                      int N, int K, int nq, const float* __restrict__ cb, int row0, Cap&& cap_of, Store&& store) {
    constexpr int ROWS = kRateRows, NEL = ROWS * D / 256;
    static_assert(ROWS * D % 256 == 0, "every thread owns NEL elements of the row set");
    const int tid = threadIdx.x;
    if (tid < ROWS) krow[tid] = cap_of(row0 + tid);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NEL; ++it) {
        const int e = tid + 256 * it, r = e / D, d = e - r * D;
        R[r][d] = krow[r] >= 0 ? x[(size_t)(row0 + r) * D + d] : 0.f;       // a row that is not measured is never read
    }
    for (int i = 0; i <= nq; ++i) {
        __syncthreads();
        if (tid < 4 * ROWS) {           // wave 0, all 64 lanes: rate_row_norm exchanges between the four lanes of a row
            const int r = tid >> 2;
            const float e2 = rate_row_norm<D>(R[r], tid & 3);
            if ((tid & 3) == 0) store(i, row0 + r, i <= krow[r] ? e2 : 0.f);
        }
        if (i == nq) break;
        __syncthreads();
        float qv[NEL];
#pragma unroll
        for (int it = 0; it < NEL; ++it) {      // all loads first (they are independent), then the LDS updates
            const int e = tid + 256 * it, r = e / D, d = e - r * D;
            qv[it] = 0.f;
            if (i < krow[r]) {
                long long idx = codes[(size_t)i * N + row0 + r];
                if (idx < 0 || idx >= K) idx = 0;                            // as rvq_codes_sum_kernel: never read out of bounds
                qv[it] = cb[((size_t)i * K + idx) * D + d];
            }
        }
#pragma unroll
        for (int it = 0; it < NEL; ++it) {
            const int e = tid + 256 * it, r = e / D, d = e - r * D;
            if (i < krow[r]) R[r][d] = __fsub_rn(R[r][d], qv[it]);
        }
    }
}

// The pick of one row from its fp64 sums E[0 .. cap] (rvq_rate_kernels.h), by one thread.  floor null: the row rule, thr = E[0] * ratio[b]
// and E[0] == 0 is silence.  floor given: the push rule, thr = floor[b] * (double)frames and E[0] <= thr is silence.
__device__ __forceinline__ int rate_pick_row(const double* E, int cap, int min_nq, const double* __restrict__ ratio,
                                             const double* __restrict__ floor, int b, int frames) {
    const int lo = min_nq < cap ? (min_nq < 1 ? 1 : min_nq) : cap;
    if (floor && floor[b] < 0.0) return cap;            // the push rule: a row switched off
    bool finite = true;
    for (int i = 0; i <= cap; ++i) finite = finite && isfinite(E[i]);
    if (!finite) return cap;
    const double thr = floor ? floor[b] * (double)frames : E[0] * ratio[b];
    if (floor ? E[0] <= thr : E[0] == 0.0) return lo;
    return rate_pick_scan(lo, cap, [&](int i) { return E[i]; }, [&](double ei) { return ei <= thr; });
}

// the cap of batch row b: its entry of the per-row table, else nq
__device__ __forceinline__ int rate_row_cap(const int* __restrict__ nq_rows, int b, int nq) {
    return nq_rows ? (nq_rows[b] < nq ? nq_rows[b] : nq) : nq;
}
}  // namespace

// 16 frames per workgroup, 256 threads: one tile of rvq_stage_errors_tile.  A row behind N, or behind its batch row's frames, is not measured.
template <int D>
__global__ __launch_bounds__(256) void rvq_stage_errors_kernel(const float* __restrict__ x, const int64_t* __restrict__ codes, int N, int K, int nq,
                                                               const float* __restrict__ cb, float* __restrict__ err, int Tf,
                                                               const int* __restrict__ nq_rows, RagLen rows) {
    __shared__ __attribute__((aligned(16))) float R[kRateRows][D + 4];
    __shared__ int krow[kRateRows];
    rvq_stage_errors_tile<D>(R, krow, x, codes, N, K, nq, cb, blockIdx.x * kRateRows,
        [&](int n) {
            if (n >= N) return -1;
            const int b = n / Tf, t = n - b * Tf;
            return t < row_frames(rows, b, Tf) ? rate_row_cap(nq_rows, b, nq) : -1;
        },
        [&](int i, int n, float v) { if (n < N) err[(size_t)i * N + n] = v; });
}

hipError_t launch_rvq_stage_errors(const float* x, const int64_t* codes, int N, int D, int K, int nq, const float* cb, float* err, int Tf,
                                   const int* nq_rows, const RagLen& rows, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    if (Tf <= 0 || N % Tf != 0 || nq < 1 || K < 1) return hipErrorInvalidValue;
    const dim3 grid((N + kRateRows - 1) / kRateRows), block(256);
#define FC_RATE_CASE(DD)                                                                                                          \
    case DD:                                                                                                                      \
        hipLaunchKernelGGL((rvq_stage_errors_kernel<DD>), grid, block, 0, st, x, codes, N, K, nq, cb, err, Tf, nq_rows, rows);      \
        break;
    switch (D) {
        FC_RATE_CASE(16)
        FC_RATE_CASE(32)
        FC_RATE_CASE(64)
        FC_RATE_CASE(128)
        FC_RATE_CASE(256)
        FC_RATE_CASE(512)
        default: return hipErrorInvalidValue;
    }
#undef FC_RATE_CASE
    return hipGetLastError();
}

// One workgroup per batch row.  E_b[i]: thread j adds the row's frames t = j, j + 256, ... in rising order in fp64, the 256 partial sums
// meet as a binary tree in LDS (no atomics): the order depends on the row's frame count alone.  Thread 0 then picks (rvq_rate_kernels.h).
__global__ __launch_bounds__(256) void rvq_rate_rows_kernel(const float* __restrict__ err, int Tf, int nq, const int* __restrict__ nq_rows,
                                                            RagLen rows, const double* __restrict__ ratio, int min_nq, int* __restrict__ k_table,
                                                            int32_t* __restrict__ n_q_out, double* __restrict__ row_err,
                                                            const double* __restrict__ floor) {
    __shared__ double red[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const size_t N = (size_t)gridDim.x * Tf;
    const int frames = row_frames(rows, b, Tf);
    if (floor && frames <= 0) return;           // the push rule: a row without a frame in the push is neither read nor written
    const int cap = rate_row_cap(nq_rows, b, nq);
    double* E = row_err + (size_t)b * (nq + 1);
    for (int i = 0; i <= nq; ++i) {
        double s = 0.0;
        if (i <= cap)
            for (int t = tid; t < frames; t += 256) s = s + (double)err[(size_t)i * N + (size_t)b * Tf + t];
        red[tid] = s;
        __syncthreads();
        for (int o = 128; o >= 1; o >>= 1) {
            if (tid < o) red[tid] = red[tid] + red[tid + o];
            __syncthreads();
        }
        if (tid == 0) E[i] = red[0];
        __syncthreads();
    }
    if (tid != 0) return;
    const int k = rate_pick_row(E, cap, min_nq, ratio, floor, b, frames);
    if (k_table) k_table[b] = k;
    if (n_q_out) n_q_out[b] = k;
}

hipError_t launch_rvq_rate_rows(const float* err, int B, int Tf, int nq, const int* nq_rows, const RagLen& rows, const double* ratio, int min_nq,
                                int* k_table, int32_t* n_q_out, double* row_err, hipStream_t st, const double* floor) {
    if (B <= 0) return hipSuccess;
    if (Tf <= 0 || nq < 1 || !err || !(ratio || floor) || !row_err) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rvq_rate_rows_kernel, dim3(B), dim3(256), 0, st, err, Tf, nq, nq_rows, rows, ratio, min_nq, k_table, n_q_out, row_err, floor);
    return hipGetLastError();
}

// THE PUSH RULE in one launch (rvq_rate_kernels.h): one workgroup per batch row, thread t owns frame t of the push (Tf <= 256).
//   1. stage errors: the row's frames in tiles of 16 through rvq_stage_errors_tile, into errf [nq + 1][Tf] in LDS (and serr_out);
//   2. E_b[i]: thread j's partial is its one term (0.0 + err, as rvq_rate_rows_kernel's loop leaves it), the 256 partials meet as that
//      kernel's binary tree, kTreeStages stages per pass;
//   3. thread 0 picks (rate_pick_row) and writes k_b;
//   4. codes[k_b:] of the row's Tf frames are zeroed and the first k_b code vectors summed in stage order from 0, element by element as
//      rvq_codes_sum_kernel does, into quant / quant_bdt / subq.
// A row without a frame in the push returns at once.  The zeroed codes lie at stages >= k_b, the summed ones below: no thread reads what
// another writes in step 4.
constexpr int kTreeStages = 4;
template <int D>
__global__ __launch_bounds__(256) void rvq_push_floor_kernel(const float* __restrict__ x, int64_t* __restrict__ codes, int Tf, int K, int nq,
                                                             const float* __restrict__ cb, const int* __restrict__ nq_rows, RagLen rows,
                                                             const double* __restrict__ floor, int min_nq, int32_t* __restrict__ n_q_out,
                                                             float* __restrict__ quant, float* __restrict__ quant_bdt, float* __restrict__ subq,
                                                             double* __restrict__ row_err, float* __restrict__ serr_out) {
    extern __shared__ float errf[];                     // [nq + 1][Tf]
    __shared__ __attribute__((aligned(16))) float R[kRateRows][D + 4];
    __shared__ int krow[kRateRows];
    __shared__ double red[kTreeStages][256];
    __shared__ double E[kPushFloorMaxStages + 1];
    __shared__ int k_row;
    const int tid = threadIdx.x, b = blockIdx.x, Bn = gridDim.x;
    const int N = Bn * Tf;
    const int frames = row_frames(rows, b, Tf);
    if (frames <= 0) return;
    const int cap = rate_row_cap(nq_rows, b, nq);
    for (int t0 = 0; t0 < Tf; t0 += kRateRows) {
        rvq_stage_errors_tile<D>(R, krow, x, codes, N, K, nq, cb, b * Tf + t0,
            [&](int n) { return n - b * Tf < frames ? cap : -1; },          // also every row of the tile behind Tf: frames <= Tf
            [&](int i, int n, float v) {
                const int t = n - b * Tf;
                if (t >= Tf) return;
                errf[i * Tf + t] = v;
                if (serr_out) serr_out[(size_t)i * N + n] = v;
            });
        __syncthreads();
    }
    for (int i0 = 0; i0 <= nq; i0 += kTreeStages) {
        const int ni = nq + 1 - i0 < kTreeStages ? nq + 1 - i0 : kTreeStages;
        for (int j = 0; j < ni; ++j) {
            double s = 0.0;
            if (i0 + j <= cap && tid < frames) s = s + (double)errf[(i0 + j) * Tf + tid];
            red[j][tid] = s;
        }
        __syncthreads();
        for (int o = 128; o >= 1; o >>= 1) {
            for (int e = tid; e < ni * o; e += 256) {
                const int j = e / o, c = e - j * o;
                red[j][c] = red[j][c] + red[j][c + o];
            }
            __syncthreads();
        }
        if (tid < ni) {
            E[i0 + tid] = red[tid][0];
            if (row_err) row_err[(size_t)b * (nq + 1) + i0 + tid] = red[tid][0];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int k = rate_pick_row(E, cap, min_nq, nullptr, floor, b, frames);
        k_row = k;
        n_q_out[b] = k;
    }
    __syncthreads();
    const int k = k_row;
    for (int e = tid; e < (nq - k) * Tf; e += 256) {
        const int i = k + e / Tf, t = e % Tf;
        codes[(size_t)i * N + (size_t)b * Tf + t] = 0;
    }
    for (int e = tid; e < Tf * D; e += 256) {
        const int t = e / D, d = e - t * D;
        const size_t n = (size_t)b * Tf + t;
        float s = 0.f;
        for (int i = 0; i < nq; ++i) {
            float v = 0.f;
            if (i < k) {
                long long idx = codes[(size_t)i * N + n];
                if (idx < 0 || idx >= K) idx = 0;
                v = cb[((size_t)i * K + idx) * D + d];
                s = s + v;
            }
            if (subq) subq[(((size_t)i * Bn + b) * D + d) * Tf + t] = v;
        }
        if (quant) quant[n * D + d] = s;
        if (quant_bdt) quant_bdt[((size_t)b * D + d) * Tf + t] = s;
    }
}

// static LDS of rvq_push_floor_kernel<D> besides errf; the launch is refused (false) where the whole does not fit 64 KiB
static size_t push_floor_static_lds(int D) {
    return sizeof(float) * kRateRows * (D + 4) + sizeof(int) * (kRateRows + 1) + sizeof(double) * (kTreeStages * 256 + kPushFloorMaxStages + 1);
}

bool rvq_push_floor_fits(int Tf, int D, int nq) {
    if (Tf < 1 || Tf > kPushFloorMaxFrames || nq < 1 || nq > kPushFloorMaxStages) return false;
    if (D != 16 && D != 32 && D != 64 && D != 128 && D != 256 && D != 512) return false;
    return push_floor_static_lds(D) + sizeof(float) * (size_t)(nq + 1) * Tf + 256 <= 64 * 1024;
}

hipError_t launch_rvq_push_floor(const float* x, int64_t* codes, int B, int Tf, int D, int K, int nq, const float* cb, const int* nq_rows,
                                 const RagLen& rows, const double* floor, int min_nq, int32_t* n_q_out, float* quant, float* quant_bdt, float* subq,
                                 double* row_err, float* serr_out, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (!rvq_push_floor_fits(Tf, D, nq) || K < 1 || !x || !codes || !floor || !n_q_out) return hipErrorInvalidValue;
    const size_t dyn = sizeof(float) * (size_t)(nq + 1) * Tf;
#define FC_FLOOR_CASE(DD)                                                                                                                   \
    case DD:                                                                                                                                \
        hipLaunchKernelGGL((rvq_push_floor_kernel<DD>), dim3(B), dim3(256), dyn, st, x, codes, Tf, K, nq, cb, nq_rows, rows, floor, min_nq,    \
                           n_q_out, quant, quant_bdt, subq, row_err, serr_out);                                                            \
        break;
    switch (D) {
        FC_FLOOR_CASE(16)
        FC_FLOOR_CASE(32)
        FC_FLOOR_CASE(64)
        FC_FLOOR_CASE(128)
        FC_FLOOR_CASE(256)
        FC_FLOOR_CASE(512)
        default: return hipErrorInvalidValue;
    }
#undef FC_FLOOR_CASE
    return hipGetLastError();
}

namespace {
// THE PUSH FRAME RULE (rvq_rate_kernels.h): the count of one frame from its fp32 errors err(0 .. cap), by one thread.  fl: the row's floor
// (-1: the row is switched off).  Comparisons only.
template <typename Err>
__device__ __forceinline__ int floor_pick_frame(int cap, int min_nq, double fl, Err&& err) {
    const int lo = min_nq < 0 ? 0 : (min_nq > cap ? cap : min_nq);
    if (fl < 0.0) return cap;
    bool finite = true;
    for (int i = 0; i <= cap; ++i) finite = finite && isfinite(err(i));
    if (!finite) return cap;
    if ((double)err(0) <= fl) return lo;
    return rate_pick_scan(lo, cap, err, [&](float ei) { return (double)ei <= fl; });
}
}  // namespace

// The pick of the chain form: one thread per frame of the push, from the stage errors launch_rvq_stage_errors wrote on the same stream.
// A frame behind its row's frames takes 0; a row without a frame in the push is not written.
__global__ __launch_bounds__(256) void rvq_floor_frames_kernel(const float* __restrict__ err, int B, int Tf, int nq, const int* __restrict__ nq_rows,
                                                               RagLen rows, const double* __restrict__ floor, int min_nq,
                                                               int32_t* __restrict__ n_q_frames) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int N = B * Tf;
    if (n >= N) return;
    const int b = n / Tf, t = n - b * Tf;
    const int frames = row_frames(rows, b, Tf);
    if (frames <= 0) return;
    int k = 0;
    if (t < frames) {
        const float* e = err + n;                       // e[i * N]: the frame's error after i stages
        k = floor_pick_frame(rate_row_cap(nq_rows, b, nq), min_nq, floor[b], [&](int i) { return e[(size_t)i * N]; });
    }
    n_q_frames[n] = k;
}

hipError_t launch_rvq_floor_frames(const float* err, int B, int Tf, int nq, const int* nq_rows, const RagLen& rows, const double* floor, int min_nq,
                                   int32_t* n_q_frames, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (Tf <= 0 || nq < 1 || !err || !floor || !n_q_frames || (long long)B * Tf > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rvq_floor_frames_kernel, dim3((unsigned)(((long long)B * Tf + 255) / 256)), dim3(256), 0, st, err, B, Tf, nq, nq_rows, rows, floor,
                       min_nq, n_q_frames);
    return hipGetLastError();
}

// THE PUSH FRAME RULE in one launch (rvq_rate_kernels.h): one workgroup per tile of 16 frames of one batch row (blockIdx.x the tile,
// blockIdx.y the row), any Tf.
//   1. stage errors of the tile through rvq_stage_errors_tile into errf [nq + 1][16] in LDS (and serr_out);
//   2. lanes 0 .. 15 pick their frame's count (floor_pick_frame) into kt[] and n_q_frames;
//   3. codes at stages >= k_t are zeroed and the first k_t code vectors summed in stage order from 0, element by element as
//      rvq_codes_sum_kernel does, into quant / quant_bdt / subq.
// A row without a frame in the push returns at once; a tile wholly behind its row's frames writes its zeros and reads nothing of x or the
// codes (every cap of the tile is -1).  The zeroed codes lie at stages >= k_t, the summed ones below, and a tile's frames are its own: no
// thread reads a code another thread of the launch writes.  No atomics, no fp64 arithmetic besides the widening of the comparisons.
template <int D>
__global__ __launch_bounds__(256) void rvq_push_floor_frames_kernel(const float* __restrict__ x, int64_t* __restrict__ codes, int Tf, int K, int nq,
                                                                    const float* __restrict__ cb, const int* __restrict__ nq_rows, RagLen rows,
                                                                    const double* __restrict__ floor, int min_nq, int32_t* __restrict__ n_q_frames,
                                                                    float* __restrict__ quant, float* __restrict__ quant_bdt,
                                                                    float* __restrict__ subq, float* __restrict__ serr_out) {
    extern __shared__ float errf[];                     // [nq + 1][16]
    __shared__ __attribute__((aligned(16))) float R[kRateRows][D + 4];
    __shared__ int krow[kRateRows];
    __shared__ int kt[kRateRows];
    const int tid = threadIdx.x, b = blockIdx.y, Bn = gridDim.y, t0 = blockIdx.x * kRateRows;
    const int N = Bn * Tf;
    const int frames = row_frames(rows, b, Tf);
    if (frames <= 0) return;
    const int cap = rate_row_cap(nq_rows, b, nq);
    const int row0 = b * Tf + t0;
    rvq_stage_errors_tile<D>(R, krow, x, codes, N, K, nq, cb, row0,
        [&](int n) { return n - b * Tf < frames ? cap : -1; },              // also every row of the tile behind Tf: frames <= Tf
        [&](int i, int n, float v) {
            const int r = n - row0;
            errf[i * kRateRows + r] = v;
            if (serr_out && t0 + r < Tf) serr_out[(size_t)i * N + n] = v;
        });
    __syncthreads();
    if (tid < kRateRows) {
        const int t = t0 + tid;
        int k = 0;
        if (t < frames) k = floor_pick_frame(cap, min_nq, floor[b], [&](int i) { return errf[i * kRateRows + tid]; });
        kt[tid] = k;
        if (t < Tf) n_q_frames[(size_t)b * Tf + t] = k;
    }
    __syncthreads();
    const int nt = Tf - t0 < kRateRows ? Tf - t0 : kRateRows;             // the tile's frames inside the push
    for (int e = tid; e < nq * nt; e += 256) {
        const int i = e / nt, r = e - i * nt;
        if (i >= kt[r]) codes[(size_t)i * N + row0 + r] = 0;
    }
    for (int e = tid; e < nt * D; e += 256) {
        const int r = e / D, d = e - r * D, t = t0 + r, k = kt[r];
        const size_t n = (size_t)row0 + r;
        float s = 0.f;
        for (int i = 0; i < nq; ++i) {
            float v = 0.f;
            if (i < k) {
                long long idx = codes[(size_t)i * N + n];
                if (idx < 0 || idx >= K) idx = 0;
                v = cb[((size_t)i * K + idx) * D + d];
                s = s + v;
            }
            if (subq) subq[(((size_t)i * Bn + b) * D + d) * Tf + t] = v;
        }
        if (quant) quant[n * D + d] = s;
        if (quant_bdt) quant_bdt[((size_t)b * D + d) * Tf + t] = s;
    }
}

hipError_t launch_rvq_push_floor_frames(const float* x, int64_t* codes, int B, int Tf, int D, int K, int nq, const float* cb, const int* nq_rows,
                                        const RagLen& rows, const double* floor, int min_nq, int32_t* n_q_frames, float* quant, float* quant_bdt,
                                        float* subq, float* serr_out, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (Tf < 1 || nq < 1 || nq > kPushFloorFramesMaxStages || B > 65535 || (long long)B * Tf > 0x7fffffffLL || K < 1 || !x || !codes || !floor ||
        !n_q_frames)
        return hipErrorInvalidValue;
    const size_t dyn = sizeof(float) * (size_t)(nq + 1) * kRateRows;
    const dim3 grid((Tf + kRateRows - 1) / kRateRows, B);
#define FC_FLOOR_CASE(DD)                                                                                                                       \
    case DD:                                                                                                                                    \
        hipLaunchKernelGGL((rvq_push_floor_frames_kernel<DD>), grid, dim3(256), dyn, st, x, codes, Tf, K, nq, cb, nq_rows, rows, floor, min_nq,     \
                           n_q_frames, quant, quant_bdt, subq, serr_out);                                                                       \
        break;
    switch (D) {
        FC_FLOOR_CASE(16)
        FC_FLOOR_CASE(32)
        FC_FLOOR_CASE(64)
        FC_FLOOR_CASE(128)
        FC_FLOOR_CASE(256)
        FC_FLOOR_CASE(512)
        default: return hipErrorInvalidValue;
    }
#undef FC_FLOOR_CASE
    return hipGetLastError();
}

// One workgroup per batch row, 256 threads; thread j owns frames t = j, j + 256, ... in rising order (the order of E_b's partial sums).
// Thread 0 classifies the row (finite / silent / threshold) into LDS; every thread then picks for its frames, keeps its fp64 partial of
// the achieved error, its count sum and its largest count; the partials meet as a binary tree in LDS (no atomics).
__global__ __launch_bounds__(256) void rvq_rate_frames_kernel(const float* __restrict__ err, const double* __restrict__ row_err, int Tf, int nq,
                                                              const int* __restrict__ nq_rows, RagLen rows, const double* __restrict__ ratio,
                                                              int min_nq, int32_t* __restrict__ n_q_frames, int32_t* __restrict__ n_q_rows_out,
                                                              int32_t* __restrict__ n_codes_out, double* __restrict__ achieved) {
    __shared__ double red[256];
    __shared__ int redk[256], redm[256];
    __shared__ int row_kind;            // 0: threshold, 1: not finite (cap), 2: silence (floor)
    __shared__ double row_thr;
    const int tid = threadIdx.x, b = blockIdx.x;
    const size_t N = (size_t)gridDim.x * Tf;
    const int frames = row_frames(rows, b, Tf);
    StageCounts caps; caps.rows = nq_rows;
    const int cap = stage_count(caps, 0, b, nq);
    const int lo = min_nq < 0 ? 0 : (min_nq > cap ? cap : min_nq);
    if (tid == 0) {
        const double* E = row_err + (size_t)b * (nq + 1);
        bool finite = true;
        for (int i = 0; i <= cap; ++i) finite = finite && isfinite(E[i]);
        row_kind = !finite ? 1 : (E[0] == 0.0 ? 2 : 0);
        row_thr = finite ? E[0] * ratio[b] : 0.0;
    }
    __syncthreads();
    const int kind = row_kind;
    const double thr = row_thr, F = (double)frames;
    double s = 0.0;
    int ksum = 0, kmax = 0;
    for (int t = tid; t < Tf; t += 256) {
        int k = 0;
        if (t < frames) {
            const float* e = err + (size_t)b * Tf + t;          // e[i * N]: the frame's error after i stages
            if (kind == 1) k = cap;
            else if (kind == 2) k = lo;
            else k = rate_pick_scan(lo, cap, [&](int i) { return e[(size_t)i * N]; }, [&](float ei) { return (double)ei * F <= thr; });
            s = s + (double)e[(size_t)k * N];
            ksum += k;
            kmax = k > kmax ? k : kmax;
        }
        n_q_frames[(size_t)b * Tf + t] = k;
    }
    red[tid] = s; redk[tid] = ksum; redm[tid] = kmax;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) {
            red[tid] = red[tid] + red[tid + o];
            redk[tid] = redk[tid] + redk[tid + o];
            redm[tid] = redm[tid] > redm[tid + o] ? redm[tid] : redm[tid + o];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    if (n_q_rows_out) n_q_rows_out[b] = redm[0];
    if (n_codes_out) n_codes_out[b] = redk[0];
    if (achieved) achieved[b] = red[0];
}

hipError_t launch_rvq_rate_frames(const float* err, const double* row_err, int B, int Tf, int nq, const int* nq_rows, const RagLen& rows,
                                  const double* ratio, int min_nq, int32_t* n_q_frames, int32_t* n_q_rows_out, int32_t* n_codes_out, double* achieved,
                                  hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (Tf <= 0 || nq < 1 || !err || !row_err || !ratio || !n_q_frames) return hipErrorInvalidValue;
    if ((long long)Tf * nq > 0x7fffffffLL) return hipErrorInvalidValue;        // n_codes_rows is an i32
    hipLaunchKernelGGL(rvq_rate_frames_kernel, dim3(B), dim3(256), 0, st, err, row_err, Tf, nq, nq_rows, rows, ratio, min_nq, n_q_frames, n_q_rows_out,
                       n_codes_out, achieved);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void rvq_rate_zero_codes_kernel(int64_t* __restrict__ codes, int N, int Tf, StageCounts k) {
    const int n = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (n < N && i >= stage_count(k, n, n / Tf, gridDim.y)) codes[(size_t)i * N + n] = 0;
}

hipError_t launch_rvq_rate_zero_codes(int64_t* codes, int N, int Tf, int nq, const StageCounts& k, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    if (Tf <= 0 || N % Tf != 0 || nq < 1 || nq > 65535 || !(k.rows || k.frames)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rvq_rate_zero_codes_kernel, dim3((N + 255) / 256, nq), dim3(256), 0, st, codes, N, Tf, k);
    return hipGetLastError();
}

}  // namespace fc
