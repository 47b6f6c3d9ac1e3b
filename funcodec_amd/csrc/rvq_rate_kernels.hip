// gfx950 (MI355X / CDNA4) kernels of the quantiser's rate control: the residual energy of every frame after every stage, made from the
// codes of a call, the fp64 sums per batch row with the pick of a stage count per row, the pick per frame, and the zeros behind a count.
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
}  // namespace

// 16 frames per workgroup, 256 threads.  The residual rows live in LDS (padded by 4 floats like rvq_encode_kernel's: the four chains of
// a row then start in different banks); the selected code rows come through L2.  Stage i: wave 0 takes |r_i|^2 of the 16 rows (four
// lanes a row, rate_row_norm) and its 16 lanes j = 0 store 16 consecutive floats of err[i]; then all threads subtract the rows' codes of
// stage i.  krow: the row's cap, -1 for a row that is not measured (behind N, or behind its batch row's frames).
template <int D>
__global__ __launch_bounds__(256) void rvq_stage_errors_kernel(const float* __restrict__ x, const int64_t* __restrict__ codes, int N, int K, int nq,
                                                               const float* __restrict__ cb, float* __restrict__ err, int Tf,
                                                               const int* __restrict__ nq_rows, RagLen rows) {
    constexpr int ROWS = kRateRows, NEL = ROWS * D / 256;
    static_assert(ROWS * D % 256 == 0, "every thread owns NEL elements of the row set");
    __shared__ __attribute__((aligned(16))) float R[ROWS][D + 4];
    __shared__ int krow[ROWS];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * ROWS;
    if (tid < ROWS) {
        const int n = row0 + tid;
        int k = -1;
        if (n < N) {
            const int b = n / Tf, t = n - b * Tf;
            if (t < row_frames(rows, b, Tf)) k = nq_rows ? (nq_rows[b] < nq ? nq_rows[b] : nq) : nq;
        }
        krow[tid] = k;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NEL; ++it) {
        const int e = tid + 256 * it, r = e / D, d = e - r * D;
        R[r][d] = krow[r] >= 0 ? x[(size_t)(row0 + r) * D + d] : 0.f;       // a row that is not measured is never read
    }
    for (int i = 0; i <= nq; ++i) {
        __syncthreads();
        if (tid < 4 * ROWS) {           // wave 0, all 64 lanes: rate_row_norm exchanges between the four lanes of a row
            const int r = tid >> 2, n = row0 + r;
            const float e2 = rate_row_norm<D>(R[r], tid & 3);
            if ((tid & 3) == 0 && n < N) err[(size_t)i * N + n] = i <= krow[r] ? e2 : 0.f;
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
                                                            int32_t* __restrict__ n_q_out, double* __restrict__ row_err) {
    __shared__ double red[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const size_t N = (size_t)gridDim.x * Tf;
    const int frames = row_frames(rows, b, Tf);
    const int cap = nq_rows ? (nq_rows[b] < nq ? nq_rows[b] : nq) : nq;
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
    const int lo = min_nq < cap ? (min_nq < 1 ? 1 : min_nq) : cap;
    int k = cap;
    bool finite = true;
    for (int i = 0; i <= cap; ++i) finite = finite && isfinite(E[i]);
    if (finite) {
        if (E[0] == 0.0) k = lo;
        else {
            const double thr = E[0] * ratio[b];
            k = rate_pick_scan(lo, cap, [&](int i) { return E[i]; }, [&](double ei) { return ei <= thr; });
        }
    }
    if (k_table) k_table[b] = k;
    if (n_q_out) n_q_out[b] = k;
}

hipError_t launch_rvq_rate_rows(const float* err, int B, int Tf, int nq, const int* nq_rows, const RagLen& rows, const double* ratio, int min_nq,
                                int* k_table, int32_t* n_q_out, double* row_err, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (Tf <= 0 || nq < 1 || !err || !ratio || !row_err) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rvq_rate_rows_kernel, dim3(B), dim3(256), 0, st, err, Tf, nq, nq_rows, rows, ratio, min_nq, k_table, n_q_out, row_err);
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
