// gfx950 (MI355X / CDNA4) kernels of the quantiser's rate control per frame: the pick of a stage count for every frame from the stage
// errors and row sums rvq_rate_kernels.hip made, and the per-frame forms of the code sum, the zeros behind a count and the decode.
// rvq_frame_rate_kernels.h states the rule.  fp32 / fp64 and integers, 64-lane wavefronts.  The encode kernels are not involved.
#include "rvq_frame_rate_kernels.h"

namespace fc {

namespace {
__device__ __forceinline__ int frame_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// frames of batch row b: all Tf, or the row's own in a length-aware call
__device__ __forceinline__ int frame_rate_frames(const RagLen& rows, int b, int Tf) {
    if (!rows.lens) return Tf;
    const int f = ragged_cols(rows.lens[b], rows.div, rows.mul, rows.add);
    return f < Tf ? f : Tf;
}
}  // namespace

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
    const int frames = frame_rate_frames(rows, b, Tf);
    const int cap = nq_rows ? frame_clampi(nq_rows[b], 0, nq) : nq;
    const int lo = frame_clampi(min_nq, 0, cap);
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
            else {
                int best = lo, hit = -1;
                float ebest = e[(size_t)lo * N];
                for (int i = lo; i <= cap; ++i) {
                    const float ei = e[(size_t)i * N];
                    if ((double)ei * F <= thr) { hit = i; break; }
                    if (ei < ebest) { ebest = ei; best = i; }
                }
                k = hit >= 0 ? hit : best;
            }
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

// rvq_codes_sum_kernel (rvq_kernels.hip) with the count of frame row n: one workgroup per frame, the sum in stage order from 0
__global__ __launch_bounds__(256) void rvq_frame_codes_sum_kernel(const int64_t* __restrict__ codes, int N, int Tf, int nq, int D, int K,
                                                                  const float* __restrict__ cb, float* __restrict__ quant,
                                                                  float* __restrict__ quant_bdt, float* __restrict__ subq,
                                                                  const int32_t* __restrict__ k_frames) {
    const int n = blockIdx.x;
    const int b = n / Tf, t = n - b * Tf, Bn = N / Tf;
    const int k = frame_clampi(k_frames[n], 0, nq);
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float s = 0.f;
        for (int i = 0; i < nq; ++i) {
            float v = 0.f;
            if (i < k) {
                long long idx = codes[(size_t)i * N + n];
                if (idx < 0 || idx >= K) idx = 0;            // the encode kernels write codes in range; never read out of bounds
                v = cb[((size_t)i * K + idx) * D + d];
                s = s + v;
            }
            if (subq) subq[(((size_t)i * Bn + b) * D + d) * Tf + t] = v;
        }
        if (quant) quant[(size_t)n * D + d] = s;
        if (quant_bdt) quant_bdt[((size_t)b * D + d) * Tf + t] = s;
    }
}

hipError_t launch_rvq_frame_codes_sum(const int64_t* codes, int N, int D, int K, int nq, const float* cb, float* quant, float* quant_bdt, float* subq,
                                      int Tf, const int32_t* k_frames, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    if (Tf <= 0 || N % Tf != 0 || nq < 1 || !k_frames) return hipErrorInvalidValue;
    const int threads = D >= 256 ? 256 : (D >= 128 ? 128 : 64);
    hipLaunchKernelGGL(rvq_frame_codes_sum_kernel, dim3(N), dim3(threads), 0, st, codes, N, Tf, nq, D, K, cb, quant, quant_bdt, subq, k_frames);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void rvq_frame_zero_codes_kernel(int64_t* __restrict__ codes, int N, const int32_t* __restrict__ k_frames) {
    const int n = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (n < N && i >= k_frames[n]) codes[(size_t)i * N + n] = 0;
}

hipError_t launch_rvq_frame_zero_codes(int64_t* codes, int N, int nq, const int32_t* k_frames, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    if (nq < 1 || nq > 65535 || !k_frames) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rvq_frame_zero_codes_kernel, dim3((N + 255) / 256, nq), dim3(256), 0, st, codes, N, k_frames);
    return hipGetLastError();
}

// rvq_decode_kernel (rvq_kernels.hip) with the count of frame row n: out = ((0 + E_0[i0]) + E_1[i1]) + ... over the frame's first k codes
__global__ __launch_bounds__(256) void rvq_frame_decode_kernel(const int64_t* __restrict__ codes, int Tf, int nq, int D, int K,
                                                               const float* __restrict__ cb, float* __restrict__ emb, float* __restrict__ emb_bdt,
                                                               unsigned* __restrict__ status, const int32_t* __restrict__ k_frames, RagLen rows) {
    const int n = blockIdx.x;   // row = b*Tf + t
    const int b = n / Tf, t = n - b * Tf;
    const int k = t < frame_rate_frames(rows, b, Tf) ? frame_clampi(k_frames[n], 0, nq) : 0;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float s = 0.f;
        for (int i = 0; i < k; ++i) {
            long long idx = codes[(size_t)n * nq + i];
            if (idx < 0 || idx >= K) {      // as rvq_decode_kernel: never read out of bounds, and make the corrupt token loud
                if (status && threadIdx.x == 0) *(volatile unsigned*)(status + FC_STATUS_BAD_CODE) = 1u;
                idx = idx < 0 ? 0 : K - 1;
            }
            s = s + cb[((size_t)i * K + idx) * D + d];
        }
        if (emb) emb[(size_t)n * D + d] = s;
        if (emb_bdt) emb_bdt[((size_t)b * D + d) * Tf + t] = s;
    }
}

hipError_t launch_rvq_frame_decode(const int64_t* codes, int B, int Tf, int nq, int D, int K, const float* cb, float* emb, float* emb_bdt,
                                   unsigned* status, const int32_t* k_frames, const RagLen& rows, hipStream_t st) {
    if ((long long)B * Tf <= 0) return hipSuccess;
    if (!k_frames || nq < 1) return hipErrorInvalidValue;
    const int threads = D >= 256 ? 256 : (D >= 128 ? 128 : 64);
    hipLaunchKernelGGL(rvq_frame_decode_kernel, dim3(B * Tf), dim3(threads), 0, st, codes, Tf, nq, D, K, cb, emb, emb_bdt, status, k_frames, rows);
    return hipGetLastError();
}

}  // namespace fc
