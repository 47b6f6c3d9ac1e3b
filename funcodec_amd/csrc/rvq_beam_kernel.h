// The beam search kernel of the residual vector quantiser (specification: rvq_beam_kernels.h) as a template, and the two macros that say
// where an instantiation lives.  rvq_beam_kernels.hip (the dispatch) sees FC_BEAM_ELSEWHERE only; one rvq_beam_w*.hip per group of shapes
// holds FC_BEAM_HERE, so that the 18 instantiations compile in parallel units (docs/history/translation_units.md has their times).
//
// One workgroup of 8 waves takes F = 16 / W frames; MFMA row f W + s is hypothesis s of frame f, so one 16 x 16 x 4 tile scores all live
// hypotheses of the workgroup against 16 codes, with the greedy kernel's operand layout (rvq_kernels.hip): A = 2 r (lane r16 = row,
// g = k), B = the codebook fragment (cb_frag order, or the plain rows), output acc[r] = row 4 g + r, code 16 t + r16.
//
// A stage:
//   1. |r|^2 of the 16 rows (rvq_row_norm) -- also the fixed-order error of a frame whose last stage has just been run;
//   2. the codebook's 16-code tiles go round the 8 waves; a lane keeps, per row, its W best (score, code) sorted in registers;
//   3. per wave and row, W rounds of a 16-lane butterfly take the lists' heads in order: the wave's W best of the row, into LDS;
//   4. wave f merges frame f's 8 waves x W parents x W entries by (score, parent, code), the greedy candidate taken out first: slots
//      1 .. W-1; slot 0 = (parent 0, g[i]).  The (parent, code) pairs are the stage's back-pointers;
//   5. residual rows of the next stage = parent's row - E_i[code], into the other LDS buffer (a child's parent may sit in any slot).
// Then the pick (lowest error, lowest slot on a tie) and the walk back along the back-pointers.
//
// A row's W best hold everything step 4 can keep: it keeps W - 1 candidates of the frame after taking out one of parent 0.
#pragma once
#include "device_common.h"

#include <cmath>
#include <cstdint>

namespace fc {

constexpr int kNone = 0x7fffffff;        // the code / key of an empty list entry (its score is +inf)

// (v, k) before (bv, bk)?  Scores ascending, then keys ascending; no NaN reaches here (a NaN score is never inserted into a list)
__device__ __forceinline__ bool beam_before(float v, int k, float bv, int bk) { return v < bv || (v == bv && k < bk); }

template <int D, int W>
__global__ __launch_bounds__(512) void rvq_beam_kernel(const float* __restrict__ x, int N, int K, int nq, const float* __restrict__ cb,
                                                       const float* __restrict__ cbf, const float* __restrict__ enorm, int64_t* codes,
                                                       int64_t* __restrict__ paths, float* __restrict__ errors, int Tf,
                                                       const int* __restrict__ nq_rows) {
    constexpr int F = 16 / W;                       // frames of the workgroup
    constexpr int NQ4 = D / 16;                     // 16-dim groups of a row: 4 MFMAs each
    constexpr int CH = NQ4 < 8 ? NQ4 : 8;           // groups per chunk: wider rows are fed in chunks of 128 dims (registers)
    constexpr int NCH = NQ4 / CH;
    constexpr int LD = D + 4;                       // row stride: the |r|^2 chains of 4 lanes per row then spread over the banks
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Rb = smem;                               // [2][16][LD] residual rows, double-buffered
    int* bp = (int*)(smem + 2 * 16 * LD);           // [nq][16] back-pointers: parent slot | code << 3
    __shared__ float xn[16];
    __shared__ float wlv[8][16][W];                 // per wave and row: the W best scores ...
    __shared__ int wlc[8][16][W];                   // ... and their codes
    __shared__ int child[16];
    __shared__ int kf[16];                          // stages of the row's frame (0 behind frame N)
    __shared__ float err[16];
    __shared__ int win[F];
    __shared__ int silent[F];                       // the frame is all zeros: it keeps its greedy codes

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, r16 = lane & 15;
    const int frame0 = blockIdx.x * F;

    auto stages_of = [&](int n) { return nq_rows ? (nq_rows[n / Tf] < nq ? nq_rows[n / Tf] : nq) : nq; };
    int nqw = 0;                                    // stages this workgroup runs: the same in every thread
#pragma unroll
    for (int f = 0; f < F; ++f)
        if (frame0 + f < N) { const int k = stages_of(frame0 + f); nqw = k > nqw ? k : nqw; }
    if (tid < 16) { const int n = frame0 + tid / W; kf[tid] = n < N ? stages_of(n) : 0; }
    for (int e = tid; e < 16 * D; e += 512) {
        const int r = e / D, d = e - r * D;
        const int n = frame0 + r / W;
        Rb[r * LD + d] = (r % W == 0 && n < N) ? x[(size_t)n * D + d] : 0.f;       // slot 0 holds the frame; the others wake at stage 1
    }
    const int ntile = K >> 4;
    int cur = 0;
    for (int i = 0;; ++i) {
        float* Rc = Rb + cur * 16 * LD;
        float* Rn = Rb + (cur ^ 1) * 16 * LD;
        __syncthreads();
        if (tid < 64) rvq_row_norm<D>(Rc + (tid >> 2) * LD, tid & 3, &xn[tid >> 2]);
        __syncthreads();
        if (i == 0 && tid < F) silent[tid] = xn[tid * W] == 0.f;
        if (tid < 16 && kf[tid] == i) err[tid] = xn[tid];      // the frame's last stage is behind it: sum_d r[d]^2, fixed order
        if (i == nqw) break;

        // ---- 2. scores, a lane's W best per row
        float lv[4][W];
        int lc[4][W];
        float xr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int s = 0; s < W; ++s) { lv[r][s] = INFINITY; lc[r][s] = kNone; }
            const int row = 4 * g + r;
            xr[r] = (i > 0 || row % W == 0) ? xn[row] : INFINITY;      // stage 0: one hypothesis per frame
        }
        f32x4 a4[CH];
        if constexpr (NCH == 1) {
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const f32x4 v = *(const f32x4*)&Rc[r16 * LD + 16 * q + 4 * g];
                a4[q] = v + v;   // 2 r, exact
            }
        }
        const int qstep = cbf ? 256 : 16;
        for (int t = wid; t < ntile; t += 8) {
            const int code = 16 * t + r16;
            const float en = enorm[(size_t)i * K + code];
            const float* e0 = cbf ? cbf + ((size_t)i * K + 16 * t) * D + lane * 4 : cb + ((size_t)i * K + code) * D + 4 * g;
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                f32x4 bq[CH];
#pragma unroll
                for (int q = 0; q < CH; ++q) bq[q] = *(const f32x4*)(e0 + qstep * (c * CH + q));
                if constexpr (NCH > 1) {
#pragma unroll
                    for (int q = 0; q < CH; ++q) {
                        const f32x4 v = *(const f32x4*)&Rc[r16 * LD + 16 * (c * CH + q) + 4 * g];
                        a4[q] = v + v;
                    }
                }
#pragma unroll
                for (int q = 0; q < CH; ++q)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q][j], bq[q][j], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float cv = __fadd_rn(__fsub_rn(xr[r], acc[r]), en);
                if (cv < lv[r][W - 1]) {       // sorted insert; a lane's codes come in ascending order, so equal scores keep the lower code first
                    int cc = code;
#pragma unroll
                    for (int s = 0; s < W; ++s)
                        if (cv < lv[r][s]) {
                            const float tv = lv[r][s]; const int tc = lc[r][s];
                            lv[r][s] = cv; lc[r][s] = cc;
                            cv = tv; cc = tc;
                        }
                }
            }
        }
        // ---- 3. the wave's W best of every row: W rounds over the heads of the 16 lanes' lists
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int s = 0; s < W; ++s) {
                float bv = lv[r][0];
                int bc = lc[r][0];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const float ov = __shfl_xor(bv, o, 64);
                    const int oc = __shfl_xor(bc, o, 64);
                    if (beam_before(ov, oc, bv, bc)) { bv = ov; bc = oc; }
                }
                if (bc != kNone && lc[r][0] == bc) {      // the lane whose head was taken moves its list up
#pragma unroll
                    for (int u = 0; u + 1 < W; ++u) { lv[r][u] = lv[r][u + 1]; lc[r][u] = lc[r][u + 1]; }
                    lv[r][W - 1] = INFINITY; lc[r][W - 1] = kNone;
                }
                if (r16 == 0) { wlv[wid][4 * g + r][s] = bv; wlc[wid][4 * g + r][s] = bc; }
            }
        }
        __syncthreads();
        // ---- 4. wave f merges frame f: keys (parent << 24 | code), so (score, key) orders by (score, parent, code)
        if (wid < F) {
            const int f = wid, n = frame0 + f;
            int gi = 0;
            if (n < N && i < kf[f * W]) {
                const long long c = codes[(size_t)i * N + n];
                gi = (c < 0 || c >= K) ? 0 : (int)c;
            }
            constexpr int NC = 8 * W * W, PER = (NC + 63) / 64;
            float cv[PER];
            int ck[PER];
#pragma unroll
            for (int m = 0; m < PER; ++m) {
                const int c = lane + 64 * m;
                cv[m] = INFINITY; ck[m] = kNone;
                if (c < NC) {
                    const int p = c / (8 * W), w = (c / W) & 7, e = c % W;
                    const int code = wlc[w][f * W + p][e];
                    if (code != kNone && !(p == 0 && code == gi)) { cv[m] = wlv[w][f * W + p][e]; ck[m] = (p << 24) | code; }
                }
            }
            for (int s = 1; s < W; ++s) {
                float bv = cv[0];
                int bk = ck[0];
#pragma unroll
                for (int m = 1; m < PER; ++m)
                    if (beam_before(cv[m], ck[m], bv, bk)) { bv = cv[m]; bk = ck[m]; }
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const float ov = __shfl_xor(bv, o, 64);
                    const int ok = __shfl_xor(bk, o, 64);
                    if (beam_before(ov, ok, bv, bk)) { bv = ov; bk = ok; }
                }
#pragma unroll
                for (int m = 0; m < PER; ++m)
                    if (bk != kNone && ck[m] == bk) { cv[m] = INFINITY; ck[m] = kNone; }
                // nothing left (a frame of NaN or inf): the slot repeats (parent 0, code 0), which is in range
                if (lane == 0) child[f * W + s] = bk == kNone ? 0 : ((bk >> 24) | ((bk & 0xffffff) << 3));
            }
            if (lane == 0) child[f * W] = gi << 3;
        }
        __syncthreads();
        // ---- 5. back-pointers and the next stage's residual rows
        if (tid < 16) bp[i * 16 + tid] = child[tid];
        for (int e = tid; e < 16 * D; e += 512) {
            const int r = e / D, d = e - r * D;
            const int ch = child[r];
            const int prow = (r / W) * W + (ch & 7);
            Rn[r * LD + d] = __fsub_rn(Rc[prow * LD + d], cb[((size_t)i * K + (ch >> 3)) * D + d]);
        }
        cur ^= 1;
    }
    __syncthreads();
    if (tid < F) {       // the pick: lowest error, the lowest slot on a tie (a NaN error never wins against slot 0)
        int best = 0;
        float bv = err[tid * W];
        for (int s = 1; s < W; ++s)
            if (err[tid * W + s] < bv) { bv = err[tid * W + s]; best = s; }
        win[tid] = silent[tid] ? 0 : best;
    }
    __syncthreads();
    if (tid < 16) {
        const int f = tid / W, s = tid % W, n = frame0 + f;
        if (n < N) {
            const int k = kf[tid];
            const bool chosen = win[f] == s;
            int at = s;
            for (int i = k - 1; i >= 0; --i) {
                const int v = bp[i * 16 + f * W + at];
                if (paths) paths[((size_t)s * nq + i) * N + n] = v >> 3;
                if (chosen) codes[(size_t)i * N + n] = v >> 3;
                at = v & 7;
            }
            if (paths)
                for (int i = k; i < nq; ++i) paths[((size_t)s * nq + i) * N + n] = 0;
            if (errors) errors[(size_t)s * N + n] = err[tid];
        }
    }
}

// where the instantiation for (D, W) is: an explicit instantiation definition in one rvq_beam_w*.hip, a declaration for everyone else
#define FC_BEAM_ARGS const float*, int, int, int, const float*, const float*, const float*, int64_t*, int64_t*, float*, int, const int*
#define FC_BEAM_ELSEWHERE(D, W) extern template __global__ void rvq_beam_kernel<D, W>(FC_BEAM_ARGS);
#define FC_BEAM_HERE(D, W) template __global__ void rvq_beam_kernel<D, W>(FC_BEAM_ARGS);

}  // namespace fc
