// gfx950 (MI355X / CDNA4) kernels of the residual vector quantiser: the greedy encode (all stages fused), the decode and the sums
// that restate its order.  The search over the stages is rvq_beam_kernels.hip.  fp32 throughout, 64-lane wavefronts.
#include "device_common.h"
#include "kernels.h"
#include "rvq_rate_kernels.h"

namespace fc {

// =================================================================================================
// Residual vector quantiser: all n_q stages fused, 16 rows per workgroup
//    (DistributedResidualVectorQuantization.forward ddp_core_vq.py:367-418, eval branch;
//     EuclideanCodebook.quantize :180-188; dequantize :190-192)
//
//    stage i:  dist[row][k] = -(( |x|^2 - (2x).e_k ) + |e_k|^2)     idx = argmax_k, FIRST max wins
//              q = E_i[idx];  residual -= q;  out += q
//
//    Arithmetic order (restated bit-for-bit by oracle/c/rvq_oracle.c):
//      |x|^2   : 4 partial chains over d in [j*D/4,(j+1)*D/4), s = s + x*x with the square rounded
//                separately (torch: x.pow(2).sum(1)), combined (p0+p1)+(p2+p3);
//      (2x).e  : one MFMA accumulator per (row, code): fmaf chain from 0 over d in the order
//                d = 16q + 4g + j  for q = 0..D/16-1, j = 0..3, g = 0..3 (innermost);
//      |e|^2   : precomputed at load time (engine.hip), sequential d = 0..D-1, squares rounded separately.
// =================================================================================================
// ---- the steps rvq_encode_kernel and rvq_encode_wide_kernel share, stated once (ROWS = rows of the workgroup).  The two tails (the RQ
//      zeros behind the last stage, the quant / quant_bdt store) are the same lines in both kernels too, but stay in the kernels: as
//      functions they changed the register allocation of most RQ instantiations (ROCm 7.2 hipcc, kernel-resource-usage remarks).

// RQ: the stages this workgroup runs (the largest count among its rows) and, in krow, every row's own count (0 behind row N; read behind
// the first barrier of stage 0).  The rows of a workgroup are consecutive frames, so their batch rows are consecutive too: every thread
// takes the same maximum.  Without RQ: nq, krow untouched.
template <int ROWS, bool RQ>
__device__ __forceinline__ int rvq_stage_counts(int row0, int N, int nq, int Tf, const int* nq_rows, int* krow) {
    if constexpr (!RQ) return nq;
    else {
        const int tid = threadIdx.x;
        const int last = (row0 + ROWS <= N ? row0 + ROWS : N) - 1;
        int nqw = 0;
        for (int b = row0 / Tf; b <= last / Tf; ++b) {
            const int k = nq_rows[b] < nq ? nq_rows[b] : nq;
            nqw = k > nqw ? k : nqw;
        }
        if (tid < ROWS) {
            const int n = row0 + tid;
            krow[tid] = n < N ? (nq_rows[n / Tf] < nq ? nq_rows[n / Tf] : nq) : 0;
        }
        return nqw;
    }
}

// rvq_row_norm (|x|^2 of one residual row by four lanes): device_common.h -- the beam search (rvq_beam_kernel.h) states its errors with it

// arg-max of a stage, FIRST max wins: every wave's (best, index) registers (row 16 s2 + 4 g + r, the wave's codes spread over the 16 lanes
// r16) meet by a 16-lane butterfly, the 8 waves' results through LDS; thread `row` then clamps the index into range (all-NaN row: torch
// would return an index too), leaves it in sel for the gather and stores the row's code -- 0 for a stage the row does not take (RQ; sel
// keeps the real index).  Holds one barrier; the caller's next barrier publishes sel.  tid, wid, g, r16: the caller's thread coordinates
// (taken as arguments: recomputed here they cost rvq_encode_kernel<128, 1> two registers).
template <int RS, bool RQ>
__device__ __forceinline__ void rvq_argmax_merge(float (&best)[RS][4], int (&bidx)[RS][4], float (*bestv)[16 * RS], int (*besti)[16 * RS],
                                                 int* sel, const int* krow, int i, int K, int N, int row0, int64_t* codes, int tid, int wid,
                                                 int g, int r16) {
#pragma unroll
    for (int s2 = 0; s2 < RS; ++s2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const float ov = __shfl_xor(best[s2][r], o, 64);
                const int oi = __shfl_xor(bidx[s2][r], o, 64);
                if (ov > best[s2][r] || (ov == best[s2][r] && oi < bidx[s2][r])) { best[s2][r] = ov; bidx[s2][r] = oi; }
            }
            if (r16 == 0) { bestv[wid][16 * s2 + 4 * g + r] = best[s2][r]; besti[wid][16 * s2 + 4 * g + r] = bidx[s2][r]; }
        }
    }
    __syncthreads();
    if (tid < 16 * RS) {
        float bv = bestv[0][tid];
        int bi = besti[0][tid];
        for (int w = 1; w < 8; ++w) {
            const float ov = bestv[w][tid];
            const int oi = besti[w][tid];
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (bi < 0 || bi >= K) bi = 0;   // all-NaN row: torch would return an index too; stay in range
        sel[tid] = bi;
        if constexpr (RQ) { if (i >= krow[tid]) bi = 0; }       // a stage the row does not take: code 0 (sel stays in range for the gather)
        if (row0 + tid < N) codes[(size_t)i * N + row0 + tid] = (int64_t)bi;
    }
}

// RS = row sets of 16 rows per workgroup.  The stage is L2-bandwidth bound when one codebook load feeds only 16 rows
// (every workgroup streams the whole 512 KiB stage codebook: 250 workgroups x 512 KiB = 128 MiB per stage at config B);
// with RS = 2 the same registers feed two independent 16-row MFMA accumulators (same arithmetic per row).
// Q0: the stage-0 source-row table `src0` is honoured (quantizer_conf.q0_ds_ratio > 1); a template parameter so that the benchmark's
// instantiations keep their register allocation (183 registers, no spill).
// RQ: the per-batch-row stage counts `nq_rows` [N / Tf] are honoured (frame row n belongs to batch row n / Tf), a template parameter for
// the same reason.  A residual quantiser is a prefix code, so row r with count k_r runs its stages i < k_r exactly as without the table; for
// i >= k_r nothing is added to its quantised sum, its code and its sub_quant of that stage are 0, and what the row still computes while
// its neighbours go on stays in the row (every row has its own residual, MFMA output row and arg-max).  The workgroup ends after the
// largest count of its rows -- the same for all its threads, so the barriers of a stage stay uniform -- and writes the zeros of the
// stages it did not run.  nq is the cap: the first dimension of codes / subq, >= every count.
template <int D, int RS, bool Q0 = false, bool RQ = false>
__global__ __launch_bounds__(512) void rvq_encode_kernel(const float* __restrict__ x, int N, int K, int nq,
                                                         const float* __restrict__ cb, const float* __restrict__ cbf,
                                                         const float* __restrict__ enorm,
                                                         int64_t* __restrict__ codes, float* __restrict__ quant,
                                                         float* __restrict__ quant_bdt, float* __restrict__ subq, int Tf,
                                                         int ablate, const int* __restrict__ src0, const int* __restrict__ nq_rows) {
    constexpr int NQ4 = D / 16;
    constexpr int ROWS = 16 * RS;
    // residual rows, padded by 4 floats: the |x|^2 chains read R[r][32 j + i] from 64 lanes (r, j) at once -- with a row stride of
    // D every lane hit the same bank (32-way conflict, ~1 us per stage); stride D + 4 spreads the 8 rows of a lane group over 8 banks
    __shared__ __attribute__((aligned(16))) float R[ROWS][D + 4];
    constexpr int NEL = (ROWS * D + 511) / 512;                // elements of the row set owned by one thread: e = tid + 512 * it
    float qreg[NEL];                                    // running sum of the selected code rows (was an LDS array)
    __shared__ float xn[ROWS];
    __shared__ float bestv[8][ROWS];
    __shared__ int besti[8][ROWS];
    __shared__ int sel[ROWS];
    __shared__ int krow[RQ ? ROWS : 1];                 // RQ: stages of the workgroup's rows (0 behind row N)

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, r16 = lane & 15;
    const int row0 = blockIdx.x * ROWS;
    const int nqw = rvq_stage_counts<ROWS, RQ>(row0, N, nq, Tf, nq_rows, krow);      // stages this workgroup runs

    for (int e = tid; e < ROWS * D; e += 512) {
        const int r = e / D, d = e - r * D;
        const int n = row0 + r;
        // src0 (quantizer_conf.q0_ds_ratio > 1, ddp_core_vq.py:396-404): stage 0 quantises the row its frame copies from the
        // half-rate sequence; the residual update of that stage starts again from the row itself (below)
        R[r][d] = n < N ? x[(size_t)(Q0 ? src0[n] : n) * D + d] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < NEL; ++it) qreg[it] = 0.f;
    const int codes_per_wave = (K >> 3) < 16 ? 16 : (K >> 3);   // 8 waves: two per SIMD hide the codebook-row load latency
    const bool wactive = wid * codes_per_wave < K;            // small codebooks keep only K/16 waves busy

    constexpr bool DEEP = RS == 1;                                // one row set: codebook tiles two ahead (the two-row-set form has twice the MFMAs per tile)
    f32x4 b0[NQ4];                                               // first codebook fragment of the stage (requested one stage ahead)
    f32x4 b1p[DEEP ? NQ4 : 1];                                   // DEEP: the second one
    for (int i = 0; i < nqw; ++i) {
        __syncthreads();
        if (tid < 4 * ROWS) rvq_row_norm<D>(R[tid >> 2], tid & 3, &xn[tid >> 2]);   // |x|^2
        f32x4 a4[RS][NQ4];
#pragma unroll
        for (int s2 = 0; s2 < RS; ++s2)
#pragma unroll
            for (int q = 0; q < NQ4; ++q) {
                const f32x4 v = *(const f32x4*)&R[16 * s2 + r16][16 * q + 4 * g];
                a4[s2][q] = v + v;   // 2*x, exact
            }
        __syncthreads();
        float best[RS][4];
        int bidx[RS][4];
        float xr[RS][4];
#pragma unroll
        for (int s2 = 0; s2 < RS; ++s2)
#pragma unroll
            for (int r = 0; r < 4; ++r) { best[s2][r] = -INFINITY; bidx[s2][r] = 0x7fffffff; xr[s2][r] = xn[16 * s2 + 4 * g + r]; }
        const float* cbi = cb + (size_t)i * K * D;
        // One 16-code tile per trip, software pipelined: the codebook fragment of tile n+1 is requested before the 4*NQ4
        // MFMAs of tile n are issued (two register buffers), so the L2 latency of the stream hides behind the matrix work;
        // the second wave on the SIMD fills the dependent-MFMA bubbles.  Each (row, code) chain keeps its own d order.
        const int ntile = wactive ? codes_per_wave >> 4 : 0;
        const int code0 = wid * codes_per_wave;
        auto frag_ptr = [&](int stage, int t) __attribute__((always_inline)) {
            const int code = code0 + 16 * t;
            return cbf ? cbf + ((size_t)stage * K + code) * D + lane * 4 : cb + ((size_t)stage * K + code + r16) * D + 4 * g;
        };
        const int qstep = cbf ? 256 : 16;
        auto load_tile = [&](int stage, int t, f32x4 (&bq)[NQ4]) __attribute__((always_inline)) {
            const float* e0 = frag_ptr(stage, t);
#pragma unroll
            for (int q = 0; q < NQ4; ++q) bq[q] = FC_ABL(ablate, 2) ? (f32x4){1.f, 1.f, 1.f, 1.f} : *(const f32x4*)(e0 + qstep * q);
        };
        auto do_tile = [&](int t, const f32x4 (&bq)[NQ4]) __attribute__((always_inline)) {
            const int code = code0 + 16 * t + r16;
            const float en = enorm[(size_t)i * K + code];
            f32x4 acc[RS];
#pragma unroll
            for (int s2 = 0; s2 < RS; ++s2) acc[s2] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (!FC_ABL(ablate, 1)) {
#pragma unroll
                for (int q = 0; q < NQ4; ++q)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int s2 = 0; s2 < RS; ++s2)
                            acc[s2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[s2][q][j], bq[q][j], acc[s2], 0, 0, 0);
            }
#pragma unroll
            for (int s2 = 0; s2 < RS; ++s2)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dist = -__fadd_rn(__fsub_rn(xr[s2][r], acc[s2][r]), en);
                    if (dist > best[s2][r]) { best[s2][r] = dist; bidx[s2][r] = code; }
                }
        };
        if (ntile > 0) {
            if constexpr (DEEP) {
                // Round 5: codebook tiles are requested TWO tiles ahead (three register buffers).  With one tile ahead the L2 round trip of a
                // fragment (~1 us under this load) is as long as the 2 x 0.43 us of MFMAs of the two waves that share a SIMD.  Measured: 525 -> 517 us
                // (of the 80 us the codebook loads cost on top of the MFMAs -- tools/ablate_rvq.py -- most is their issue time, not latency)
                f32x4 b2[NQ4];
                if (i == 0) { load_tile(0, 0, b0); if (ntile > 1) load_tile(0, 1, b1p); }
                int t = 0;
                for (; t + 3 <= ntile; t += 3) {
                    load_tile(i, t + 2, b2);
                    do_tile(t, b0);
                    if (t + 3 < ntile) load_tile(i, t + 3, b0);
                    do_tile(t + 1, b1p);
                    if (t + 4 < ntile) load_tile(i, t + 4, b1p);
                    do_tile(t + 2, b2);
                }
                if (t < ntile) do_tile(t, b0);                 // 0, 1 or 2 tiles left: already requested into b0 / b1p
                if (t + 1 < ntile) do_tile(t + 1, b1p);
                // the next stage's first fragments do not depend on this stage's result: requested now, the arg-max / residual-update tail
                // of this stage hides their latency
                if (i + 1 < nqw) { load_tile(i + 1, 0, b0); if (ntile > 1) load_tile(i + 1, 1, b1p); }
            } else {
                f32x4 b1[NQ4];
                if (i == 0) load_tile(0, 0, b0);
                int t = 0;
                for (; t + 2 <= ntile; t += 2) {
                    load_tile(i, t + 1, b1);
                    do_tile(t, b0);
                    if (t + 2 < ntile) load_tile(i, t + 2, b0);
                    do_tile(t + 1, b1);
                }
                if (t < ntile) do_tile(t, b0);
                // the next stage's first fragment does not depend on this stage's result: request it now, the arg-max /
                // residual-update tail of this stage hides its latency
                if (i + 1 < nqw) load_tile(i + 1, 0, b0);
            }
        }
        rvq_argmax_merge<RS, RQ>(best, bidx, bestv, besti, sel, krow, i, K, N, row0, codes, tid, wid, g, r16);
        __syncthreads();
        // gather the selected code rows: all loads first (they are independent), then the LDS / register updates
        float qv[NEL];
#pragma unroll
        for (int it = 0; it < NEL; ++it) {
            const int e = tid + 512 * it, r = e / D, d = e - r * D;
            qv[it] = 0.f;
            if (ROWS * D % 512 == 0 || e < ROWS * D) qv[it] = FC_ABL(ablate, 8) ? 0.001f : cbi[(size_t)sel[r] * D + d];
        }
#pragma unroll
        for (int it = 0; it < NEL; ++it) {
            const int e = tid + 512 * it, r = e / D, d = e - r * D;
            if (ROWS * D % 512 != 0 && e >= ROWS * D) continue;
            const int n = row0 + r;
            float res = R[r][d];
            if (Q0 && i == 0 && n < N) res = x[(size_t)n * D + d];
            R[r][d] = res - qv[it];
            bool keep = true;
            if constexpr (RQ) keep = i < krow[r];
            if (keep) qreg[it] = qreg[it] + qv[it];
            if (subq && n < N && !FC_ABL(ablate, 4)) {
                const int bb = n / Tf, t = n - bb * Tf;
                const int Bn = N / Tf;
                subq[(((size_t)i * Bn + bb) * D + d) * Tf + t] = keep ? qv[it] : 0.f;
            }
        }
    }
    // The two tails; rvq_encode_wide_kernel repeats them line for line (why they are not one function: the note above
    // rvq_stage_counts).  An edit here is an edit there.
    if constexpr (RQ) {       // the stages behind the workgroup's last one: codes and sub_quants 0
        if (tid < ROWS && row0 + tid < N)
            for (int i = nqw; i < nq; ++i) codes[(size_t)i * N + row0 + tid] = 0;
        if (subq)
            for (int i = nqw; i < nq; ++i)
#pragma unroll
                for (int it = 0; it < NEL; ++it) {
                    const int e = tid + 512 * it, r = e / D, d = e - r * D;
                    const int n = row0 + r;
                    if (n >= N || (ROWS * D % 512 != 0 && e >= ROWS * D)) continue;
                    const int bb = n / Tf, t = n - bb * Tf;
                    const int Bn = N / Tf;
                    subq[(((size_t)i * Bn + bb) * D + d) * Tf + t] = 0.f;
                }
    }
#pragma unroll
    for (int it = 0; it < NEL; ++it) {
        const int e = tid + 512 * it, r = e / D, d = e - r * D;
        const int n = row0 + r;
        if (n >= N || (ROWS * D % 512 != 0 && e >= ROWS * D)) continue;
        const float v = qreg[it];
        if (quant) quant[(size_t)n * D + d] = v;
        if (quant_bdt) {
            const int bb = n / Tf, t = n - bb * Tf;
            quant_bdt[((size_t)bb * D + d) * Tf + t] = v;
        }
    }
}

// Wide codebooks (D = 512, the SoundStream recipe): the shared steps above around its own matrix loop.  A (row, code) chain is fed in
// chunks of 256 dims -- the 2x fragment of the row (re-read from LDS per chunk) and the two in-flight codebook fragments then fit the
// register file -- and the residual update fuses each gather with its use.  Q0, RQ: see rvq_encode_kernel.
template <int D, bool Q0 = false, bool RQ = false>
__global__ __launch_bounds__(512) void rvq_encode_wide_kernel(const float* __restrict__ x, int N, int K, int nq,
                                                              const float* __restrict__ cb, const float* __restrict__ cbf,
                                                              const float* __restrict__ enorm,
                                                              int64_t* __restrict__ codes, float* __restrict__ quant,
                                                              float* __restrict__ quant_bdt, float* __restrict__ subq, int Tf,
                                                              const int* __restrict__ src0, const int* __restrict__ nq_rows) {
    static_assert(D % 256 == 0, "chunks of 256 dims");
    constexpr int NC = D / 256, CQ = 16, NEL = 16 * D / 512;
    __shared__ __attribute__((aligned(16))) float R[16][D];
    __shared__ float xn[16];
    __shared__ float bestv[8][16];
    __shared__ int besti[8][16];
    __shared__ int sel[16];
    __shared__ int krow[RQ ? 16 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, r16 = lane & 15;
    const int row0 = blockIdx.x * 16;
    const int nqw = rvq_stage_counts<16, RQ>(row0, N, nq, Tf, nq_rows, krow);
    float qreg[NEL];                                     // running sum of the selected code rows, element e = tid + 512*i
#pragma unroll
    for (int i2 = 0; i2 < NEL; ++i2) {
        const int e = tid + 512 * i2, r = e / D, d = e - r * D, n = row0 + r;
        R[r][d] = n < N ? x[(size_t)(Q0 ? src0[n] : n) * D + d] : 0.f;       // Q0 / src0: see rvq_encode_kernel
        qreg[i2] = 0.f;
    }
    const int codes_per_wave = (K >> 3) < 16 ? 16 : (K >> 3);
    const bool wactive = wid * codes_per_wave < K;
    const int ntile = wactive ? codes_per_wave >> 4 : 0, nunit = ntile * NC;
    const int code0 = wid * codes_per_wave;
    for (int i = 0; i < nqw; ++i) {
        __syncthreads();
        if (tid < 64) rvq_row_norm<D>(R[tid >> 2], tid & 3, &xn[tid >> 2]);   // |x|^2
        __syncthreads();
        float best[1][4], xr[4];
        int bidx[1][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { best[0][r] = -INFINITY; bidx[0][r] = 0x7fffffff; xr[r] = xn[4 * g + r]; }
        const float* cbi = cb + (size_t)i * K * D;
        auto load_unit = [&](int u, f32x4 (&bq)[CQ]) __attribute__((always_inline)) {
            const int t = u / NC, c = u - t * NC, code = code0 + 16 * t;
            const float* e0 = cbf ? cbf + ((size_t)i * K + code) * D + (size_t)c * CQ * 256 + lane * 4
                                  : cbi + (size_t)(code + r16) * D + 256 * c + 4 * g;
            const int qstep = cbf ? 256 : 16;
#pragma unroll
            for (int q = 0; q < CQ; ++q) bq[q] = *(const f32x4*)(e0 + qstep * q);
        };
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        auto do_unit = [&](int u, const f32x4 (&bq)[CQ]) __attribute__((always_inline)) {
            const int t = u / NC, c = u - t * NC, code = code0 + 16 * t + r16;
            if (c == 0) acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < CQ; ++q) {
                const f32x4 v = *(const f32x4*)&R[r16][256 * c + 16 * q + 4 * g];
                const f32x4 a = v + v;                                  // 2*x, exact
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bq[q][j], acc, 0, 0, 0);
            }
            if (c == NC - 1) {
                const float en = enorm[(size_t)i * K + code];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dist = -__fadd_rn(__fsub_rn(xr[r], acc[r]), en);
                    if (dist > best[0][r]) { best[0][r] = dist; bidx[0][r] = code; }
                }
            }
        };
        if (nunit > 0) {
            f32x4 b0[CQ], b1[CQ];
            load_unit(0, b0);
            int u = 0;
            for (; u + 2 <= nunit; u += 2) {
                load_unit(u + 1, b1);
                do_unit(u, b0);
                if (u + 2 < nunit) load_unit(u + 2, b0);
                do_unit(u + 1, b1);
            }
            if (u < nunit) do_unit(u, b0);
        }
        rvq_argmax_merge<1, RQ>(best, bidx, bestv, besti, sel, krow, i, K, N, row0, codes, tid, wid, g, r16);
        __syncthreads();
#pragma unroll
        for (int i2 = 0; i2 < NEL; ++i2) {
            const int e = tid + 512 * i2, r = e / D, d = e - r * D, n = row0 + r;
            const float qv = cbi[(size_t)sel[r] * D + d];
            float res = R[r][d];
            if (Q0 && i == 0 && n < N) res = x[(size_t)n * D + d];
            R[r][d] = res - qv;
            bool keep = true;
            if constexpr (RQ) keep = i < krow[r];
            if (keep) qreg[i2] = qreg[i2] + qv;
            if (subq && n < N) {
                const int bb = n / Tf, t = n - bb * Tf, Bn = N / Tf;
                subq[(((size_t)i * Bn + bb) * D + d) * Tf + t] = keep ? qv : 0.f;
            }
        }
    }
    // The two tails, line for line those of rvq_encode_kernel (why they are not one function: the note above rvq_stage_counts).  An edit
    // here is an edit there.
    if constexpr (RQ) {
        if (tid < 16 && row0 + tid < N)
            for (int i = nqw; i < nq; ++i) codes[(size_t)i * N + row0 + tid] = 0;
        if (subq)
            for (int i = nqw; i < nq; ++i)
#pragma unroll
                for (int i2 = 0; i2 < NEL; ++i2) {
                    const int e = tid + 512 * i2, r = e / D, d = e - r * D, n = row0 + r;
                    if (n >= N) continue;
                    const int bb = n / Tf, t = n - bb * Tf, Bn = N / Tf;
                    subq[(((size_t)i * Bn + bb) * D + d) * Tf + t] = 0.f;
                }
    }
#pragma unroll
    for (int i2 = 0; i2 < NEL; ++i2) {
        const int e = tid + 512 * i2, r = e / D, d = e - r * D, n = row0 + r;
        if (n >= N) continue;
        if (quant) quant[(size_t)n * D + d] = qreg[i2];
        if (quant_bdt) {
            const int bb = n / Tf, t = n - bb * Tf;
            quant_bdt[((size_t)bb * D + d) * Tf + t] = qreg[i2];
        }
    }
}

// quantizer_conf.q0_ds_ratio > 1 (ddp_core_vq.py:396-404): map[b * Tf + t] = b * Tf + q0_source_frame(t, Tf)   (kernels.h)
__global__ __launch_bounds__(256) void q0_map_kernel(int* __restrict__ map, int Tf) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t < Tf) map[(size_t)b * Tf + t] = b * Tf + q0_source_frame(t, Tf);
}

hipError_t launch_q0_map(int* map, int B, int Tf, hipStream_t st) {
    if (B <= 0 || Tf < 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(q0_map_kernel, dim3(ceil_div(Tf, 256), B), dim3(256), 0, st, map, Tf);
    return hipGetLastError();
}

hipError_t launch_rvq_encode(const float* x, int N, int D, int K, int nq, const float* cb, const float* cb_frag,
                             const float* enorm, int64_t* codes, float* quant, float* quant_bdt, float* subq, int Tf, hipStream_t st,
                             const int* src0, const int* nq_rows) {
    if (N <= 0) return hipSuccess;
    if (K % 16 != 0 || (K > 128 && K % 128 != 0)) return hipErrorInvalidValue;
    if (nq_rows && (Tf <= 0 || N % Tf != 0)) return hipErrorInvalidValue;      // the table is indexed by n / Tf
    if (D == 512) {
#define FC_RVQ_WIDE(Q0_, RQ_)                                                                                                     \
    hipLaunchKernelGGL((rvq_encode_wide_kernel<512, Q0_, RQ_>), dim3(ceil_div(N, 16)), dim3(512), 0, st, x, N, K, nq, cb, cb_frag, enorm, \
                       codes, quant, quant_bdt, subq, Tf, src0, nq_rows)
        if (nq_rows) { if (src0) FC_RVQ_WIDE(true, true); else FC_RVQ_WIDE(false, true); }
        else if (src0) FC_RVQ_WIDE(true, false);
        else FC_RVQ_WIDE(false, false);
#undef FC_RVQ_WIDE
        return hipGetLastError();
    }
    // two row sets per workgroup once there are enough rows to keep ~half the CUs busy that way (L2 traffic halves)
    static const int ablate = ab_knob("FC_ABLATE_RVQ", 0);
    // Round 4 (tools/rvq_scaling.py): the kernel's time is linear in the workgroups per CU (one 8-wave workgroup per CU, 183 registers).
    // Up to 16 rows per CU the 16-row form is the fastest (497 vs 807 us at 4 000 rows); beyond that two row sets per workgroup -- the
    // codebook fragments of a stage are loaded once for both, 32 rows per MFMA pass -- take 413 us per 32 rows per CU against 2 x 489:
    // 846 vs 974 us at 8 000 rows, 1 613 vs 1 943 at 16 000.  FC_RVQ_TWO=0 / 1 forces one form (A / B runs).
    static const int two_env = ab_knob("FC_RVQ_TWO", -1);
    // CU count of the CURRENT device, looked up per call from a table filled once per device (thread-safe: function-local static of a
    // type with a constructor; ADVICE r4: the round-4 form cached whichever device was current at the first call, unsynchronised)
    struct CuTable {
        int n[64];
        CuTable() {
            int nd = 0;
            if (hipGetDeviceCount(&nd) != hipSuccess) nd = 0;
            for (int d = 0; d < 64; ++d) {
                hipDeviceProp_t prop;
                n[d] = (d < nd && hipGetDeviceProperties(&prop, d) == hipSuccess) ? prop.multiProcessorCount : 256;
            }
        }
    };
    static const CuTable cu_table;
    int cur_dev = 0;
    (void)hipGetDevice(&cur_dev);
    const int n_cus = cu_table.n[cur_dev & 63];
    const bool two = !src0 && D <= 128 && (two_env >= 0 ? (two_env != 0 && N >= 2048) : N > 16 * n_cus);
    dim3 grid(ceil_div(N, two ? 32 : 16)), block(512);
#define FC_RVQ_FORM(DD, RS_, Q0_, RQ_)                                                                             \
    hipLaunchKernelGGL((rvq_encode_kernel<DD, RS_, Q0_, RQ_>), grid, block, 0, st, x, N, K, nq, cb, cb_frag, enorm, codes, quant, quant_bdt, \
                       subq, Tf, ablate, src0, nq_rows)
#define FC_RVQ_CASE(DD)                                                                                            \
    case DD:                                                                                                       \
        if (nq_rows) {                                     /* the same choice of form, with the per-row stage counts */ \
            if (two) FC_RVQ_FORM((DD <= 128 ? DD : 16), 2, false, true);                                           \
            else if (src0) FC_RVQ_FORM(DD, 1, true, true);                                                         \
            else FC_RVQ_FORM(DD, 1, false, true);                                                                  \
        } else if (two) FC_RVQ_FORM((DD <= 128 ? DD : 16), 2, false, false);                                       \
        else if (src0) FC_RVQ_FORM(DD, 1, true, false);                                                            \
        else FC_RVQ_FORM(DD, 1, false, false);                                                                     \
        break;
    switch (D) {
        FC_RVQ_CASE(16)
        FC_RVQ_CASE(32)
        FC_RVQ_CASE(64)
        FC_RVQ_CASE(128)
        FC_RVQ_CASE(256)
        default: return hipErrorInvalidValue;
    }
#undef FC_RVQ_CASE
#undef FC_RVQ_FORM
    return hipGetLastError();
}

// DRVQ.decode (ddp_core_vq.py:442-453): out = ((0 + E_0[i0]) + E_1[i1]) + ...
// counts (rvq_rate_kernels.h): frame row n sums its first k stages; the codes behind them are not read.  rows (lens given): a frame behind
// its row's frames sums none
__global__ __launch_bounds__(256) void rvq_decode_kernel(const int64_t* __restrict__ codes, int Tf, int nq, int D, int K,
                                                         const float* __restrict__ cb, float* __restrict__ emb,
                                                         float* __restrict__ emb_bdt, unsigned* __restrict__ status,
                                                         StageCounts counts, RagLen rows) {
    const int n = blockIdx.x;   // row = b*Tf + t
    const int b = n / Tf, t = n - b * Tf;
    const int k = t < row_frames(rows, b, Tf) ? stage_count(counts, n, b, nq) : 0;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float s = 0.f;
        for (int i = 0; i < k; ++i) {
            long long idx = codes[(size_t)n * nq + i];
            // F.embedding raises on an index outside [0, K) (ddp_core_vq.py:191): never read out of bounds, but make the
            // corrupt token loud -- the engine status word reports it (fc_engine_status)
            if (idx < 0 || idx >= K) {
                if (status && threadIdx.x == 0) *(volatile unsigned*)(status + FC_STATUS_BAD_CODE) = 1u;
                idx = idx < 0 ? 0 : K - 1;
            }
            s = s + cb[((size_t)i * K + idx) * D + d];
        }
        if (emb) emb[(size_t)n * D + d] = s;
        if (emb_bdt) emb_bdt[((size_t)b * D + d) * Tf + t] = s;
    }
}

hipError_t launch_rvq_decode(const int64_t* codes, int B, int Tf, int nq, int D, int K, const float* cb, float* emb, float* emb_bdt,
                             unsigned* status, const StageCounts& k, const RagLen& rows, hipStream_t st) {
    if ((long long)B * Tf <= 0) return hipSuccess;
    if (nq < 1) return hipErrorInvalidValue;
    const int threads = D >= 256 ? 256 : (D >= 128 ? 128 : 64);
    hipLaunchKernelGGL(rvq_decode_kernel, dim3(B * Tf), dim3(threads), 0, st, codes, Tf, nq, D, K, cb, emb, emb_bdt, status, k, rows);
    return hipGetLastError();
}

// quant / quant_bdt / subq of the final codes: one workgroup per frame, the sum in stage order from 0 (launch_rvq_decode's order) over the
// frame's first k codes (counts: rvq_rate_kernels.h)
__global__ __launch_bounds__(256) void rvq_codes_sum_kernel(const int64_t* __restrict__ codes, int N, int Tf, int nq, int D, int K,
                                                            const float* __restrict__ cb, float* __restrict__ quant,
                                                            float* __restrict__ quant_bdt, float* __restrict__ subq, StageCounts counts) {
    const int n = blockIdx.x;
    const int b = n / Tf, t = n - b * Tf, Bn = N / Tf;
    const int k = stage_count(counts, n, b, nq);
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float s = 0.f;
        for (int i = 0; i < nq; ++i) {
            float v = 0.f;
            if (i < k) {
                long long idx = codes[(size_t)i * N + n];
                if (idx < 0 || idx >= K) idx = 0;            // the search writes codes in range; never read out of bounds
                v = cb[((size_t)i * K + idx) * D + d];
                s = s + v;
            }
            if (subq) subq[(((size_t)i * Bn + b) * D + d) * Tf + t] = v;
        }
        if (quant) quant[(size_t)n * D + d] = s;
        if (quant_bdt) quant_bdt[((size_t)b * D + d) * Tf + t] = s;
    }
}

hipError_t launch_rvq_codes_sum(const int64_t* codes, int N, int D, int K, int nq, const float* cb, float* quant, float* quant_bdt, float* subq,
                                int Tf, const StageCounts& k, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    if (Tf <= 0 || N % Tf != 0 || nq < 1) return hipErrorInvalidValue;
    const int threads = D >= 256 ? 256 : (D >= 128 ? 128 : 64);
    hipLaunchKernelGGL(rvq_codes_sum_kernel, dim3(N), dim3(threads), 0, st, codes, N, Tf, nq, D, K, cb, quant, quant_bdt, subq, k);
    return hipGetLastError();
}

}  // namespace fc
