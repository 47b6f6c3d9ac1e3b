// gfx950 (MI355X / CDNA4) attention of the SEANet transformer bottleneck (seq_kernels.h): MultiHeadedAttention.forward
// (funcodec/modules/attention.py:16-115) with an all-ones mask, optionally causal, over channel-major q | k | v.
//
// Flash-style: one wave = 16 queries of one (utterance, head); it streams the keys in 16-key tiles and keeps, per query, the running
// maximum and sum of exponentials of the online softmax in fp32.  Nothing is held per key, so T is unbounded.
//
// Both products run on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate) in the TRANSPOSED orientation, so that the query sits on the
// lane and every per-query quantity is lane-local:
//   S^T [key][query]  = K [key][dim] . Q^T [dim][query]     A = K (16 keys x 4 dims per step), B = Q^T (4 dims x 16 queries)
//   O^T [dim][query] += V [dim][key] . P^T [key][query]     A = V (16 dims x 4 keys per step), B = P^T straight from the S^T accumulator
// MFMA 16x16x4 operand layout: lane l = 16 g + r;  A operand = A[row r][k g];  B operand = B[k g][col r];  accumulator register v =
// D[row 4 g + v][col r].  The S^T accumulator of lane (g, r) holds keys 4 g + v of query r, which is exactly the B operand of the
// P^T step v (k index g <-> key 4 g + v): no data movement between the two products.
//
// Masking (causal, tail keys past T): a masked entry gets probability exactly 0 and is left out of the running maximum, so it adds
// exactly nothing (0 * v) and a query's result does not depend on keys it cannot see.  Key tiles wholly above the diagonal are skipped.
#include "seq_kernels.h"
#include "device_common.h"

namespace fc {

namespace {

template <int DK>
__global__ __launch_bounds__(256) void seq_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int H, int T, int causal,
                                                       float scale) {
    constexpr int NC = DK / 4;     // k steps of Q . K (4 dims each)
    constexpr int ND = DK / 16;    // 16-dim tiles of the output
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, r = lane & 15;
    const int i0 = (blockIdx.x * 4 + w) * 16;
    if (i0 >= T) return;
    const int h = blockIdx.y, b = blockIdx.z, C = H * DK;
    const size_t Tz = (size_t)T;
    const float* qb = qkv + ((size_t)b * 3 * C + (size_t)h * DK) * Tz;
    const float* kb = qb + (size_t)C * Tz;
    const float* vb = kb + (size_t)C * Tz;
    const int iq = i0 + r;                                   // this lane's query (rows past T are computed on a clamped copy, not written)
    const int iqc = iq < T ? iq : T - 1;
    float qf[NC];                                            // B operand of step c: Q[query r][dim 4 c + g]
#pragma unroll
    for (int c = 0; c < NC; ++c) qf[c] = qb[(size_t)(4 * c + g) * Tz + iqc];
    f32x4 o[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float NEG_INF = -__builtin_inff();
    float m = NEG_INF, l = 0.f;
    int jend = T;
    if (causal && i0 + 16 < T) jend = i0 + 16;               // tiles past the diagonal tile are invisible to every query of the wave
    for (int j0 = 0; j0 < jend; j0 += 16) {
        const int jk = j0 + r < T ? j0 + r : T - 1;
        // ---- S^T = K . Q^T (two accumulation chains: the dependent-issue latency of the 16x16x4 form is 40 cycles)
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
        for (int c = 0; c < NC; c += 2) {
            s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[(size_t)(4 * c + g) * Tz + jk], qf[c], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[(size_t)(4 * c + 4 + g) * Tz + jk], qf[c + 1], s1, 0, 0, 0);
        }
        // ---- online softmax: lane (g, r) holds keys j0 + 4 g + v of query r; the other three key groups sit in lanes r + 16, 32, 48
        float p[4];
        unsigned vis = 0;
        float tmax = NEG_INF;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + 4 * g + v;
            const bool ok = j < T && (!causal || j <= iq);
            p[v] = (s0[v] + s1[v]) * scale;
            if (ok) { vis |= 1u << v; tmax = fmaxf(tmax, p[v]); }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);
        const float alpha = m == NEG_INF ? 0.f : expf(m - mn);
        float ts = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            p[v] = (vis >> v) & 1u ? expf(p[v] - mn) : 0.f;
            ts += p[v];
        }
        ts += __shfl_xor(ts, 16, 64);
        ts += __shfl_xor(ts, 32, 64);
        l = l * alpha + ts;
        m = mn;
        // ---- O^T = alpha O^T + V . P^T
        const bool full = j0 + 16 <= T;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const float* vrow = vb + (size_t)(16 * d + r) * Tz;
            f32x4 vv;
            if (full) {
                vv = *(const f32x4u*)(vrow + j0 + 4 * g);    // rows are not 16-byte aligned unless T % 4 == 0
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int j = j0 + 4 * g + v;
                    vv[v] = vrow[j < T ? j : T - 1];         // finite stand-in for a tail key: its probability is exactly 0
                }
            }
            o[d] *= alpha;
#pragma unroll
            for (int v = 0; v < 4; ++v) o[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[v], p[v], o[d], 0, 0, 0);
        }
    }
    if (iq >= T) return;
    const float inv = 1.f / l;
    float* ob = out + ((size_t)b * C + (size_t)h * DK) * Tz + iq;
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int v = 0; v < 4; ++v) ob[(size_t)(16 * d + 4 * g + v) * Tz] = o[d][v] * inv;
}

}  // namespace

bool seq_attn_supported(int DK) { return DK == 16 || DK == 32 || DK == 64 || DK == 128 || DK == 256; }

const char* seq_attn_kernel_name(int DK) {
    switch (DK) {
        case 16: return "seq_attn_kernel<16>";
        case 32: return "seq_attn_kernel<32>";
        case 64: return "seq_attn_kernel<64>";
        case 128: return "seq_attn_kernel<128>";
        default: return "seq_attn_kernel<256>";
    }
}

hipError_t launch_seq_attn(const SeqAttn& a, hipStream_t st) {
    if (!a.qkv || !a.out || a.B < 1 || a.H < 1 || a.T < 1 || !seq_attn_supported(a.DK)) return hipErrorInvalidValue;
    const dim3 grid((a.T + 63) / 64, a.H, a.B), block(256);
    const float scale = 1.f / sqrtf((float)a.DK);
    switch (a.DK) {
        case 16: hipLaunchKernelGGL(seq_attn_kernel<16>, grid, block, 0, st, a.qkv, a.out, a.H, a.T, a.causal, scale); break;
        case 32: hipLaunchKernelGGL(seq_attn_kernel<32>, grid, block, 0, st, a.qkv, a.out, a.H, a.T, a.causal, scale); break;
        case 64: hipLaunchKernelGGL(seq_attn_kernel<64>, grid, block, 0, st, a.qkv, a.out, a.H, a.T, a.causal, scale); break;
        case 128: hipLaunchKernelGGL(seq_attn_kernel<128>, grid, block, 0, st, a.qkv, a.out, a.H, a.T, a.causal, scale); break;
        default: hipLaunchKernelGGL(seq_attn_kernel<256>, grid, block, 0, st, a.qkv, a.out, a.H, a.T, a.causal, scale); break;
    }
    return hipGetLastError();
}

}  // namespace fc
