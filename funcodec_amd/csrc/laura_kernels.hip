// gfx950 (MI355X / CDNA4) kernels of the LauraTTS generation path (laura_kernels.h).  fp32 everywhere; contractions on the
// fp32-input matrix cores (v_mfma_f32_16x16x4_f32: an fmaf chain in k order, no narrower arithmetic).  Wavefront = 64 lanes.
//
// MFMA 16x16x4 operand layout (as used by the codec kernels): lane l = 16 g + r;  A operand = A[row r][k g];
// B operand = B[k g][col r];  accumulator register v = D[row 4 g + v][col r].
#include "laura_kernels.h"
#include "kernels.h"
#include "device_common.h"

#include <atomic>
#include <cstdlib>

namespace fc {
namespace laura {

namespace {

__device__ __forceinline__ int ceil_div_d(int a, int b) { return (a + b - 1) / b; }
inline int ceil_div_h(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float act_f(float v, int act) {
    if (act == 1) return v > 0.f ? v : 0.f;
    if (act == 2) return v / (1.f + expf(-v));      // Swish: x * sigmoid(x) (nets_utils.py:568-574)
    return v;
}

// opt-in to > 64 KiB of dynamic LDS, once per (kernel, device)
template <typename F>
hipError_t big_lds(F kfn, std::atomic<unsigned long long>& done, int bytes = 160 * 1024) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
        done.fetch_or(bit, std::memory_order_release);
    }
    return hipSuccess;
}

}  // namespace

// =====================================================================================================================
// LayerNorm over the channel axis of a feature-major tensor (torch.nn.LayerNorm, biased variance; eps 1e-12 inside the blocks,
// funcodec/modules/layer_norm.py:22, 1e-5 in the input layers).  One thread column per time step (coalesced over t), the C
// channels split over 4 thread rows; two-pass mean / variance in fp32.
// =====================================================================================================================
// round 3: a workgroup = 16 time steps x 16 channel groups; a thread keeps its C / 16 values in registers (one read of the tensor, one
// write) and the statistics meet in LDS.  The first version (64 time steps x 4 channel groups, three passes over global memory) ran
// 56 workgroups for a batch of 8 x 430 columns and took ~100 us per call.
template <int CPT>                                     // channels per thread = C / 16 (<= CPT)
__global__ __launch_bounds__(256) void layernorm_fm_kernel(const float* __restrict__ x, const float* __restrict__ add, float* sum_out,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           int relu, float post_scale, float* __restrict__ y, int C, int T) {
    __shared__ float red[16][17];
    const int tx = threadIdx.x & 15, cg = threadIdx.x >> 4;
    const int t = blockIdx.x * 16 + tx, b = blockIdx.y;
    const bool ok = t < T;
    const size_t base = (size_t)b * C * T + (ok ? t : 0);
    const int cpt = C / 16, c0 = cg * cpt;
    float v[CPT];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        v[i] = 0.f;
        if (i < cpt) {
            float u = x[base + (size_t)(c0 + i) * T];
            if (add) u += add[base + (size_t)(c0 + i) * T];
            v[i] = u;
            s += u;
        }
    }
    red[cg][tx] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) tot += red[g][tx];
    const float mean = tot / (float)C;
    __syncthreads();
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (i < cpt) { const float dv = v[i] - mean; q += dv * dv; }
    red[cg][tx] = q;
    __syncthreads();
    tot = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) tot += red[g][tx];
    const float rstd = 1.f / sqrtf(tot / (float)C + eps);
    if (!ok) return;
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (i < cpt) {
            const int c = c0 + i;
            if (sum_out) sum_out[base + (size_t)c * T] = v[i];
            float o = (v[i] - mean) * rstd * gamma[c] + beta[c];
            if (relu) o = o > 0.f ? o : 0.f;
            y[base + (size_t)c * T] = o * post_scale;
        }
}

hipError_t launch_layernorm_fm(const float* x, const float* add, float* sum_out, const float* gamma, const float* beta, float eps,
                               int relu, float post_scale, float* y, int B, int C, int T, hipStream_t st) {
    if (C % 16 || C > 1024) return hipErrorInvalidValue;
    const dim3 grid(ceil_div_h(T, 16), B);
    if (C <= 128) hipLaunchKernelGGL(layernorm_fm_kernel<8>, grid, dim3(256), 0, st, x, add, sum_out, gamma, beta, eps, relu, post_scale, y, C, T);
    else if (C <= 512) hipLaunchKernelGGL(layernorm_fm_kernel<32>, grid, dim3(256), 0, st, x, add, sum_out, gamma, beta, eps, relu, post_scale, y, C, T);
    else hipLaunchKernelGGL(layernorm_fm_kernel<64>, grid, dim3(256), 0, st, x, add, sum_out, gamma, beta, eps, relu, post_scale, y, C, T);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void act_kernel(float* x, size_t n, int act) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
        f32x4 v = *(f32x4*)(x + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_f(v[j], act);
        *(f32x4*)(x + i) = v;
    } else {
        for (size_t k = i; k < n; ++k) x[k] = act_f(x[k], act);
    }
}
hipError_t launch_act(float* x, size_t n, int act, hipStream_t st) {
    if (!act || !n) return hipSuccess;
    hipLaunchKernelGGL(act_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, st, x, n, act);
    return hipGetLastError();
}

// =====================================================================================================================
// Full-sequence rel-pos attention (RelPositionMultiHeadedAttention.forward, funcodec/modules/attention.py:265-308 +
// forward_attention :64-96).  One workgroup = 16 queries of one (utterance, head):
//   A  scores of the 16 queries against every key tile (4 waves, one 16-key tile each per trip) into LDS:
//        ac = (q + u) . k_j                       one 16x16 MFMA tile
//        bd = (q + v) . p_{i-j}                   the 31 relative positions of the tile as two MFMA tiles against the position
//                                                 table, the (i, j) diagonal picked through LDS (= the reference's rel_shift)
//        s  = (ac + bd) / sqrt(dk), masked (padding; causal with a bidirectional prefix block for the LM)
//   B  row softmax in LDS (max, exp, sum, divide; masked entries 0 like masked_fill(mask, 0.0))
//   C  ctx = P . V: wave w owns 16 of the dk output dims, A operand = probabilities from LDS, B operand = V rows (16-byte loads)
// =====================================================================================================================
struct AttnFullArgs {
    const float *qkv, *ptab, *bias_u, *bias_v;
    const int *lens, *bidir;
    float* ctx;
    int causal, H, T, R, PR, SW;     // SW = LDS row stride of the score block
};

template <int DK>
__global__ __launch_bounds__(256) void attn_full_kernel(AttnFullArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* S = lds;                          // [16][SW]
    float* Gs = lds + 16 * a.SW;             // [4 waves][16][33]
    constexpr int NC = DK / 16;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, r16 = lane & 15;
    const int i0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
    const int T = a.T, d = a.H * DK;
    const int len = a.lens[b];
    const int bid = (a.causal && a.bidir) ? a.bidir[b] : 0;
    if (i0 >= len) {       // padded queries: the reference computes garbage there too and every consumer masks them; write zeros
        if (w < NC) {
            const int t0 = i0 + 4 * g;
            if (t0 < T) *(f32x4*)(a.ctx + ((size_t)b * d + h * DK + 16 * w + r16) * T + t0) = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        return;
    }
    // key tiles this query tile can see at all
    int nkt = ceil_div_d(len, 16);
    if (a.causal) {
        int lim = i0 + 16;
        if (bid > lim) lim = bid;
        if (lim < len) nkt = ceil_div_d(lim, 16);
    }
    const float* qb = a.qkv + (size_t)b * 3 * d * T;
    const float* kb = qb + (size_t)d * T;
    const float* vb = kb + (size_t)d * T;
    // query fragments (A operand): lane (r16 = query, g) holds dims 16 c + 4 g + j
    const int iq = (i0 + r16 < T) ? i0 + r16 : T - 1;
    float qu[NC][4], qv[NC][4];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dd = h * DK + 16 * c + 4 * g + j;
            const float q = qb[(size_t)dd * T + iq];
            qu[c][j] = q + a.bias_u[dd];
            qv[c][j] = q + a.bias_v[dd];
        }
    const float scale = 1.f / sqrtf((float)DK);
    const float NEG = -3.4028234663852886e38f;       // numpy.finfo(float32).min (attention.py:79-82)
    float* Gw = Gs + w * 16 * 33;
    const int ntrip = ceil_div_d(nkt, 4);
    for (int trip = 0; trip < ntrip; ++trip) {
        const int kt = trip * 4 + w;
        const bool active = kt < nkt;
        const int j0 = kt * 16;
        f32x4 ac = {0.f, 0.f, 0.f, 0.f}, g0 = ac, g1 = ac;
        if (active) {
            const int jk = (j0 + r16 < T) ? j0 + r16 : T - 1;
            const int rlo = i0 - j0 - 15 + (a.R - 1);                 // table column of window column 0
            int p0 = rlo + r16, p1 = rlo + 16 + r16;
            p0 = p0 < 0 ? 0 : (p0 >= a.PR ? a.PR - 1 : p0);
            p1 = p1 < 0 ? 0 : (p1 >= a.PR ? a.PR - 1 : p1);
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int dd = h * DK + 16 * c + 4 * g + j;
                    const float kv = kb[(size_t)dd * T + jk];
                    const float pa = a.ptab[(size_t)dd * a.PR + p0];
                    const float pb = a.ptab[(size_t)dd * a.PR + p1];
                    ac = __builtin_amdgcn_mfma_f32_16x16x4f32(qu[c][j], kv, ac, 0, 0, 0);
                    g0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qv[c][j], pa, g0, 0, 0, 0);
                    g1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qv[c][j], pb, g1, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Gw[(4 * g + r) * 33 + r16] = g0[r];
                Gw[(4 * g + r) * 33 + 16 + r16] = g1[r];
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = 4 * g + r, i = i0 + il, j = j0 + r16;
                const float bd = Gw[il * 33 + (il - r16 + 15)];      // window column of relative position i - j
                bool vis = j < len;
                if (a.causal) vis = vis && (j <= i || (i < bid && j < bid));
                S[il * a.SW + j] = vis ? (ac[r] + bd) * scale : NEG;
            }
        }
        __syncthreads();
    }
    // ---- B: softmax, 16 threads per row
    {
        const int row = tid >> 4, part = tid & 15;
        const int nk = nkt * 16;
        float* Sr = S + row * a.SW;
        float m = NEG;
        for (int j = part; j < nk; j += 16) m = fmaxf(m, Sr[j]);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float s = 0.f;
        for (int j = part; j < nk; j += 16) {
            const float v = Sr[j];
            const float e = (v == NEG) ? 0.f : expf(v - m);
            Sr[j] = e;
            s += e;
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float inv = s > 0.f ? 1.f / s : 0.f;
        for (int j = part; j < nk; j += 16) Sr[j] *= inv;
    }
    __syncthreads();
    // ---- C: ctx[i][dd] = sum_j P[i][j] V[dd][j]
    if (w < NC) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* vrow = vb + (size_t)(h * DK + 16 * w + r16) * T;
        for (int kt = 0; kt < nkt; ++kt) {
            const int j = kt * 16 + 4 * g;
            const f32x4 p = *(const f32x4*)(S + r16 * a.SW + j);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j < T) v = *(const f32x4*)(vrow + j);               // T % 4 == 0: the 16-byte piece is inside the row or past it
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(p[jj], v[jj], acc, 0, 0, 0);
        }
        const int t0 = i0 + 4 * g;
        if (t0 < T) *(f32x4*)(a.ctx + ((size_t)b * d + h * DK + 16 * w + r16) * T + t0) = acc;
    }
}

static int attn_sw(int T) { return ((T + 15) / 16) * 16 + 4; }
size_t attn_full_lds_bytes(int T) { return (size_t)(16 * attn_sw(T) + 4 * 16 * 33) * sizeof(float); }

hipError_t launch_attn_full(const AttnFull& a, hipStream_t st) {
    if (a.T % 4 || a.T < 1 || (a.DK != 64 && a.DK != 32)) return hipErrorInvalidValue;
    const size_t lds = attn_full_lds_bytes(a.T);
    if (lds > 160 * 1024 || a.T > a.R) return hipErrorInvalidValue;
    AttnFullArgs k{a.qkv, a.ptab, a.bias_u, a.bias_v, a.lens, a.bidir, a.ctx, a.causal, a.H, a.T, a.R, a.PR, attn_sw(a.T)};
    const dim3 grid(ceil_div_h(a.T, 16), a.H, a.B);
    static std::atomic<unsigned long long> d64{0ull}, d32{0ull};
    hipError_t e;
    if (a.DK == 64) {
        if ((e = big_lds(attn_full_kernel<64>, d64)) != hipSuccess) return e;
        hipLaunchKernelGGL(attn_full_kernel<64>, grid, dim3(256), lds, st, k);
    } else {
        if ((e = big_lds(attn_full_kernel<32>, d32)) != hipSuccess) return e;
        hipLaunchKernelGGL(attn_full_kernel<32>, grid, dim3(256), lds, st, k);
    }
    return hipGetLastError();
}

// =====================================================================================================================
// layout changes and input assembly (all HBM-bound elementwise work)
// =====================================================================================================================
__global__ __launch_bounds__(256) void tm_to_fm_kernel(const float* __restrict__ in, const int* __restrict__ lens, int L, int D, int T,
                                                       float* __restrict__ out) {
    // 32 x 32 tile transpose through LDS: read rows of D (coalesced over d), write rows of T (coalesced over t)
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = lens ? lens[b] : L;
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, d = d0 + tx;
        tile[r][tx] = (t < len && t < L && d < D) ? in[((size_t)b * L + t) * D + d] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int d = d0 + r, t = t0 + tx;
        if (d < D && t < T) out[((size_t)b * D + d) * T + t] = tile[tx][r];
    }
}
hipError_t launch_tm_to_fm(const float* in, const int* lens, int B, int L, int D, int T, float* out, hipStream_t st) {
    hipLaunchKernelGGL(tm_to_fm_kernel, dim3(ceil_div_h(T, 32), ceil_div_h(D, 32), B), dim3(256), 0, st, in, lens, L, D, T, out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void fm_to_tm_kernel(const float* __restrict__ in, const int* __restrict__ lens, int D, int T, int L,
                                                       float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = lens ? lens[b] : L;
    for (int r = ty; r < 32; r += 8) {
        const int d = d0 + r, t = t0 + tx;
        tile[r][tx] = (d < D && t < T && t < len) ? in[((size_t)b * D + d) * T + t] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, d = d0 + tx;
        if (t < L && d < D) out[((size_t)b * L + t) * D + d] = tile[tx][r];
    }
}
hipError_t launch_fm_to_tm(const float* in, const int* lens, int B, int D, int T, int L, float* out, hipStream_t st) {
    hipLaunchKernelGGL(fm_to_tm_kernel, dim3(ceil_div_h(L, 32), ceil_div_h(D, 32), B), dim3(256), 0, st, in, lens, D, T, L, out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void token_embed_fm_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table, int vocab,
                                                             int L, int D, int T, float* __restrict__ out) {
    const int b = blockIdx.z, t = blockIdx.x * 64 + (threadIdx.x & 63);
    if (t >= T) return;
    long long id = t < L ? ids[(size_t)b * L + t] : -1;
    if (id >= vocab) id = -1;
    for (int d = blockIdx.y * 4 + (threadIdx.x >> 6); d < D; d += gridDim.y * 4)
        out[((size_t)b * D + d) * T + t] = id >= 0 ? table[(size_t)id * D + d] : 0.f;
}
hipError_t launch_token_embed_fm(const int64_t* ids, const float* table, int vocab, int B, int L, int D, int T, float* out,
                                 hipStream_t st) {
    hipLaunchKernelGGL(token_embed_fm_kernel, dim3(ceil_div_h(T, 64), 8, B), dim3(256), 0, st, ids, table, vocab, L, D, T, out);
    return hipGetLastError();
}

__device__ __forceinline__ float codebook_sum(const float* cb, int K, int D, int nq, const int64_t* tok, int stride, int d) {
    // sum over the groups in group order (QuantizerCodebook.forward, laura_model.py:51-53; cal_codec_emb :303-310)
    float s = 0.f;
    for (int k = 0; k < nq; ++k) {
        long long c = tok[k * stride];
        c = c < 0 ? 0 : (c >= K ? K - 1 : c);
        const float v = cb[((size_t)k * K + c) * D + d];
        s = k == 0 ? v : s + v;
    }
    return s;
}

__global__ __launch_bounds__(256) void lm_assemble_kernel(const float* __restrict__ text_fm, int Tt, const int* __restrict__ text_lens,
                                                          const float* __restrict__ lm_emb, const float* __restrict__ cb, int K, int nq,
                                                          const int64_t* __restrict__ codec, const int* __restrict__ codec_lens, int Cmax,
                                                          int D, int T, float* __restrict__ out, int* seq_len, int* bidir_len) {
    const int b = blockIdx.z, t = blockIdx.x * 64 + (threadIdx.x & 63);
    const int tl = text_lens[b], cl = (codec && codec_lens) ? codec_lens[b] : 0;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        seq_len[b] = tl + 2 + cl;
        if (bidir_len) bidir_len[b] = tl + 1;          // <sos> + text (transformer_lm.py:286-288)
    }
    if (t >= T) return;
    for (int d = blockIdx.y * 4 + (threadIdx.x >> 6); d < D; d += gridDim.y * 4) {
        float v = 0.f;
        if (t == 0) v = lm_emb[d];                                         // sos_eos = 0
        else if (t <= tl) v = text_fm[((size_t)b * D + d) * Tt + (t - 1)];
        else if (t == tl + 1) v = lm_emb[D + d];                           // task_id = 1
        else if (t < tl + 2 + cl) v = codebook_sum(cb, K, D, nq, codec + ((size_t)b * Cmax + (t - tl - 2)) * nq, 1, d);
        out[((size_t)b * D + d) * T + t] = v;
    }
}
hipError_t launch_lm_assemble(const float* text_fm, int Tt, const int* text_lens, const float* lm_emb, const float* cb, int K, int nq,
                              const int64_t* codec, const int* codec_lens, int Cmax, int B, int D, int T, float* out, int* seq_len,
                              int* bidir_len, hipStream_t st) {
    hipLaunchKernelGGL(lm_assemble_kernel, dim3(ceil_div_h(T, 64), 8, B), dim3(256), 0, st, text_fm, Tt, text_lens, lm_emb, cb, K, nq,
                       codec, codec_lens, Cmax, D, T, out, seq_len, bidir_len);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void nar_assemble_kernel(const float* __restrict__ text_fm, int Tt, const int* __restrict__ text_lens,
                                                           const float* __restrict__ cb, int K, int nq, const int64_t* __restrict__ codec,
                                                           const int* __restrict__ codec_lens, int Cmax, int cstride,
                                                           const float* __restrict__ pe_abs, int split, int D, int T,
                                                           float* __restrict__ out, int* seq_len) {
    const int b = blockIdx.z, t = blockIdx.x * 64 + (threadIdx.x & 63);
    const int tl = text_lens[b], cl = codec_lens[b];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) seq_len[b] = tl + cl;
    if (t >= T) return;
    const float xs = sqrtf((float)D);
    for (int d = blockIdx.y * 4 + (threadIdx.x >> 6); d < D; d += gridDim.y * 4) {
        float v = 0.f;
        if (t < tl) {
            v = text_fm[((size_t)b * D + d) * Tt + t];
            if (split) v = v * xs + pe_abs[(size_t)t * D + d];              // PositionalEncoding.forward (embedding.py:79-91)
        } else if (t < tl + cl) {
            v = codebook_sum(cb, K, D, nq, codec + ((size_t)b * Cmax + (t - tl)) * cstride, 1, d);
            if (split) v = v * xs + pe_abs[(size_t)(t - tl) * D + d];
        }
        out[((size_t)b * D + d) * T + t] = v;
    }
}
hipError_t launch_nar_assemble(const float* text_fm, int Tt, const int* text_lens, const float* cb, int K, int nq, const int64_t* codec,
                               const int* codec_lens, int Cmax, int codec_stride_nq, const float* pe_abs, int split, int B, int D, int T,
                               float* out, int* seq_len, hipStream_t st) {
    hipLaunchKernelGGL(nar_assemble_kernel, dim3(ceil_div_h(T, 64), 8, B), dim3(256), 0, st, text_fm, Tt, text_lens, cb, K, nq, codec,
                       codec_lens, Cmax, codec_stride_nq, pe_abs, split, D, T, out, seq_len);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void nar_extract_kernel(const float* __restrict__ in, const int* __restrict__ text_lens,
                                                          const int* __restrict__ codec_lens, int D, int T, int Cmax,
                                                          float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int tl = text_lens[b], cl = codec_lens[b];
    for (int r = ty; r < 32; r += 8) {
        const int d = d0 + r, c = c0 + tx, t = tl + c;
        tile[r][tx] = (d < D && c < cl && t < T) ? in[((size_t)b * D + d) * T + t] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, d = d0 + tx;
        if (c < Cmax && d < D) out[((size_t)b * Cmax + c) * D + d] = tile[tx][r];
    }
}
hipError_t launch_nar_extract(const float* in, const int* text_lens, const int* codec_lens, int B, int D, int T, int Cmax, float* out,
                              hipStream_t st) {
    hipLaunchKernelGGL(nar_extract_kernel, dim3(ceil_div_h(Cmax, 32), ceil_div_h(D, 32), B), dim3(256), 0, st, in, text_lens, codec_lens,
                       D, T, Cmax, out);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void logsoftmax_fm_kernel(const float* __restrict__ in, const int* __restrict__ lens, int V, int T, int L,
                                                           float* __restrict__ out) {
    const int b = blockIdx.y, t = blockIdx.x * 64 + threadIdx.x;
    if (t >= L) return;
    float* o = out + ((size_t)b * L + t) * V;
    if (t >= lens[b] || t >= T) {
        for (int v = 0; v < V; ++v) o[v] = 0.f;
        return;
    }
    const float* x = in + (size_t)b * V * T + t;
    float m = -INFINITY;
    for (int v = 0; v < V; ++v) m = fmaxf(m, x[(size_t)v * T]);
    float s = 0.f;
    for (int v = 0; v < V; ++v) s += expf(x[(size_t)v * T] - m);
    const float ls = logf(s);
    for (int v = 0; v < V; ++v) o[v] = (x[(size_t)v * T] - m) - ls;
}
hipError_t launch_logsoftmax_fm(const float* in, const int* lens, int B, int V, int T, int L, float* out, hipStream_t st) {
    hipLaunchKernelGGL(logsoftmax_fm_kernel, dim3(ceil_div_h(L, 64), B), dim3(64), 0, st, in, lens, V, T, L, out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void kv_store_kernel(const float* __restrict__ qkv, const int* __restrict__ lens, int d, int T, int Tcap,
                                                       float* __restrict__ kc, float* __restrict__ vc) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = lens[b];
    const float* kb = qkv + ((size_t)b * 3 + 1) * d * T;
    const float* vb = qkv + ((size_t)b * 3 + 2) * d * T;
    for (int r = ty; r < 32; r += 8) {
        const int n = n0 + r, t = t0 + tx;
        const bool ok = n < d && t < len && t < T;
        if (ok) kc[((size_t)b * d + n) * Tcap + t] = kb[(size_t)n * T + t];
        tile[r][tx] = ok ? vb[(size_t)n * T + t] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, n = n0 + tx;
        if (t < len && t < T && n < d) vc[((size_t)b * Tcap + t) * d + n] = tile[tx][r];
    }
}
hipError_t launch_kv_store(const float* qkv, const int* lens, int B, int d, int T, int Tcap, float* kc, float* vc, hipStream_t st) {
    hipLaunchKernelGGL(kv_store_kernel, dim3(ceil_div_h(T, 32), ceil_div_h(d, 32), B), dim3(256), 0, st, qkv, lens, d, T, Tcap, kc, vc);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void gather_last_kernel(const float* __restrict__ x, const int* __restrict__ lens, int C, int T,
                                                          float* __restrict__ out) {
    const int b = blockIdx.x;
    const int t = lens[b] - 1;
    for (int c = threadIdx.x; c < C; c += 256) out[(size_t)b * C + c] = x[((size_t)b * C + c) * T + (t < 0 ? 0 : t)];
}
hipError_t launch_gather_last(const float* x, const int* lens, int B, int C, int T, float* out, hipStream_t st) {
    hipLaunchKernelGGL(gather_last_kernel, dim3(B), dim3(256), 0, st, x, lens, C, T, out);
    return hipGetLastError();
}

// kv_store_kernel for a prefix pass of several prompts of a decoding session: batch row b goes to the session's slot rs.slot[b].  The
// values are copied, so a slot's cache positions are those of the one-row pass whatever the other rows hold.
__global__ __launch_bounds__(256) void kv_store_slots_kernel(const float* __restrict__ qkv, const int* __restrict__ lens, RowSlots rs, int d,
                                                             int T, int Tcap, float* __restrict__ kc, float* __restrict__ vc) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = lens[b] < Tcap ? lens[b] : Tcap;
    const size_t slot = (size_t)rs.slot[b];
    const float* kb = qkv + ((size_t)b * 3 + 1) * d * T;
    const float* vb = qkv + ((size_t)b * 3 + 2) * d * T;
    for (int r = ty; r < 32; r += 8) {
        const int n = n0 + r, t = t0 + tx;
        const bool ok = n < d && t < len && t < T;
        if (ok) kc[(slot * d + n) * Tcap + t] = kb[(size_t)n * T + t];
        tile[r][tx] = ok ? vb[(size_t)n * T + t] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, n = n0 + tx;
        if (t < len && t < T && n < d) vc[(slot * Tcap + t) * d + n] = tile[tx][r];
    }
}
static bool row_slots_ok(const RowSlots& rs, int S) {
    if (rs.n < 1 || rs.n > 16 || S < 1) return false;
    for (int i = 0; i < rs.n; ++i) {
        if (rs.slot[i] < 0 || rs.slot[i] >= S) return false;
        for (int j = 0; j < i; ++j)
            if (rs.slot[j] == rs.slot[i]) return false;
    }
    return true;
}
hipError_t launch_kv_store_slots(const float* qkv, const int* lens, const RowSlots& rs, int S, int d, int T, int Tcap, float* kc, float* vc,
                                 hipStream_t st) {
    if (!row_slots_ok(rs, S) || d < 1 || T < 1 || Tcap < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kv_store_slots_kernel, dim3(ceil_div_h(T, 32), ceil_div_h(d, 32), rs.n), dim3(256), 0, st, qkv, lens, rs, d, T, Tcap,
                       kc, vc);
    return hipGetLastError();
}

// gather_last_kernel with a destination slot per batch row, and the row's length as the slot's cache fill
__global__ __launch_bounds__(256) void gather_last_slots_kernel(const float* __restrict__ x, const int* __restrict__ lens, RowSlots rs, int C,
                                                                int T, float* __restrict__ xs, int* __restrict__ pos) {
    const int b = blockIdx.x;
    const size_t slot = (size_t)rs.slot[b];
    int t = lens[b] - 1;
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    for (int c = threadIdx.x; c < C; c += 256) xs[slot * C + c] = x[((size_t)b * C + c) * T + t];
    if (threadIdx.x == 0) pos[slot] = lens[b];
}
hipError_t launch_gather_last_slots(const float* x, const int* lens, const RowSlots& rs, int S, int C, int T, float* xs, int* pos,
                                    hipStream_t st) {
    if (!row_slots_ok(rs, S) || C < 1 || T < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_last_slots_kernel, dim3(rs.n), dim3(256), 0, st, x, lens, rs, C, T, xs, pos);
    return hipGetLastError();
}

__global__ void fill_i32_kernel(int* p, int v, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) p[i] = v;
}
hipError_t launch_fill_i32(int* p, int v, int n, hipStream_t st) {
    hipLaunchKernelGGL(fill_i32_kernel, dim3(ceil_div_h(n, 64)), dim3(64), 0, st, p, v, n);
    return hipGetLastError();
}

// =====================================================================================================================
// STEP FORM.  Weight-streaming GEMV for B <= 64 new tokens, 16 per column block: y[b][n] = f(sum_k W[n][k] g(x)[b][k] + bias[n]).
//   workgroup = one 16-row tile of W, KS waves splitting K; W in fragment order [tile][K/16][lane][4]: every wave load is one
//   contiguous 1 KiB, all loads of a wave's K range issued before its MFMAs; x (optionally LayerNorm'ed) staged in LDS as the
//   B operand (batch = the 16 MFMA columns, rows >= B read a zero row); partial tiles reduced across the waves in wave order
//   (deterministic), then bias / activation / residual add / cache scatter.
// =====================================================================================================================
struct GemvArgs {
    const float *x, *wf, *bias, *gamma, *beta;
    float eps;
    int act, mode;
    float* y;
    int ldy;
    float *kc, *vc;
    const int* pos;
    int d, Tcap, B, K, N, XS;       // XS = LDS row stride of x
    const float* apart;             // attention partials [B][H][NS][DK + 2] (x is then their combination), or null
    int H, DK, NS;
    int ablate;                     // FC_GEMV_ABLATE (tuning aid): 1 no x loads, 2 no weight loads, 4 no LayerNorm, 8 no MFMAs
    int W, NW;                      // gemv_win_kernel: x staged in NW windows of W columns (XS = W + 4)
};

// Rows beyond 16: a workgroup's rows are those of COLUMN BLOCK blockIdx.y, rows 16 j .. min(B, 16 j + 16) - 1, and the kernels below see
// that block alone: everything indexed by row (x, y, pos, the K / V cache slot of mode 2, the attention partials) starts at the block's
// first row and B is the block's row count.  The tile stays on blockIdx.x, the fast index.  EXPECTED, from the dispatch order and not
// measured (no counter run): workgroups go round-robin over the 8 XCDs by linear id, so the blocks of one tile meet on one XCD whenever
// the tile count is a multiple of 8, and the tile's weight fragments are re-read from that XCD's L2.  Up to 16 rows (grid.y = 1) the
// launcher takes the instantiations with WIDE = false, which do not have this prologue at all: the kernels of 16 columns.
__device__ __forceinline__ void gemv_column_block(GemvArgs& a) {
    const int j = blockIdx.y;
    if (j == 0) { a.B = a.B < 16 ? a.B : 16; return; }
    const size_t r0 = (size_t)16 * j;
    a.B = a.B - 16 * j < 16 ? a.B - 16 * j : 16;
    if (a.x) a.x += r0 * a.K;
    a.y += r0 * a.ldy;
    if (a.mode == 2) {
        a.pos += r0;
        a.kc += r0 * a.d * a.Tcap;
        a.vc += r0 * a.Tcap * a.d;
    }
    if (a.apart) a.apart += r0 * a.H * a.NS * (a.DK + 2);
}

// CPW = 16-wide k chunks per wave as a compile-time constant (2 or 8 for every layer of the recipe): the weight loads are then
// unconditional straight-line code.  Under a run-time count every load sat behind its own `if`, and hipcc waits for a conditional
// load right where it is issued (DESIGN.md §5, round-2 finding) -- the "prefetch" was eight serialised round trips.  CPW = 0: generic.
template <int KS, int CPW, bool WIDE>
__global__ __launch_bounds__(64 * KS) void gemv_kernel(GemvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if constexpr (WIDE) gemv_column_block(a);
    float* Xs = lds;                                   // [B + 1][XS], row B = zeros
    float* red = lds + (a.B + 1) * a.XS;               // [KS][64][4]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, r16 = lane & 15;
    const int K = a.K, B = a.B, XS = a.XS;
    const int tile = blockIdx.x;
    const int nch = K / 16;                            // 16-wide k chunks of the row
    const int cpw = CPW ? CPW : nch / KS;              // chunks per wave
    // the weight fragments do not depend on x: request them first, the staging / LayerNorm of x runs under their latency
    const float* wp = a.wf + ((size_t)tile * nch + (size_t)w * cpw) * 256 + lane * 4;
    constexpr int NPRE = CPW ? CPW : 1;
    f32x4 wv[CPW ? CPW : 8];
#pragma unroll
    for (int u = 0; u < NPRE; ++u) wv[u] = (a.ablate & 2) ? (f32x4){1.f, 1.f, 1.f, 1.f} : *(const f32x4*)(wp + (size_t)u * 256);
    // epilogue operands (bias, the residual row for mode 1, the cache position for mode 2) requested NOW: fetched at the end of the kernel
    // they are two serial memory round trips with nothing left to overlap them (measured: ~1.5 us of an 8 us kernel)
    const int eb = r16 < B ? r16 : 0, en0 = tile * 16 + 4 * g;
    float ebias[4], eold[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = en0 + r < a.N ? en0 + r : a.N - 1;
        ebias[r] = a.bias[n];
        eold[r] = a.mode == 1 ? a.y[(size_t)eb * a.ldy + n] : 0.f;
    }
    const int epos = a.mode == 2 ? a.pos[eb] : 0;
    if (a.apart) {
        // x[b][h * DK + dd] = combination of the NS key-range partials of head h (flash-decoding): o_s, running max m_s, sum l_s.
        // First the B * H * NS normalised weights exp(m_s - M) / L (one thread per (b, h)), in LDS of their own: B * H * 8 floats do not
        // fit the reduction scratch at every accepted width (d_model 320 with 10 heads: KS = 4, 1024 floats, 16 rows need 1280)
        const int PS = a.DK + 2;
        float* wn = red + KS * 256;                    // [B * H][8], behind the reduction scratch (gemv_lds_bytes)
        // NS <= 8 key ranges; every loop below runs its 8 trips with clamped indices so that the loads are unconditional and
        // independent (a run-time trip count made each partial its own serialised round trip: 11 us instead of 5 for this kernel)
        for (int e = tid; e < B * a.H; e += 64 * KS) {
            const float* pp = a.apart + (size_t)e * a.NS * PS;
            float mv[8], lv[8];
#pragma unroll
            for (int sp = 0; sp < 8; ++sp) {
                const int sc = sp < a.NS ? sp : a.NS - 1;
                mv[sp] = pp[sc * PS + a.DK];
                lv[sp] = pp[sc * PS + a.DK + 1];
            }
            float M = -INFINITY;
#pragma unroll
            for (int sp = 0; sp < 8; ++sp) M = fmaxf(M, sp < a.NS ? mv[sp] : -INFINITY);
            float L = 0.f, wg[8];
#pragma unroll
            for (int sp = 0; sp < 8; ++sp) {
                wg[sp] = sp < a.NS ? expf(mv[sp] - M) : 0.f;
                L = fmaf(lv[sp], wg[sp], L);
            }
            const float inv = 1.f / L;
#pragma unroll
            for (int sp = 0; sp < 8; ++sp) wn[e * 8 + sp] = wg[sp] * inv;
        }
        __syncthreads();
        for (int e = tid; e < B * K; e += 64 * KS) {
            const int b = e / K, k = e - b * K, h = k / a.DK, dd = k - h * a.DK;
            const float* pp = a.apart + ((size_t)(b * a.H + h) * a.NS) * PS + dd;
            const float* wq = wn + (b * a.H + h) * 8;
            float ov[8];
#pragma unroll
            for (int sp = 0; sp < 8; ++sp) ov[sp] = pp[(sp < a.NS ? sp : a.NS - 1) * PS];
            float o = 0.f;
#pragma unroll
            for (int sp = 0; sp < 8; ++sp) o = fmaf(ov[sp], wq[sp], o);        // weights of ranges >= NS are 0
            Xs[b * XS + k] = o;
        }
        for (int k = tid; k < K; k += 64 * KS) Xs[B * XS + k] = 0.f;
    } else {
        for (int e = tid * 4; e < (B + 1) * K; e += 64 * KS * 4) {
            const int b = e / K, k = e - b * K;
            f32x4 v = (a.ablate & 1) ? (f32x4){1.f, 0.f, 1.f, 0.f} : *(const f32x4*)(a.x + (size_t)(b < B ? b : B - 1) * K + k);      // unconditional load, the zero row by select
            if (b >= B) v = (f32x4){0.f, 0.f, 0.f, 0.f};
            *(f32x4*)(Xs + b * XS + k) = v;
        }
    }
    __syncthreads();
    if (a.gamma && !(a.ablate & 4)) {       // LayerNorm of every row, two-pass in LDS (one wave per row at a time)
        for (int b = w; b < B; b += KS) {
            float* xr = Xs + b * XS;
            float s = 0.f;
            for (int k = lane; k < K; k += 64) s += xr[k];
            const float mean = wave_sum(s) / (float)K;
            float q = 0.f;
            for (int k = lane; k < K; k += 64) { const float dv = xr[k] - mean; q += dv * dv; }
            const float rstd = 1.f / sqrtf(wave_sum(q) / (float)K + a.eps);
            for (int k = lane; k < K; k += 64) xr[k] = (xr[k] - mean) * rstd * a.gamma[k] + a.beta[k];
        }
        __syncthreads();
    }
    const float* xb = Xs + (r16 < B ? r16 : B) * XS + w * cpw * 16 + 4 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NPRE; ++u) {
        const f32x4 xv = *(const f32x4*)(xb + u * 16);
        if (a.ablate & 8) { acc += wv[u] * xv[0]; continue; }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u][j], xv[j], acc, 0, 0, 0);
    }
    for (int c0 = NPRE; c0 < cpw; c0 += 8) {           // generic form: the remaining chunks in batches of up to 8
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (c0 + u < cpw) wv[u] = *(const f32x4*)(wp + (size_t)(c0 + u) * 256);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (c0 + u < cpw) {
                const f32x4 xv = *(const f32x4*)(xb + (c0 + u) * 16);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u][j], xv[j], acc, 0, 0, 0);
            }
    }
    *(f32x4*)(red + (w * 64 + lane) * 4) = acc;
    __syncthreads();
    if (w != 0) return;
    f32x4 s = *(const f32x4*)(red + lane * 4);
    for (int u = 1; u < KS; ++u) s += *(const f32x4*)(red + (u * 64 + lane) * 4);
    const int b = r16;
    if (b >= B) return;
    const int p = epos;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = tile * 16 + 4 * g + r;
        if (n >= a.N) continue;
        float v = act_f(s[r] + ebias[r], a.act);
        if (a.mode == 0) a.y[(size_t)b * a.ldy + n] = v;
        else if (a.mode == 1) a.y[(size_t)b * a.ldy + n] = eold[r] + v;
        else {
            if (n < a.d) a.y[(size_t)b * a.ldy + n] = v;
            else if (n < 2 * a.d) a.kc[((size_t)b * a.d + (n - a.d)) * a.Tcap + p] = v;
            else a.vc[((size_t)b * a.Tcap + p) * a.d + (n - 2 * a.d)] = v;
        }
    }
}

// K beyond one LDS stage (w_2 at ff = 4096: 17 x 4100 floats would be 279 KB): x is staged in NW windows of W columns, one after the
// other through the same LDS rows, and the MFMA chain runs over each window into the same accumulators.  Wave w owns CPW chunks of
// EVERY window (chunks s * W/16 + w * CPW + u), so all waves have MFMA work between every pair of window barriers.  Specialised form
// (CPW, NW compile-time; the music recipe's w_2 is <16, 4, 4>): all NW * CPW weight loads of a wave issued up front, before any
// barrier (a plain global load survives __syncthreads), and the next window's x requested into registers (a fixed trip count with
// clamped addresses: unconditional loads) while the current one is multiplied.  CPW = 0: generic, loads per window.
// x as given (no LayerNorm, no attention partials: both need whole rows); modes 0 and 1.
template <int KS, int CPW, int NW, bool WIDE>
__global__ __launch_bounds__(64 * KS) void gemv_win_kernel(GemvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if constexpr (WIDE) gemv_column_block(a);
    float* Xs = lds;                                   // [B + 1][XS]: the current window, row B = zeros
    float* red = lds + (a.B + 1) * a.XS;               // [KS][64][4]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, r16 = lane & 15;
    const int K = a.K, B = a.B, XS = a.XS, W = a.W;
    const int nw = NW ? NW : a.NW;
    const int tile = blockIdx.x;
    const int nch = K / 16, cw = W / 16;               // 16-wide k chunks of the row / of a window
    const int cpw = CPW ? CPW : cw / KS;               // chunks per wave per window
    const float* wp = a.wf + ((size_t)tile * nch + (size_t)w * cpw) * 256 + lane * 4;
    constexpr int NWV = CPW ? CPW * NW : 8;
    f32x4 wv[NWV];
    if constexpr (CPW > 0) {
#pragma unroll
        for (int s = 0; s < NW; ++s)
#pragma unroll
            for (int u = 0; u < CPW; ++u) wv[s * CPW + u] = *(const f32x4*)(wp + ((size_t)s * cw + u) * 256);
    }
    const int eb = r16 < B ? r16 : 0, en0 = tile * 16 + 4 * g;
    float ebias[4], eold[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = en0 + r < a.N ? en0 + r : a.N - 1;
        ebias[r] = a.bias[n];
        eold[r] = a.mode == 1 ? a.y[(size_t)eb * a.ldy + n] : 0.f;
    }
    const int lim = (B + 1) * W;                       // floats of one staged window
    // specialised: x of one window in NXT f32x4 per thread (17 rows at most)
    constexpr int NXT = CPW ? (17 * CPW + 15) / 16 : 1;
    f32x4 xr[NXT];
    auto request_x = [&](int s) {
#pragma unroll
        for (int i = 0; i < NXT; ++i) {
            int e = (tid + i * 64 * KS) * 4;
            e = e < lim ? e : lim - 4;
            const int b = e / W, k = e - b * W;
            xr[i] = *(const f32x4*)(a.x + (size_t)(b < B ? b : B - 1) * K + (size_t)s * W + k);
        }
    };
    if constexpr (CPW > 0) request_x(0);
    const float* xb = Xs + (r16 < B ? r16 : B) * XS + w * cpw * 16 + 4 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < nw; ++s) {
        if (s) __syncthreads();                        // every wave is done with the previous window
        if constexpr (CPW > 0) {
#pragma unroll
            for (int i = 0; i < NXT; ++i) {
                const int e = (tid + i * 64 * KS) * 4;
                if (e < lim) *(f32x4*)(Xs + (e / W) * XS + e % W) = e / W < B ? xr[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        } else {
            for (int e = tid * 4; e < lim; e += 64 * KS * 4) {
                const int b = e / W, k = e - b * W;
                f32x4 v = *(const f32x4*)(a.x + (size_t)(b < B ? b : B - 1) * K + (size_t)s * W + k);
                if (b >= B) v = (f32x4){0.f, 0.f, 0.f, 0.f};
                *(f32x4*)(Xs + b * XS + k) = v;
            }
        }
        __syncthreads();
        if constexpr (CPW > 0) {
            if (s + 1 < nw) request_x(s + 1);          // lands under this window's MFMAs
#pragma unroll
            for (int u = 0; u < CPW; ++u) {
                const f32x4 xv = *(const f32x4*)(xb + u * 16);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s * CPW + u][j], xv[j], acc, 0, 0, 0);
            }
        } else {
            const float* ws = wp + (size_t)s * cw * 256;
            for (int c0 = 0; c0 < cpw; c0 += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (c0 + u < cpw) wv[u] = *(const f32x4*)(ws + (size_t)(c0 + u) * 256);
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (c0 + u < cpw) {
                        const f32x4 xv = *(const f32x4*)(xb + (c0 + u) * 16);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u][j], xv[j], acc, 0, 0, 0);
                    }
            }
        }
    }
    *(f32x4*)(red + (w * 64 + lane) * 4) = acc;
    __syncthreads();
    if (w != 0) return;
    f32x4 sum = *(const f32x4*)(red + lane * 4);
    for (int u = 1; u < KS; ++u) sum += *(const f32x4*)(red + (u * 64 + lane) * 4);
    const int b = r16;
    if (b >= B) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = tile * 16 + 4 * g + r;
        if (n >= a.N) continue;
        const float v = act_f(sum[r] + ebias[r], a.act);
        a.y[(size_t)b * a.ldy + n] = a.mode == 1 ? eold[r] + v : v;
    }
}

namespace {
// x rows + the zero row, the reduction scratch, and with attention partials (heads > 0) the 8 range weights of every (row, head)
size_t gemv_lds_bytes(int B, int XS, int KS, int heads = 0) {
    return ((size_t)(B + 1) * XS + (size_t)KS * 256 + (size_t)B * heads * 8) * sizeof(float);
}

hipError_t launch_gemv_windowed(const Gemv& g, GemvArgs a, int KS, dim3 grid, hipStream_t st) {
    if (g.gamma || g.apart || g.mode == 2) return hipErrorInvalidValue;       // whole-row prologues / the cache scatter: K <= d
    // the fewest windows of <= 1024 columns that split every wave's chunks evenly (stage 2, test hook: at least two windows)
    const int cpw = g.K / 16 / KS, wmax = g.stage == 2 ? g.K : 1024;
    const int rows = g.B < 16 ? g.B : 16;                  // of a column block: the LDS stage never holds more
    int nw = 0;
    for (int n = g.stage == 2 ? 2 : 1; n <= cpw && !nw; ++n)
        if (cpw % n == 0 && g.K / n <= wmax && gemv_lds_bytes(rows, g.K / n + 4, KS) <= 160 * 1024) nw = n;
    if (!nw) return hipErrorInvalidValue;
    a.W = g.K / nw; a.NW = nw; a.XS = a.W + 4;
    const size_t lds = gemv_lds_bytes(rows, a.XS, KS);
    static std::atomic<unsigned long long> d_spec[2], d_gen[5][2];       // per kernel: [0] the 16-column form, [1] over column blocks
    const bool wide = grid.y > 1 || g.wide;
    hipError_t e;
#define FC_GEMV_WIN_LAUNCH(ks, cpwc, nwc, flag)                                                              \
    do {                                                                                                     \
        if (wide) {                                                                                          \
            if ((e = big_lds(gemv_win_kernel<ks, cpwc, nwc, true>, flag[1])) != hipSuccess) return e;        \
            hipLaunchKernelGGL((gemv_win_kernel<ks, cpwc, nwc, true>), grid, dim3(64 * ks), lds, st, a);     \
        } else {                                                                                             \
            if ((e = big_lds(gemv_win_kernel<ks, cpwc, nwc, false>, flag[0])) != hipSuccess) return e;       \
            hipLaunchKernelGGL((gemv_win_kernel<ks, cpwc, nwc, false>), grid, dim3(64 * ks), lds, st, a);    \
        }                                                                                                    \
        return hipGetLastError();                                                                            \
    } while (0)
    if (KS == 16 && cpw / nw == 4 && nw == 4) FC_GEMV_WIN_LAUNCH(16, 4, 4, d_spec);
#define FC_GEMV_WIN_CASE(ks, i) \
    if (KS == ks) FC_GEMV_WIN_LAUNCH(ks, 0, 0, d_gen[i]);
    FC_GEMV_WIN_CASE(16, 0)
    FC_GEMV_WIN_CASE(8, 1)
    FC_GEMV_WIN_CASE(4, 2)
    FC_GEMV_WIN_CASE(2, 3)
    FC_GEMV_WIN_CASE(1, 4)
#undef FC_GEMV_WIN_CASE
#undef FC_GEMV_WIN_LAUNCH
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t launch_gemv(const Gemv& g, hipStream_t st) {
    if (g.B < 1 || g.B > 64 || g.K % 16 || g.K < 16) return hipErrorInvalidValue;
    const int nch = g.K / 16;
    const int rows = g.B < 16 ? g.B : 16;                  // of a column block (gemv_column_block): what the LDS stage holds
    static const int ks_cap = fc::ab_knob("FC_GEMV_KS", 16);     // tuning aid: waves per workgroup
    int KS = ks_cap >= 1 && ks_cap <= 16 ? ks_cap : 16;
    while (KS > 1 && (nch % KS || nch / KS < 2)) KS >>= 1;     // >= 2 chunks per wave, K split evenly
    if (nch % KS) KS = 1;
    GemvArgs a{g.x, g.wf, g.bias, g.gamma, g.beta, g.eps, g.act, g.mode, g.y, g.ldy, g.kc, g.vc, g.pos, g.d, g.Tcap, g.B, g.K, g.N, g.K + 4,
               g.apart, g.H, g.DK, g.NS, 0, 0, 0};
    static const int ablate = fc::ab_knob("FC_GEMV_ABLATE", 0);
    a.ablate = ablate;
    if (g.apart && (g.H * g.DK != g.K || g.NS < 1 || g.NS > 8)) return hipErrorInvalidValue;
    const int wn_heads = g.apart ? g.H : 0;
    const dim3 grid(ceil_div_h(g.N, 16), ceil_div_h(g.B, 16));      // tile x column block
    // one LDS stage whenever it fits at the largest batch (every K <= 2112: the path does not depend on B), windows beyond that
    const bool one_stage = g.stage == 1 || (g.stage == 0 && gemv_lds_bytes(16, g.K + 4, KS, wn_heads) <= 160 * 1024);
    if (!one_stage) return launch_gemv_windowed(g, a, KS, grid, st);
    const size_t lds = gemv_lds_bytes(rows, a.XS, KS, wn_heads);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> d16[6][2], d8[6][2], d4[6][2], d2[6][2], d1[6][2];     // [.][1]: over column blocks
    const bool wide = grid.y > 1 || g.wide;
    hipError_t e;
#define FC_GEMV_LAUNCH(ks, cpwc, flag)                                                                  \
    do {                                                                                                \
        if (wide) {                                                                                     \
            if ((e = big_lds(gemv_kernel<ks, cpwc, true>, flag[1])) != hipSuccess) return e;            \
            hipLaunchKernelGGL((gemv_kernel<ks, cpwc, true>), grid, dim3(64 * ks), lds, st, a);         \
        } else {                                                                                        \
            if ((e = big_lds(gemv_kernel<ks, cpwc, false>, flag[0])) != hipSuccess) return e;           \
            hipLaunchKernelGGL((gemv_kernel<ks, cpwc, false>), grid, dim3(64 * ks), lds, st, a);        \
        }                                                                                               \
        return hipGetLastError();                                                                       \
    } while (0)
#define FC_GEMV_CASE(ks, flag)                                \
    if (KS == ks) {                                           \
        const int cpw = nch / ks;                             \
        if (cpw == 2) FC_GEMV_LAUNCH(ks, 2, flag[0]);         \
        else if (cpw == 8) FC_GEMV_LAUNCH(ks, 8, flag[1]);    \
        else if (cpw == 4) FC_GEMV_LAUNCH(ks, 4, flag[3]);    \
        else if (cpw == 16) FC_GEMV_LAUNCH(ks, 16, flag[4]);  \
        else if (cpw == 32) FC_GEMV_LAUNCH(ks, 32, flag[5]);  \
        else FC_GEMV_LAUNCH(ks, 0, flag[2]);                  \
    }
    FC_GEMV_CASE(16, d16)
    FC_GEMV_CASE(8, d8)
    FC_GEMV_CASE(4, d4)
    FC_GEMV_CASE(2, d2)
    FC_GEMV_CASE(1, d1)
#undef FC_GEMV_CASE
#undef FC_GEMV_LAUNCH
    return hipErrorInvalidValue;
}

__global__ __launch_bounds__(64) void layernorm_rows_kernel(float* x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float eps, int relu, float post_scale, int C) {
    float* xr = x + (size_t)blockIdx.x * C;
    const int lane = threadIdx.x;
    float s = 0.f;
    for (int k = lane; k < C; k += 64) s += xr[k];
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int k = lane; k < C; k += 64) { const float dv = xr[k] - mean; q += dv * dv; }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
    for (int k = lane; k < C; k += 64) {
        float o = (xr[k] - mean) * rstd * gamma[k] + beta[k];
        if (relu) o = o > 0.f ? o : 0.f;
        xr[k] = o * post_scale;
    }
}
hipError_t launch_layernorm_rows(float* x, const float* gamma, const float* beta, float eps, int relu, float post_scale, int B, int C,
                                 hipStream_t st) {
    hipLaunchKernelGGL(layernorm_rows_kernel, dim3(B), dim3(64), 0, st, x, gamma, beta, eps, relu, post_scale, C);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Step attention: one query (the newest token) of one (utterance, head) against the KV cache.  K cache feature-major
// [dd][j] (lanes over keys: coalesced), V cache token-major [j][dd] (lanes over dims: coalesced); relative position of key j
// is pos - j >= 0, read backwards from the position table.
// ---------------------------------------------------------------------------------------------------------------------
struct AttnStepArgs {
    const float *q, *kc, *vc, *ptab, *bias_u, *bias_v;
    const int* pos;
    float* part;         // [B][H][NS][DK + 2]: o[DK] (unnormalised), running max, sum of exponentials
    int H, Tcap, R, PR, NS;
};

// One query (the newest token) of one (utterance, head) against ONE key range of the KV cache (flash-decoding split: NS ranges,
// combined by the consumer, gemv_kernel's `apart` prologue).  The kernel is latency-bound, so every load of a thread is an
// independent 16-byte piece and the K / position-table / V loads of the first pass are all in flight together:
//   scores: thread (dg, q) owns DK/8 dims of 4 consecutive keys (K cache rows are key-contiguous; the position table is read
//           backwards: key j sits at column R-1+pos-j); the 8 dim-group partials meet in LDS;
//   context: thread (jg, dq) owns 4 dims of every 16th key (V cache rows are dim-contiguous).
template <int DK>
__global__ __launch_bounds__(256) void attn_step_kernel(AttnStepArgs a) {
    constexpr int DG = 8, DPG = DK / DG;             // dim groups, dims per group
    constexpr int NQ = DK / 4, NG = 256 / NQ;        // dim quads, key groups of the context pass
    constexpr int CH = 128;                          // keys per pass
    __shared__ __attribute__((aligned(16))) float part[DG][CH];
    __shared__ float sc[CH];
    __shared__ float qu[DK], qv[DK];
    __shared__ float wred[4];
    __shared__ __attribute__((aligned(16))) float cred[NG][DK];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, d = a.H * DK;
    const int p = a.pos[b], n = p + 1;
    int chunk = ((n + a.NS - 1) / a.NS + 3) & ~3;    // keys per split, whole quads
    const int k0 = sp * chunk;
    const int k1 = k0 + chunk < n ? k0 + chunk : n;
    float* out = a.part + ((size_t)(b * a.H + h) * a.NS + sp) * (DK + 2);
    if (k0 >= k1) {                                  // empty range: weight 0 in the combination
        if (tid < DK) out[tid] = 0.f;
        if (tid == 0) { out[DK] = -INFINITY; out[DK + 1] = 0.f; }
        return;
    }
    if (tid < DK) {
        const float q = a.q[(size_t)b * d + h * DK + tid];
        qu[tid] = q + a.bias_u[h * DK + tid];
        qv[tid] = q + a.bias_v[h * DK + tid];
    }
    const int dg = tid >> 5, ql = tid & 31;          // scores: dim group, quad of the pass
    const int dq = tid % NQ, jg = tid / NQ;          // context: dim quad, key group
    const float* kb = a.kc + ((size_t)b * d + h * DK + dg * DPG) * a.Tcap;
    const float* pb = a.ptab + (size_t)(h * DK + dg * DPG) * a.PR + (a.R - 1) + p;
    const float* vb = a.vc + (size_t)b * a.Tcap * d + h * DK + 4 * dq;
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 o_acc = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = k0; c0 < k1; c0 += CH) {
        const int cn = k1 - c0 < CH ? k1 - c0 : CH;  // keys of this pass
        // ---- all loads of the pass: K / position rows for the scores, V rows for the context
        const int j0 = c0 + 4 * ql;
        const bool sq = 4 * ql < cn;
        // straight-line loads with clamped addresses: hipcc waits for a load under a run-time condition right where it is issued, which
        // would serialise the round trips this kernel exists to overlap.  Quads / rows past the range read key c0 and are never used.
        const int jq = sq ? j0 : c0;
        f32x4 kv[DPG], pv[DPG];
#pragma unroll
        for (int dd = 0; dd < DPG; ++dd) {
            kv[dd] = *(const f32x4*)(kb + (size_t)dd * a.Tcap + jq);
            pv[dd] = *(const f32x4u*)(pb + (size_t)dd * a.PR - jq - 3);     // columns of keys jq+3, jq+2, jq+1, jq
        }
        constexpr int NV = CH / NG;                  // V rows per thread and pass
        f32x4 vv[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int jj = jg + i * NG;
            vv[i] = *(const f32x4*)(vb + (size_t)(c0 + (jj < cn ? jj : 0)) * d);
        }
        __syncthreads();                             // qu / qv visible (first pass); LDS of the previous pass free
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dd = 0; dd < DPG; ++dd) {
            const float u = qu[dg * DPG + dd], v = qv[dg * DPG + dd];
            acc[0] = fmaf(u, kv[dd][0], fmaf(v, pv[dd][3], acc[0]));
            acc[1] = fmaf(u, kv[dd][1], fmaf(v, pv[dd][2], acc[1]));
            acc[2] = fmaf(u, kv[dd][2], fmaf(v, pv[dd][1], acc[2]));
            acc[3] = fmaf(u, kv[dd][3], fmaf(v, pv[dd][0], acc[3]));
        }
        *(f32x4*)&part[dg][4 * ql] = acc;
        __syncthreads();
        const float scale = 1.f / sqrtf((float)DK);
        float s = -INFINITY;
        if (tid < cn) {
            float t = 0.f;
#pragma unroll
            for (int gq = 0; gq < DG; ++gq) t += part[gq][tid];
            s = t * scale;
        }
        float m = wave_max(s);
        if (lane == 0) wred[w] = m;
        __syncthreads();
        m = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
        const float m_new = fmaxf(m_run, m);
        const float e = tid < cn ? expf(s - m_new) : 0.f;
        if (tid < CH) sc[tid] = e;
        float l = wave_sum(e);
        __syncthreads();                             // wred read by all; sc written
        if (lane == 0) wred[w] = l;
        __syncthreads();
        const float corr = expf(m_run - m_new);      // 0 on the first pass (m_run = -inf)
        l_run = l_run * corr + (wred[0] + wred[1] + wred[2] + wred[3]);
        m_run = m_new;
        o_acc *= corr;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int jj = jg + i * NG;
            if (jj < cn) o_acc += sc[jj] * vv[i];
        }
    }
    *(f32x4*)&cred[jg][4 * dq] = o_acc;
    __syncthreads();
    if (tid < DK) {
        float o = 0.f;
#pragma unroll
        for (int gq = 0; gq < NG; ++gq) o += cred[gq][tid];
        out[tid] = o;
    }
    if (tid == 0) { out[DK] = m_run; out[DK + 1] = l_run; }
}

hipError_t launch_attn_step(const AttnStep& a, hipStream_t st) {
    if ((a.DK != 64 && a.DK != 32) || a.NS < 1 || a.Tcap % 4) return hipErrorInvalidValue;
    AttnStepArgs k{a.q, a.kc, a.vc, a.ptab, a.bias_u, a.bias_v, a.pos, a.part, a.H, a.Tcap, a.R, a.PR, a.NS};
    if (a.DK == 64) hipLaunchKernelGGL(attn_step_kernel<64>, dim3(a.H, a.B, a.NS), dim3(256), 0, st, k);
    else hipLaunchKernelGGL(attn_step_kernel<32>, dim3(a.H, a.B, a.NS), dim3(256), 0, st, k);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Device-side token sampling (LauraGenModel.sampling_ids, laura_model.py:466-499; the loop body of decode_codec :537-542).
// One workgroup per utterance, the nq groups in turn.  The reference samples from softmax(log_softmax(logits)[group]) =
// softmax(logits[group]).  The multinomial draw is the inverse CDF of ONE uniform number per (utterance, step, group) from a
// counter-based generator (Philox4x32-10 keyed by the caller's seed), so a generation is reproducible from its seed and never
// leaves the device; torch.multinomial's own generator stream cannot be shared by any second implementation.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned mulhi32(unsigned a, unsigned b) { return __umulhi(a, b); }
__device__ float philox_uniform(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2) {
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    unsigned x0 = c0, x1 = c1, x2 = c2, x3 = 0x5eedu;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = mulhi32(0xD2511F53u, x0), l0 = 0xD2511F53u * x0;
        const unsigned h1 = mulhi32(0xCD9E8D57u, x2), l1 = 0xCD9E8D57u * x2;
        const unsigned n0 = h1 ^ x1 ^ k0, n1 = l1, n2 = h0 ^ x3 ^ k1, n3 = l0;
        x0 = n0; x1 = n1; x2 = n2; x3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (float)(x0 >> 8) * (1.0f / 16777216.0f);      // [0, 1)
}

struct SampleArgs {
    const float* logits;
    int K, nq, mode, ki;
    float pf;
    unsigned long long seed;
    const int64_t* forced;
    int max_steps;
    int64_t* tokens;
    int tok_stride;
    const int* tok_off;
    int *n_gen, *done, *n_done, *pos, *step;
    float* logp_out;
    float* score_out;
    const float* cb;
    int D;
    float* next_emb;
    int B;
    // fused input layer of the LM for the next step (TransformerEncoder_s0.embed, transformer_encoder.py:463-470):
    // xs[b] = [relu](LayerNorm(W e + bias)) * xscale;  emb_wt [D][dm] (W transposed), null = not fused
    const float *emb_wt, *emb_bias, *emb_g, *emb_b;
    int dm, emb_relu;
    float xscale;
    float* xs;
    unsigned* launch_seq;
    // decoding session: per-row parameters (null: the call's own, above), the row stride of forced / logp_out / score_out, the first row of this launch
    const SampleRow* rows;
    int stride, row0;
    // a queued session's refill phase (sample_kernel<true>): the claim table and its line count, else null
    const QueueClaim* claims;
    const int* nclaims;
};

#define FC_SAMPLE_MAXV 2048      // candidates per group, padded to a power of two for the bitonic sort (K + 1 <= 2048)

// ---------------------------------------------------------------------------------------------------------------------
// The tail of a sample: the LM's next input row of utterance b from the nq chosen ids.  next_emb[b] = sum_k cb[k][chosen[k]], then (emb_wt
// given) the LM's fused input layer into xs[b].  One 256-thread workgroup; val[] / idx[] (FC_SAMPLE_MAXV words each) and wred[4] are the
// caller's LDS, free at this point; chosen[] is visible to every thread.  sample_kernel and slot_branch_kernel both call this and nothing
// else, so a slot that is re-embedded from a kept token gets the sampler's own bits.
// ---------------------------------------------------------------------------------------------------------------------
struct EmbedNext {
    const float* cb;
    int K, nq, D;
    float* next_emb;
    const float *emb_wt, *emb_bias, *emb_g, *emb_b;
    int dm, emb_relu;
    float xscale;
    float* xs;
};

__device__ __forceinline__ void embed_next(const EmbedNext& e, int b, const int* chosen, float* val, int* idx, float* wred) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // next LM input: sum of the groups' codebook rows (build_llm_io -> calc_dense_vector)
    for (int dd = tid; dd < e.D; dd += 256) {
        float s = 0.f;
        for (int k = 0; k < e.nq; ++k) {
            const float v = e.cb[((size_t)k * e.K + chosen[k]) * e.D + dd];
            s = k == 0 ? v : s + v;
        }
        e.next_emb[(size_t)b * e.D + dd] = s;
        val[dd] = s;                                   // val[] is free now: the embedding for the fused input layer
    }
    if (e.emb_wt) {
        __syncthreads();
        // y[n] = bias[n] + sum_k W^T[k][n] e[k]: thread (output quad nq4, k part kp) takes 4 consecutive outputs over its share of
        // the k range with independent 16-byte loads; the parts meet in LDS (idx[] reinterpreted, free now)
        float* ysum = (float*)idx;                      // [dm] after the reduction
        const int nquads = e.dm >> 2;                   // dm % 4 == 0
        const int kparts = 256 / nquads > 0 ? 256 / nquads : 1;
        const int nq4 = tid % nquads, kp = tid / nquads;
        const int kper = (e.D + kparts - 1) / kparts;
        f32x4 accq = {0.f, 0.f, 0.f, 0.f};
        if (kp < kparts && tid < nquads * kparts) {
            const int kb0 = kp * kper, kb1 = kb0 + kper < e.D ? kb0 + kper : e.D;
            const float* wq = e.emb_wt + 4 * nq4;
            int kk = kb0;
            for (; kk + 16 <= kb1; kk += 16) {          // 16 independent 16-byte loads in flight (the table is cold in L2 every step)
                f32x4 wv16[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) wv16[u] = *(const f32x4*)(wq + (size_t)(kk + u) * e.dm);
#pragma unroll
                for (int u = 0; u < 16; ++u) accq += val[kk + u] * wv16[u];
            }
            for (; kk + 4 <= kb1; kk += 4) {
                f32x4 wv4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) wv4[u] = *(const f32x4*)(wq + (size_t)(kk + u) * e.dm);
#pragma unroll
                for (int u = 0; u < 4; ++u) accq += val[kk + u] * wv4[u];
            }
            for (; kk < kb1; ++kk) accq += val[kk] * *(const f32x4*)(wq + (size_t)kk * e.dm);
        }
        __syncthreads();                                // everybody is done with idx[] (the sampler's candidate ids)
        float* ypart = (float*)idx;                     // [kparts][dm], kparts * dm <= 2048 floats
        if (tid < nquads * kparts) *(f32x4*)(ypart + kp * e.dm + 4 * nq4) = accq;
        __syncthreads();
        float yv[4];
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = tid + 256 * i;
            yv[i] = 0.f;
            if (n < e.dm) {
                float acc = e.emb_bias[n];
                for (int q = 0; q < kparts; ++q) acc += ypart[q * e.dm + n];
                yv[i] = acc;
                ps += acc;
            }
        }
        (void)ysum;
        ps = wave_sum(ps);
        if (lane == 0) wred[w] = ps;
        __syncthreads();
        const float mean = (wred[0] + wred[1] + wred[2] + wred[3]) / (float)e.dm;
        __syncthreads();
        float pq = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (tid + 256 * i < e.dm) { const float dv = yv[i] - mean; pq += dv * dv; }
        pq = wave_sum(pq);
        if (lane == 0) wred[w] = pq;
        __syncthreads();
        const float rstd = 1.f / sqrtf((wred[0] + wred[1] + wred[2] + wred[3]) / (float)e.dm + 1e-5f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = tid + 256 * i;
            if (n < e.dm) {
                float o = (yv[i] - mean) * rstd * e.emb_g[n] + e.emb_b[n];
                if (e.emb_relu) o = o > 0.f ? o : 0.f;
                e.xs[(size_t)b * e.dm + n] = o * e.xscale;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// sum over a group of exp(x - m), m the group's maximum: the normaliser of softmax(logits[group]), by all 256 threads.  xr[] holds the
// thread's logits (entry i = logit tid + 256 i, clamped past G).  One statement of the sum, so that the sampling modes, which draw from
// it, and the step's score (SampleArgs::score_out), which greedy mode forms without drawing, get the same bits: per thread in i order,
// wave_sum, the four waves in wave order.  STORE: the unnormalised probabilities and their indices into val[] / idx[] for the draw
// (padding -1: sorts last).  Ends behind a barrier; wred[] is read by every thread and free again at the caller's next barrier.
// ---------------------------------------------------------------------------------------------------------------------
template <bool STORE>
__device__ __forceinline__ float group_exp_total(const float (&xr)[FC_SAMPLE_MAXV / 256], float m, int G, float* val, int* idx, float* wred) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < FC_SAMPLE_MAXV / 256; ++i) {
        const int v = tid + 256 * i;
        const float e = v < G ? expf(xr[i] - m) : -1.f;
        if (STORE) {
            val[v] = e;
            idx[v] = v;
        }
        if (v < G) s += e;
    }
    s = wave_sum(s);
    if (lane == 0) wred[w] = s;
    __syncthreads();
    return wred[0] + wred[1] + wred[2] + wred[3];
}

// ---------------------------------------------------------------------------------------------------------------------
// One draw by inverse CDF over the first ncand candidates of val[] / idx[] in their order: chunk sums, then an exact walk inside the
// chunk.  The uniform number is Philox of (seed, step, rng_row, word).  All 256 threads call it; returns the drawn candidate's id to
// every thread.  csum[256] and sh_pick are the caller's LDS.  The sampler's first draw of a group (word = the group) and the repeat
// rule's second draw (word = 8 + the group) both go through here and nowhere else.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int draw_inverse_cdf(const float* val, const int* idx, int ncand, float* csum, int* sh_pick,
                                                unsigned long long seed, unsigned step, unsigned rng_row, unsigned word) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int CH = (ncand + 255) / 256;
    float cs = 0.f;
    for (int i = tid * CH; i < (tid + 1) * CH && i < ncand; ++i) cs += val[i];
    csum[tid] = cs;
    __syncthreads();
    if (w == 0) {        // wave 0: lane l owns chunks 4l .. 4l+3; prefix sums by shuffles, then one lane walks its chunks / elements
        const float c0 = csum[4 * lane], c1 = csum[4 * lane + 1], c2 = csum[4 * lane + 2], c3 = csum[4 * lane + 3];
        const float mine = (c0 + c1) + (c2 + c3);
        float incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        const float tot = __shfl(incl, 63, 64);
        const float u = philox_uniform(seed, step, rng_row, word);
        const float target = u * tot;
        const float below = incl - mine;
        // the lane whose range [below, incl) holds the target; rounding at the very top goes to the last non-empty lane
        const unsigned long long nonempty = __ballot(mine > 0.f);
        const unsigned long long ballot = __ballot(mine > 0.f && target >= below && target < incl);
        const int owner = ballot ? (int)__ffsll((long long)ballot) - 1 : (nonempty ? 63 - __clzll((long long)nonempty) : 0);
        if (lane == owner) {
            float run = below;
            int c = 0;                                  // the first of the lane's chunks 0 .. 2 that the target falls in, else chunk 3
            if (run + c0 <= target) {
                run += c0; c = 1;
                if (run + c1 <= target) {
                    run += c1; c = 2;
                    if (run + c2 <= target) { run += c2; c = 3; }
                }
            }
            int i = (4 * lane + c) * CH;
            const int iend = (4 * lane + c + 1) * CH < ncand ? (4 * lane + c + 1) * CH : ncand;
            while (i + 1 < iend && run + val[i] <= target) { run += val[i]; ++i; }
            if (i >= ncand) i = ncand - 1;
            // a walk that rounding carried to the end of a chunk can stand on an entry without mass (an underflowed expf, a masked id):
            // the CDF does not rise there, the draw belongs to the last entry before it that has some
            while (i > 0 && !(val[i] > 0.f)) --i;
            if (i < 0) i = 0;
            *sh_pick = idx[i];
        }
    }
    __syncthreads();
    const int pick = *sh_pick;
    __syncthreads();
    return pick;
}

// The score of a step (score_out, a decoding session opened with scores): for utterance b at generated step gen, with the FINAL picks t[k]
// of the groups (a forced token replaces the draw first),
//     term[gen] = sum over k < nq, in k order, of ( (x_k[t[k]] - m_k) - logf(sum_v exp(x_k[v] - m_k)) ),
// the log of the probability LauraGenModel.sampling_ids gives the picks before any top-k / nucleus truncation (laura_model.py:466-499:
// softmax over the group's own G = K + 1 logits; step_logp's rows are the whole-vocabulary log-softmax instead).  A function of the step's
// logits and the final picks only: the same bits in every sampling mode and for forced tokens (greedy mode, which draws nothing, runs
// group_exp_total for it).  Thread 0 forms and writes it, for every step the sampler runs for the row, the ending <eos> step included.
//
// A row's sampling rules (SampleRow, stated in full at fc_laura_slots_set_rules): x above is the group's logits AFTER the temperature
// (x / T, an fp32 division) and the minimum length (<eos> = -inf while gen < min_length), so the arg-max, the softmax total, the top-k
// select, the nucleus walk and the score all see that vector; logp_out stays the log-softmax of the raw logits.  top_p cuts the top-k
// candidates to their nucleus; the repeat rule draws a second time, from the whole group in index order, when the first draw fills the
// window.  While <eos> is masked it is the last candidate in every order (probability 0, the highest index) and is left out of the
// candidates, so no rounding of the draw can return it.  The neutral rules skip every one of these statements.
//
//
// CLAIMS: a second instantiation for a queued session's refill phase -- block i takes the row from line i of the claim table and the
// blocks behind the claim count leave at once.  CLAIMS false is every other launch: the same statements as before the parameter
// (as gemv_kernel's WIDE), compiled to the same number of instructions, registers (112 VGPRs, no private segment) and LDS bytes.
template <bool CLAIMS>
__global__ __launch_bounds__(256) void sample_kernel(SampleArgs a) {
    if constexpr (CLAIMS) {
        if ((int)blockIdx.x >= *a.nclaims) return;
    }
    __shared__ __attribute__((aligned(16))) float val[FC_SAMPLE_MAXV];
    __shared__ __attribute__((aligned(16))) int idx[FC_SAMPLE_MAXV];
    __shared__ float csum[256];
    __shared__ float wred[4];
    __shared__ int wredi[4];
    __shared__ int chosen[8];
    __shared__ float sh_f[2];
    __shared__ int sh_i[2];
    __shared__ unsigned hist[256];
    __shared__ float cval[256];
    __shared__ int cidx[256];
    __shared__ int ccount;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = CLAIMS ? a.claims[blockIdx.x].slot : a.row0 + blockIdx.x;
    const int G = a.K + 1, V = a.nq * G;
    // the call's parameters, or the row's own (a decoding session: the table is device memory, so a captured step never changes)
    const SampleRow* row = a.rows ? a.rows + b : nullptr;
    const int mode = row ? row->mode : a.mode, ki = row ? row->ki : a.ki, max_steps = row ? row->max_steps : a.max_steps;
    const float pf = row ? row->pf : a.pf;
    const unsigned long long seed = row ? row->seed : a.seed;
    const int64_t* forced = (row && !row->forced_on) ? nullptr : a.forced;
    const unsigned rng_row = row ? row->rng_row : (unsigned)b;      // second word of the Philox counter
    const int step = a.step[b];          // per-utterance sample counter (RNG stream position)
    const int gen = a.n_gen[b];
    const bool was_done = a.done[b] != 0;
    // the row's rules (a call without a table has the neutral ones), through LDS: as five more scalars, or read through `row` where
    // they are used, they cost the kernel a private segment (68 / 100 bytes per lane reserved, no access to it)
    __shared__ float sh_rf[2];                       // temperature, top_p
    __shared__ int sh_ri[3];                         // min_length, repeat_window, repeat_count
    if (tid == 0) {
        sh_rf[0] = row ? row->temperature : 1.f; sh_rf[1] = row ? row->top_p : 0.f;
        sh_ri[0] = row ? row->min_length : 0; sh_ri[1] = row ? row->repeat_window : 0; sh_ri[2] = row ? row->repeat_count : 1;
    }
    __syncthreads();
    const float* lg = a.logits + (size_t)b * V;
    // log-softmax over the whole vocabulary of the step (TransformerEmbedLM.score, transformer_lm.py:309-311), when asked for
    if (a.logp_out && !was_done && gen < max_steps) {
        float m = -INFINITY;
        for (int v = tid; v < V; v += 256) m = fmaxf(m, lg[v]);
        m = wave_max(m);
        if (lane == 0) wred[w] = m;
        __syncthreads();
        m = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
        __syncthreads();
        float s = 0.f;
        for (int v = tid; v < V; v += 256) s += expf(lg[v] - m);
        s = wave_sum(s);
        if (lane == 0) wred[w] = s;
        __syncthreads();
        const float ls = logf(wred[0] + wred[1] + wred[2] + wred[3]);
        float* o = a.logp_out + ((size_t)b * a.stride + gen) * V;
        for (int v = tid; v < V; v += 256) o[v] = (lg[v] - m) - ls;
        __syncthreads();
    }
    float term = 0.f;                                // thread 0: the step's score
    for (int k = 0; k < a.nq; ++k) {
        const float* x = lg + k * G;
        // ---- group maximum and its FIRST index (greedy: weighted_scores.topk(1))
        // the group's logits, once, as 8 unconditional clamped loads per thread (a `for (v = tid; v < G; v += 256)` loop waits for
        // every load before the next: three such passes per group were most of this kernel's 33 us)
        constexpr int XPT = FC_SAMPLE_MAXV / 256;
        float xr[XPT];
#pragma unroll
        for (int i = 0; i < XPT; ++i) { const int v = tid + 256 * i; xr[i] = x[v < G ? v : G - 1]; }
        // rules 1 and 2: everything below sees x / T with <eos> masked
        const float temp = sh_rf[0];
        const bool no_eos = gen < sh_ri[0];           // <eos> masked at this step
        if (temp != 1.f) {
#pragma unroll
            for (int i = 0; i < XPT; ++i) xr[i] = __fdiv_rn(xr[i], temp);
        }
        if (no_eos) {
#pragma unroll
            for (int i = 0; i < XPT; ++i)
                if (tid + 256 * i >= G - 1) xr[i] = -INFINITY;          // <eos>, and the clamped copies of it behind the group
        }
        float m = -INFINITY;
        int mi = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int v = tid + 256 * i;
            if (v < G && xr[i] > m) { m = xr[i]; mi = v; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(m, o, 64);
            const int oi = __shfl_xor(mi, o, 64);
            if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
        }
        if (lane == 0) { wred[w] = m; wredi[w] = mi; }
        __syncthreads();
        m = wred[0]; mi = wredi[0];
        for (int u = 1; u < 4; ++u)
            if (wred[u] > m || (wred[u] == m && wredi[u] < mi)) { m = wred[u]; mi = wredi[u]; }
        __syncthreads();
        int pick = mi;
        float norm = 0.f;                            // the group's sum of exp(x - max), where the step's score needs it
        if (mode == 0 && a.score_out) norm = group_exp_total<false>(xr, m, G, val, idx, wred);
        if (mode != 0) {
            // unnormalised probabilities exp(x - max) (the normaliser cancels in every mode except the nucleus threshold)
            const float total = group_exp_total<true>(xr, m, G, val, idx, wred);
            norm = total;
            int ncand = G;
            bool selected = false;                   // top-k candidates already in val[] / idx[] order
            if (mode == 2 && ki <= 64) {
                // top-k with a small k (the recipe samples with --sampling 25): radix-select the k-th largest logit (4 passes over
                // 8-bit digits of the order-preserving integer image of the float), collect everything >= it, order those few by
                // (probability descending, index ascending) with a counting rank -- no full sort of the 1025 logits
                const int kk = ki < 1 ? 1 : ki;
                unsigned lk[XPT];
                int nl = 0;
#pragma unroll
                for (int i = 0; i < XPT; ++i) {
                    unsigned u = __float_as_uint(xr[i]);
                    if (u == 0x80000000u) u = 0u;       // -0.0 = +0.0 in every float comparison of this kernel: one key for both
                    lk[i] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                    if (tid + 256 * i < G) nl = i + 1;
                }
                unsigned prefix = 0u, mask = 0u;
                int need = kk;
                for (int shift = 24; shift >= 0; shift -= 8) {
                    hist[tid] = 0u;
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < XPT; ++i)
                        if (i < nl && (lk[i] & mask) == prefix) atomicAdd(&hist[(lk[i] >> shift) & 255u], 1u);
                    __syncthreads();
                    if (w == 0) {        // wave 0: lane l owns bins 4l .. 4l+3; suffix sums (bins above) by shuffles, then one lane walks its 4 bins
                        const int h0 = (int)hist[4 * lane], h1 = (int)hist[4 * lane + 1], h2 = (int)hist[4 * lane + 2], h3 = (int)hist[4 * lane + 3];
                        const int mine = h0 + h1 + h2 + h3;
                        int incl = mine;
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            const int t = __shfl_down(incl, o, 64);
                            if (lane + o < 64) incl += t;
                        }
                        const int above = incl - mine;               // entries in bins of higher lanes
                        if (above < need && need <= incl) {
                            int cum = above, bin = 4 * lane + 3;
                            const int hh[4] = {h0, h1, h2, h3};
                            for (; bin > 4 * lane; --bin) {
                                if (cum + hh[bin & 3] >= need) break;
                                cum += hh[bin & 3];
                            }
                            sh_i[0] = bin;
                            sh_i[1] = need - cum;
                        }
                    }
                    __syncthreads();
                    prefix |= (unsigned)sh_i[0] << shift;
                    need = sh_i[1];
                    mask |= 255u << shift;
                    __syncthreads();
                }
                if (tid == 0) ccount = 0;
                __syncthreads();
#pragma unroll
                for (int i = 0; i < XPT; ++i) {
                    const int v = tid + 256 * i;
                    if (i < nl && lk[i] >= prefix) {
                        const int slot = atomicAdd(&ccount, 1);
                        if (slot < 256) { cval[slot] = val[v]; cidx[slot] = v; }
                    }
                }
                __syncthreads();
                // more than 256 logits at or above the k-th key (hundreds of ties at the threshold: saturated or constant logits): which of
                // them the 256 slots hold depends on the order of the atomics -- take the full sort below instead, whose tie-break
                // (probability descending, index ascending) is the documented one.  ccount is uniform here.
                if (ccount <= 256) {
                    const int nc = ccount;
                    float myv = 0.f;
                    int myi = 0, rank = 0;
                    if (tid < nc) {
                        myv = cval[tid]; myi = cidx[tid];
                        for (int c = 0; c < nc; ++c) {
                            const float ov = cval[c];
                            const int oi = cidx[c];
                            rank += (ov > myv || (ov == myv && oi < myi)) ? 1 : 0;
                        }
                    }
                    __syncthreads();
                    if (tid < nc) { val[rank] = myv; idx[rank] = myi; }
                    __syncthreads();
                    ncand = kk < nc ? kk : nc;
                    selected = true;
                }
            }
            if (!selected && mode >= 2) {
                // descending by probability, ties by index (topk / a stable descending sort): bitonic sort of 2048 pairs
                for (int kk = 2; kk <= FC_SAMPLE_MAXV; kk <<= 1)
                    for (int j = kk >> 1; j > 0; j >>= 1) {
                        __syncthreads();
                        for (int i = tid; i < FC_SAMPLE_MAXV; i += 256) {
                            const int l = i ^ j;
                            if (l > i) {
                                const bool up = (i & kk) == 0;      // "up" = descending order here
                                const float vi = val[i], vl = val[l];
                                const int ii = idx[i], il = idx[l];
                                const bool i_first = vi > vl || (vi == vl && ii < il);
                                if (up ? !i_first : i_first) { val[i] = vl; val[l] = vi; idx[i] = il; idx[l] = ii; }
                            }
                        }
                    }
                __syncthreads();
                if (mode == 2) ncand = ki < G ? (ki < 1 ? 1 : ki) : G;
                else {
                    // nucleus: take entries while the running probability mass is < pf (the entry that crosses is kept)
                    if (tid == 0) {
                        float cum = 0.f;
                        int n = 0;
                        const float thr = pf * total;
                        while (n < G && cum < thr) { cum += val[n]; ++n; }
                        sh_i[0] = n < 1 ? 1 : n;
                    }
                    __syncthreads();
                    ncand = sh_i[0];
                }
            }
            const float top_p = sh_rf[1];
            const int rep_w = sh_ri[1];
            if (mode == 2 && top_p > 0.f) {
                // top-k with top-p: mode 3's walk over the top-k candidates, stopped at k
                if (tid == 0) {
                    float cum = 0.f;
                    int n = 0;
                    const float thr = top_p * total;
                    while (n < ncand && cum < thr) { cum += val[n]; ++n; }
                    sh_i[0] = n < 1 ? 1 : n;
                }
                __syncthreads();
                ncand = sh_i[0];
            }
            if (no_eos && ncand > G - 1) ncand = G - 1;
            // the draw, and under the repeat rule at most one more (one statement of the draw for both: every condition is uniform)
            for (unsigned word = (unsigned)k;; word += 8u) {
                pick = draw_inverse_cdf(val, idx, ncand, csum, &sh_i[1], seed, (unsigned)step, rng_row, word);
                if (rep_w <= 0 || word >= 8u) break;
                // the repeat rule: how often the drawn id stands in the group's last rep_w generated tokens, one token per thread
                const int j = gen - 1 - tid;
                bool hit = false;
                if (tid < rep_w && j >= 0) hit = a.tokens[((size_t)b * a.tok_stride + a.tok_off[b] + j) * a.nq + k] == (int64_t)pick;
                const unsigned long long hits = __ballot(hit);
                if (lane == 0) wredi[w] = __popcll(hits);
                __syncthreads();
                const int count = wredi[0] + wredi[1] + wredi[2] + wredi[3];
                __syncthreads();
                if (count < sh_ri[2]) break;
                // drawn again from softmax over the whole group in index order: val[] / idx[] rebuilt from the registers (the select
                // overwrote their head), the same sum as the first time
                group_exp_total<true>(xr, m, G, val, idx, wred);
                ncand = no_eos ? G - 1 : G;
            }
        }
        if (tid == 0) {
            if (forced && gen < max_steps) pick = (int)forced[((size_t)b * a.stride + gen) * a.nq + k];
            chosen[k] = pick;
            if (a.score_out) {                       // from the logits row: val[] is sorted by now
                const int pc = pick < 0 ? 0 : (pick < G ? pick : G - 1);
                float xp = x[pc];
                if (temp != 1.f) xp = __fdiv_rn(xp, temp);         // as xr[] above
                if (no_eos && pc == G - 1) xp = -INFINITY;         // a forced <eos> below the minimum length
                const float t = (xp - m) - logf(norm);
                term = k == 0 ? t : term + t;
            }
        }
        __syncthreads();
    }
    // the step's score, for a step that runs for the row (`active` below).  Written here, not in the bookkeeping at the end: the pointer
    // live across embed_next cost the kernel a private segment (68 bytes per lane reserved, no access to it) even when it is null
    if (tid == 0 && a.score_out && !was_done && gen < max_steps) a.score_out[(size_t)b * a.stride + gen] = term;
    // ---- bookkeeping of decode_codec (laura_model.py:519-546): a step whose ids contain <eos> ends the utterance and is dropped
    bool eos = false;
    for (int k = 0; k < a.nq; ++k) eos = eos || chosen[k] == a.K;
    const bool active = !was_done && gen < max_steps;
    if (active && !eos) {
        if (tid < a.nq) a.tokens[((size_t)b * a.tok_stride + a.tok_off[b] + gen) * a.nq + tid] = (int64_t)chosen[tid];
        embed_next(EmbedNext{a.cb, a.K, a.nq, a.D, a.next_emb, a.emb_wt, a.emb_bias, a.emb_g, a.emb_b, a.dm, a.emb_relu, a.xscale, a.xs},
                   b, chosen, val, idx, wred);
    }
    __syncthreads();
    if (tid == 0) {
        if (active) {
            if (eos) { a.done[b] = 1; atomicAdd(a.n_done, 1); }
            else {
                a.n_gen[b] = gen + 1;
                if (step > 0) a.pos[b] += 1;      // step 0 samples from the prefix; later steps appended one token to the cache
                if (gen + 1 >= max_steps) { a.done[b] = 1; atomicAdd(a.n_done, 1); }
            }
        }
        a.step[b] = step + 1;
        if (blockIdx.x == 0 && a.launch_seq) *a.launch_seq += 1u;
    }
}

hipError_t launch_sample(const Sample& s, hipStream_t st) {
    if (s.K + 1 > FC_SAMPLE_MAXV || s.nq > 8 || s.nq < 1) return hipErrorInvalidValue;
    if (s.emb_wt && (s.dm > 1024 || s.dm % 4 || s.D > FC_SAMPLE_MAXV)) return hipErrorInvalidValue;
    SampleArgs a{s.logits, s.K, s.nq, s.mode, s.ki, s.pf, s.seed, s.forced, s.max_steps, s.tokens, s.tok_stride, s.tok_off, s.n_gen,
                 s.done, s.n_done, s.pos, s.step, s.logp_out, s.score_out, s.cb, s.D, s.next_emb, s.B,
                 s.emb_wt, s.emb_bias, s.emb_g, s.emb_b, s.dm, s.emb_relu, s.xscale, s.xs, s.launch_seq,
                 s.rows, s.rows ? s.row_stride : s.max_steps, s.row0, nullptr, nullptr};
    const int n = s.nrows > 0 ? s.nrows : s.B;
    if (s.row0 < 0 || s.row0 + n > s.B) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_kernel<false>, dim3(n), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// One slot of a decoding session back to "nothing generated": its counters and position, its row of the sampling table, a zero LM
// input row, its token row = the continual prompt (what copy_prompt_kernel does per call) followed by zeros, its forced tokens, zero
// log-probability rows, a zero score row.  The other slots' rows are not touched.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slot_reset_kernel(SlotReset r) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
    const int b = r.slot;
    if (tid == 0) {
        r.n_gen[b] = 0; r.done[b] = r.free_slot ? 1 : 0; r.step[b] = 0; r.pos[b] = 0; r.tok_off[b] = r.cont_len;
        r.rows[b] = r.row;
    }
    for (size_t i = tid; i < (size_t)r.dm; i += nth) r.xs[(size_t)b * r.dm + i] = 0.f;
    const size_t nprompt = (size_t)r.cont_len * r.nq, ntok = (size_t)r.tok_stride * r.nq;
    for (size_t i = tid; i < ntok; i += nth) r.tokens[(size_t)b * ntok + i] = i < nprompt ? r.continual[i] : 0;
    if (r.forced_src) {
        const size_t nf = (size_t)r.row.max_steps * r.nq;
        for (size_t i = tid; i < nf; i += nth) r.forced[(size_t)b * ntok + i] = r.forced_src[i];
    }
    if (r.logp) {
        const size_t nl = (size_t)r.row.max_steps * r.V;
        for (size_t i = tid; i < nl; i += nth) r.logp[(size_t)b * r.tok_stride * r.V + i] = 0.f;
    }
    if (r.score)
        for (size_t i = tid; i < (size_t)r.tok_stride; i += nth) r.score[(size_t)b * r.tok_stride + i] = 0.f;
}
hipError_t launch_slot_reset(const SlotReset& r, hipStream_t st) {
    if (r.slot < 0 || r.cont_len < 0 || r.row.max_steps < 0 || r.cont_len + r.row.max_steps > r.tok_stride) return hipErrorInvalidValue;
    hipLaunchKernelGGL(slot_reset_kernel, dim3(64), dim3(256), 0, st, r);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The prefix of slot `src` of a source session (its first P cache positions and the logits its prefix pass ended with) into slot `dst`
// of a destination session of the same engine: what a prefix pass of the same prompt would leave there, bit for bit, for the price of a
// copy.  The two sessions may be one (fc_laura_slots_start_from, fork: dst != src then) or two whose slot counts and cache pitches
// differ.  grid.y = layer; along x a layer's K vectors, then its V vectors, then one block (layer 0 only) for the logits and the
// position.  A block takes FC_PREFIX_VPT x 256 consecutive 16-byte vectors, its loads in flight together (kv_chunk_copy).
//   K [d][Tcap]: rows of pad4(P) floats from pitch Tcap_src to pitch Tcap_dst (both % 4 == 0: every row start is 16-byte aligned).
//   Columns [P, pad4(P)) carry whatever the source holds there (its own later positions).  A destination never reads a column it did
//   not write itself: a step writes K and V at pos before its attention reads keys 0 .. pos -- on the kernel chain the QKV GEMV's
//   scatter is the launch ahead of attn_step_kernel, in the persistent step an attention unit waits for the whole QKV phase
//   (wait_phase(ph - 1)) -- and the first step of a destination runs at pos = P.  (A slot reused by `start` has its previous
//   utterance's columns there in the same way.)
//   V [Tcap][d]: the first P * d floats of the slot's row, contiguous in both sessions (d % 4 == 0).
//   lg0_src[src] into lg_dst[dst] and lg0_dst[dst]; pos_dst[dst] = P.
// ---------------------------------------------------------------------------------------------------------------------
#define FC_PREFIX_VPT 4
typedef long long i64x2 __attribute__((ext_vector_type(2)));

// blocks of FC_PREFIX_VPT x 256 vectors that hold nvec vectors
__host__ __device__ inline int prefix_blocks(int nvec) { return (nvec + 256 * FC_PREFIX_VPT - 1) / (256 * FC_PREFIX_VPT); }

// chunks of one layer's first P positions of one slot: its K vectors (d rows of pad4(P) / 4), then its V vectors
__device__ __forceinline__ int kv_chunks(int d, int P) { return prefix_blocks(d * ((P + 3) >> 2)) + prefix_blocks((P * d) >> 2); }

// Chunk `chunk` < kv_chunks(d, P) of that copy, by the 256 threads of a block: ks / vs and kd / vd are the slot's K and V rows of the
// layer in the source and the destination, whose pitches are Tcap_s and Tcap_d.
__device__ __forceinline__ void kv_chunk_copy(const float* ks, const float* vs, float* kd, float* vd, int Tcap_s, int Tcap_d, int d, int P,
                                              int chunk, int tid) {
    const int kq = (P + 3) >> 2;                                      // vectors per K row: pad4(P) / 4
    const int nK = d * kq, nV = (P * d) >> 2, bK = prefix_blocks(nK);
    const bool isK = chunk < bK;
    const float* sb = isK ? ks : vs;
    float* db = isK ? kd : vd;
    const int nvec = isK ? nK : nV;
    const int i0 = (isK ? chunk : chunk - bK) * 256 * FC_PREFIX_VPT + tid;
    size_t od[FC_PREFIX_VPT];
    f32x4 v[FC_PREFIX_VPT];
#pragma unroll
    for (int u = 0; u < FC_PREFIX_VPT; ++u) {
        int i = i0 + 256 * u;
        i = i < nvec ? i : nvec - 1;                                  // clamped: unconditional loads, predicated stores
        const size_t os = isK ? (size_t)(i / kq) * Tcap_s + 4 * (size_t)(i % kq) : 4 * (size_t)i;
        od[u] = isK ? (size_t)(i / kq) * Tcap_d + 4 * (size_t)(i % kq) : 4 * (size_t)i;
        v[u] = *(const f32x4*)(sb + os);
    }
#pragma unroll
    for (int u = 0; u < FC_PREFIX_VPT; ++u)
        if (i0 + 256 * u < nvec) *(f32x4*)(db + od[u]) = v[u];
}

// a row of V logits into a slot's row of the step's logits and of the saved prefix logits (V need not be a multiple of 4: scalar)
__device__ __forceinline__ void copy_logits(const float* __restrict__ s, float* lg, float* lg0, int V, int t0, int nth) {
    for (int v = t0; v < V; v += nth) {
        const float x = s[v];
        lg[v] = x;
        lg0[v] = x;
    }
}

// nvec 16-byte vectors of zeros from `row` on (16-byte aligned)
__device__ __forceinline__ void zero_row(float* row, int nvec, int t0, int nth) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = t0; i < nvec; i += nth) ((f32x4*)row)[i] = zero;
}

__global__ __launch_bounds__(256) void prefix_import_kernel(PrefixImport c) {
    const int l = blockIdx.y, tid = threadIdx.x, blk = blockIdx.x;
    if (blk >= kv_chunks(c.d, c.P)) {                                 // the logits, the saved logits, the position
        if (l != 0) return;
        copy_logits(c.lg0_src + (size_t)c.src * c.V, c.lg_dst + (size_t)c.dst * c.V, c.lg0_dst + (size_t)c.dst * c.V, c.V, tid, 256);
        if (tid == 0) c.pos_dst[c.dst] = c.P;
        return;
    }
    const size_t os = ((size_t)l * c.S_src + c.src) * c.d * c.Tcap_src, od = ((size_t)l * c.S_dst + c.dst) * c.d * c.Tcap_dst;
    kv_chunk_copy(c.kc_src + os, c.vc_src + os, c.kc_dst + od, c.vc_dst + od, c.Tcap_src, c.Tcap_dst, c.d, c.P, blk, tid);
}

// the grid of that copy along x without its last block: false where the vectors of a layer cannot be counted in int
static bool prefix_chunks(int d, int P, int* bK, int* bV) {
    const long long nK = (long long)d * (((P + 3) & ~3) >> 2), nV = ((long long)P * d) >> 2;
    if (nK > 0x7fffffff || nV > 0x7fffffff) return false;
    *bK = prefix_blocks((int)nK); *bV = prefix_blocks((int)nV);
    return true;
}

hipError_t launch_prefix_import(const PrefixImport& c, hipStream_t st) {
    if (c.NL < 1 || c.S_src < 1 || c.S_dst < 1 || c.src < 0 || c.src >= c.S_src || c.dst < 0 || c.dst >= c.S_dst) return hipErrorInvalidValue;
    if (c.d < 4 || c.d % 4 || c.Tcap_src % 4 || c.Tcap_dst % 4 || c.P < 1 || c.V < 1) return hipErrorInvalidValue;
    if (((c.P + 3) & ~3) > c.Tcap_src || ((c.P + 3) & ~3) > c.Tcap_dst) return hipErrorInvalidValue;
    // inside one session the copy must not alias: another slot, and the same pitch and slot count by construction
    if (c.kc_src == c.kc_dst && (c.dst == c.src || c.S_src != c.S_dst || c.Tcap_src != c.Tcap_dst)) return hipErrorInvalidValue;
    int bK = 0, bV = 0;
    if (!prefix_chunks(c.d, c.P, &bK, &bV)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prefix_import_kernel, dim3(bK + bV + 1, c.NL), dim3(256), 0, st, c);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Slot `dst` takes up slot `src`'s utterance as it stood after its first `keep` >= 1 generated tokens (dst == src: the slot goes back
// there in place).  What the next step and the sampler's bookkeeping read, and nothing else:
//   block 0: the LM's next input, next_emb[dst] and xs[dst], from kept token keep - 1 through embed_next -- the sampler's own tail, the
//   same block shape and LDS -- and, one thread, the counters (n_gen = step = keep, done = 0, tok_off), dst's row of the sampling table.
//   pos is the copy's (prefix_import_kernel with P + keep - 1 positions) or, in place, set here.
//   blocks 1 ..: grid-stride over 16-byte vectors of the token row ([0, cont_len + keep) kept, zeros behind), the forced row (the
//   source's) and the log-probability rows ([0, keep) kept, zeros up to max_steps: take(return_logp) relies on rows never run being
//   zero) and, in a session with scores, the score row ([0, keep) kept, zeros behind to the row's end, so a branched utterance carries
//   the score of its whole path and holds no term of the steps it left).  In place the kept parts are not touched, only the zeros behind them are written.  Every vector lies inside the slot's own
//   row: tok_stride % 4 == 0, so a row's length is a whole number of vectors and its start is 16-byte aligned.
// A source that is running may be stepped again behind this launch: rows [0, keep) of its tables never change once written.
// ---------------------------------------------------------------------------------------------------------------------
// A float row of the branch: floats [0, ncopy) of `src` kept, zeros behind them up to vector nvec (16-byte vectors; both rows start
// 16-byte aligned).  In place (same) the kept floats are not touched: the floats up to the next vector boundary one by one, whole
// vectors behind.  Thread t0 of nth.
__device__ __forceinline__ void branch_f32_row(const float* src, float* dst, size_t ncopy, size_t nvec, bool same, size_t t0, size_t nth) {
    const f32x4* sv = (const f32x4*)src;
    f32x4* dv = (f32x4*)dst;
    if (same && t0 < 4 && ncopy + t0 < ((ncopy + 3) & ~(size_t)3)) dst[ncopy + t0] = 0.f;
    for (size_t i = (same ? (ncopy + 3) >> 2 : 0) + t0; i < nvec; i += nth) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (4 * i < ncopy) v = sv[i];
        if (4 * i + 3 >= ncopy) {                                     // the vector the kept part ends in, or one behind it
            if (4 * i >= ncopy) v.x = 0.f;
            if (4 * i + 1 >= ncopy) v.y = 0.f;
            if (4 * i + 2 >= ncopy) v.z = 0.f;
            v.w = 0.f;
        }
        dv[i] = v;
    }
}

static_assert(sizeof(SampleRow) == 56, "slot_branch_kernel stores the row field by field: a new field goes there too");
__global__ __launch_bounds__(256) void slot_branch_kernel(SlotBranch r) {
    __shared__ __attribute__((aligned(16))) float val[FC_SAMPLE_MAXV];
    __shared__ __attribute__((aligned(16))) int idx[FC_SAMPLE_MAXV];
    __shared__ float wred[4];
    __shared__ int chosen[8];
    const int tid = threadIdx.x;
    const int d = r.dst, s = r.src;
    const bool same = d == s;
    const size_t ntok = (size_t)r.tok_stride * r.nq;                  // int64 per token / forced row, even
    if (blockIdx.x == 0) {
        if (tid < r.nq) chosen[tid] = (int)r.tokens[(size_t)s * ntok + (size_t)(r.cont_len + r.keep - 1) * r.nq + tid];
        __syncthreads();
        embed_next(EmbedNext{r.cb, r.K, r.nq, r.D, r.next_emb, r.emb_wt, r.emb_bias, r.emb_g, r.emb_b, r.dm, r.emb_relu, r.xscale, r.xs},
                   d, chosen, val, idx, wred);
        if (tid == 0) {
            r.n_gen[d] = r.keep; r.step[d] = r.keep; r.done[d] = 0; r.tok_off[d] = r.cont_len;
            if (same) r.pos[d] = r.P + r.keep - 1;
            // field by field: as one aggregate copy the row went through a private segment here (32 bytes per lane, 77 VGPRs)
            SampleRow* o = r.rows + d;
            o->mode = r.row.mode; o->ki = r.row.ki; o->pf = r.row.pf; o->max_steps = r.row.max_steps; o->seed = r.row.seed;
            o->forced_on = r.row.forced_on; o->rng_row = r.row.rng_row; o->temperature = r.row.temperature; o->min_length = r.row.min_length;
            o->top_p = r.row.top_p; o->repeat_window = r.row.repeat_window; o->repeat_count = r.row.repeat_count;
        }
        return;
    }
    const size_t t0 = (size_t)(blockIdx.x - 1) * 256 + tid, nth = (size_t)(gridDim.x - 1) * 256;
    {   // the token row
        const size_t ncopy = (size_t)(r.cont_len + r.keep) * r.nq;
        const i64x2* sv = (const i64x2*)(r.tokens + (size_t)s * ntok);
        i64x2* dv = (i64x2*)(r.tokens + (size_t)d * ntok);
        // in place: whole vectors behind the kept part, the odd element ahead of them on its own (kept data is never rewritten)
        if (same && (ncopy & 1) && t0 == 0) r.tokens[(size_t)d * ntok + ncopy] = 0;
        for (size_t i = (same ? (ncopy + 1) >> 1 : 0) + t0; i < ntok >> 1; i += nth) {
            i64x2 v = {0, 0};
            if (2 * i < ncopy) v = sv[i];
            if (2 * i + 1 >= ncopy) v.y = 0;
            dv[i] = v;
        }
    }
    if (!same && r.row.forced_on) {   // the forced row, as far as the source's reaches
        const size_t nf = ((size_t)r.forced_rows * r.nq + 1) >> 1;
        const i64x2* sv = (const i64x2*)(r.forced + (size_t)s * ntok);
        i64x2* dv = (i64x2*)(r.forced + (size_t)d * ntok);
        for (size_t i = t0; i < nf; i += nth) dv[i] = sv[i];
    }
    // the log-probability rows up to max_steps, the score row to its end (as the token row: a term is one float per step)
    if (r.logp)
        branch_f32_row(r.logp + (size_t)s * r.tok_stride * r.V, r.logp + (size_t)d * r.tok_stride * r.V, (size_t)r.keep * r.V,
                       ((size_t)r.row.max_steps * r.V + 3) >> 2, same, t0, nth);
    if (r.score)
        branch_f32_row(r.score + (size_t)s * r.tok_stride, r.score + (size_t)d * r.tok_stride, (size_t)r.keep, (size_t)r.tok_stride >> 2, same,
                       t0, nth);
}
hipError_t launch_slot_branch(const SlotBranch& r, hipStream_t st) {
    if (r.S < 1 || r.dst < 0 || r.dst >= r.S || r.src < 0 || r.src >= r.S || r.keep < 1 || r.cont_len < 0 || r.P < 1) return hipErrorInvalidValue;
    if (r.tok_stride % 4 || r.row.max_steps <= r.keep || r.cont_len + r.row.max_steps > r.tok_stride || r.P + r.row.max_steps > r.tok_stride)
        return hipErrorInvalidValue;
    if (r.forced_rows < 0 || r.forced_rows > r.tok_stride) return hipErrorInvalidValue;
    if (r.K + 1 > FC_SAMPLE_MAXV || r.nq > 8 || r.nq < 1 || !r.cb || !r.next_emb) return hipErrorInvalidValue;
    if (r.emb_wt && (r.dm > 1024 || r.dm % 4 || r.D > FC_SAMPLE_MAXV)) return hipErrorInvalidValue;      // as launch_sample
    hipLaunchKernelGGL(slot_branch_kernel, dim3(65), dim3(256), 0, st, r);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The refill phase of a queued decoding session.  Four launches at the head of every step, each a function of device memory only:
//   queue_turn_kernel        one wave, lane = slot.  A slot that runs a ticket and has ended is RETIRED: its result entry's words (token
//                            rows, generated count, ended on <eos>, order of finishing), a line of the retire table, no ticket any more.
//                            Then every free slot, in ascending order, CLAIMS the oldest waiting ticket: a line of the claim table, the
//                            slot's ticket and entry words, and what slot_reset_kernel's thread 0 and the prefix import's last block
//                            write -- counters, position = P, prompt length, the slot's row of the sampling table.
//   queue_retire_copy_kernel the retired slots' token rows [0, n_tok) and score rows into their entries of the result ring.
//   queue_claim_copy_kernel  per claim what slot_reset_kernel and prefix_import_kernel do: a zero LM input row, the token row = the held
//                            row's continual prompt with zeros behind, a zero score row, the prefix keys / values (the import's vectors,
//                            chunks and clamped loads in flight), the prefix logits into the step's and the saved row.
//   sample_kernel<true>      the claimed slots' first sample.
// The grids are fixed; the copy kernels stride over (table line x chunk) and read the line count first, so a step that retires or
// claims nothing costs each block one load.  Every loop is bounded by S, a table's line count or a row size; nothing waits.
// A queued session keeps no log-probability rows and takes no forced tokens, so those parts of slot_reset_kernel have no counterpart.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void queue_put_kernel(QueuePhase q, QueueTicket t, int ticket) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    q.ring[ticket % q.Q] = t;
    int* meta = q.qw + FC_QUEUE_WORDS + t.entry * FC_QUEUE_META;
    meta[FC_QMETA_STATE] = 1; meta[FC_QMETA_TICKET] = ticket; meta[FC_QMETA_NTOK] = 0; meta[FC_QMETA_NGEN] = 0; meta[FC_QMETA_EOS] = 0;
    meta[FC_QMETA_SEQ] = 0;
    q.qw[FC_QUEUE_TAIL] = ticket + 1;
}

__global__ __launch_bounds__(64) void queue_turn_kernel(QueuePhase q, int claim) {
    const int s = threadIdx.x;
    const bool valid = s < q.S;
    const unsigned long long below = (1ull << s) - 1ull;
    const int head = q.qw[FC_QUEUE_HEAD], tail = q.qw[FC_QUEUE_TAIL], fin = q.qw[FC_QUEUE_FINISHED];
    const int ticket = valid ? q.qw[FC_QUEUE_SLOT_TICKET + s] : -1;
    const bool ended = ticket >= 0 && q.done[s] != 0;
    const unsigned long long ended_mask = __ballot(ended);
    if (ended) {
        const int at = __popcll(ended_mask & below), entry = q.qw[FC_QUEUE_SLOT_ENTRY + s];
        const int gen = q.n_gen[s], n_tok = q.tok_off[s] + gen;
        q.retires[at] = QueueRetire{s, entry, n_tok, 0};
        int* meta = q.qw + FC_QUEUE_WORDS + entry * FC_QUEUE_META;
        meta[FC_QMETA_STATE] = 2; meta[FC_QMETA_TICKET] = ticket; meta[FC_QMETA_NTOK] = n_tok; meta[FC_QMETA_NGEN] = gen;
        meta[FC_QMETA_EOS] = gen < q.rows[s].max_steps ? 1 : 0;       // ended below its max_length: on <eos>
        meta[FC_QMETA_SEQ] = fin + at;
        q.qw[FC_QUEUE_SLOT_TICKET + s] = -1;
    }
    const int waiting = claim ? tail - head : 0;
    const bool is_free = valid && (ticket < 0 || ended);
    const unsigned long long free_mask = __ballot(is_free);
    const int at = __popcll(free_mask & below);
    if (is_free && at < waiting) {
        const QueueTicket t = q.ring[(head + at) % q.Q];
        q.claims[at] = QueueClaim{s, t.row, t.P, t.cont_len};
        q.qw[FC_QUEUE_SLOT_TICKET + s] = head + at;
        q.qw[FC_QUEUE_SLOT_ENTRY + s] = t.entry;
        q.n_gen[s] = 0; q.done[s] = 0; q.step[s] = 0; q.pos[s] = t.P; q.tok_off[s] = t.cont_len;
        q.rows[s] = t.srow;
    }
    if (s == 0) {
        const int n_free = __popcll(free_mask), n_claim = n_free < waiting ? n_free : waiting, n_retire = __popcll(ended_mask);
        q.qw[FC_QUEUE_HEAD] = head + n_claim;
        q.qw[FC_QUEUE_FINISHED] = fin + n_retire;
        q.qw[FC_QUEUE_NRETIRE] = n_retire;
        q.qw[FC_QUEUE_NCLAIM] = n_claim;
    }
}

__global__ __launch_bounds__(256) void queue_retire_copy_kernel(QueuePhase q) {
    const int n = q.qw[FC_QUEUE_NRETIRE];
    const int t0 = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    const size_t tok_row = (size_t)q.R * q.nq;                        // int64 per row: even (R % 4 == 0)
    for (int r = 0; r < n; ++r) {
        const QueueRetire rt = q.retires[r];
        const i64x2* ts = (const i64x2*)(q.tokens + (size_t)rt.slot * tok_row);
        i64x2* td = (i64x2*)(q.ring_tokens + (size_t)rt.entry * tok_row);
        const int nv = (rt.n_tok * q.nq + 1) >> 1;                    // <= tok_row / 2
        for (int i = t0; i < nv; i += nth) td[i] = ts[i];
        if (q.score) {
            const f32x4* ss = (const f32x4*)(q.score + (size_t)rt.slot * q.R);
            f32x4* sd = (f32x4*)(q.ring_score + (size_t)rt.entry * q.R);
            for (int i = t0; i < (q.R >> 2); i += nth) sd[i] = ss[i];
        }
    }
}

__global__ __launch_bounds__(256) void queue_claim_copy_kernel(QueuePhase q) {
    const int n = q.qw[FC_QUEUE_NCLAIM];
    const int tid = threadIdx.x;
    if ((int)blockIdx.y == q.NL) {                                    // the rows of slot_reset_kernel and the import's logits
        const int t0 = blockIdx.x * 256 + tid, nth = gridDim.x * 256;
        const size_t tok_row = (size_t)q.R * q.nq;
        for (int c = 0; c < n; ++c) {
            const QueueClaim cl = q.claims[c];
            zero_row(q.xs + (size_t)cl.slot * q.dm, q.dm >> 2, t0, nth);
            const long long nprompt = (long long)cl.cont_len * q.nq;
            const int64_t* ps = q.tokens_src + (size_t)cl.row * q.R_src * q.nq;
            i64x2* td = (i64x2*)(q.tokens + (size_t)cl.slot * tok_row);
            for (int i = t0; i < (int)(tok_row >> 1); i += nth) {
                i64x2 v = {0, 0};
                if (2ll * i < nprompt) v.x = ps[2 * i];
                if (2ll * i + 1 < nprompt) v.y = ps[2 * i + 1];
                td[i] = v;
            }
            if (q.score) zero_row(q.score + (size_t)cl.slot * q.R, q.R >> 2, t0, nth);
            copy_logits(q.lg0_src + (size_t)cl.row * q.V, q.lg + (size_t)cl.slot * q.V, q.lg0 + (size_t)cl.slot * q.V, q.V, t0, nth);
        }
        return;
    }
    const int l = blockIdx.y;
    for (int c = 0; c < n; ++c) {
        const QueueClaim cl = q.claims[c];
        const size_t os = ((size_t)l * q.S_src + cl.row) * q.d * q.R_src, od = ((size_t)l * q.S + cl.slot) * q.d * q.R;
        const int nchunk = kv_chunks(q.d, cl.P);
        for (int chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x)          // prefix_import_kernel's block `chunk` of layer l
            kv_chunk_copy(q.kc_src + os, q.vc_src + os, q.kc + od, q.vc + od, q.R_src, q.R, q.d, cl.P, chunk, tid);
    }
}

static bool queue_phase_ok(const QueuePhase& q) {
    if (!q.qw || !q.ring || !q.claims || !q.retires || q.Q < 1 || q.S < 1 || q.S > 64) return false;
    if (q.R < 4 || q.R % 4 || q.R_src < 4 || q.R_src % 4 || q.nq < 1 || q.d < 4 || q.d % 4 || q.dm < 4 || q.dm % 4 || q.NL < 1 || q.V < 1) return false;
    if ((long long)q.d * q.R > 0x7fffffff || (long long)q.R * q.nq > 0x7fffffff) return false;       // a row's vectors are counted in int
    return q.S_src >= 1 && q.kc && q.vc && q.kc_src && q.vc_src && q.tokens && q.tokens_src && q.ring_tokens && q.lg && q.lg0 && q.lg0_src &&
           (q.score == nullptr) == (q.ring_score == nullptr);
}
hipError_t launch_queue_put(const QueuePhase& q, const QueueTicket& t, int ticket, hipStream_t st) {
    if (!queue_phase_ok(q) || ticket < 0 || t.entry < 0 || t.entry >= q.Q || t.row < 0 || t.row >= q.S_src) return hipErrorInvalidValue;
    // the rows the claim copies: inside both sessions' pitches
    if (t.P < 1 || ((t.P + 3) & ~3) > q.R || ((t.P + 3) & ~3) > q.R_src || t.cont_len < 0 || t.cont_len > t.P) return hipErrorInvalidValue;
    if (t.srow.max_steps < 1 || t.P + t.srow.max_steps > q.R) return hipErrorInvalidValue;
    hipLaunchKernelGGL(queue_put_kernel, dim3(1), dim3(1), 0, st, q, t, ticket);
    return hipGetLastError();
}
hipError_t launch_queue_phase(const QueuePhase& q, int claim, hipStream_t st) {
    if (!queue_phase_ok(q)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(queue_turn_kernel, dim3(1), dim3(64), 0, st, q, claim);
    hipLaunchKernelGGL(queue_retire_copy_kernel, dim3(q.S < 16 ? q.S : 16), dim3(256), 0, st, q);
    if (claim) hipLaunchKernelGGL(queue_claim_copy_kernel, dim3(32, q.NL + 1), dim3(256), 0, st, q);
    return hipGetLastError();
}
hipError_t launch_sample_claims(const Sample& s, const QueuePhase& q, hipStream_t st) {
    if (s.K + 1 > FC_SAMPLE_MAXV || s.nq > 8 || s.nq < 1 || !s.rows || s.logp_out || s.launch_seq) return hipErrorInvalidValue;
    if (s.emb_wt && (s.dm > 1024 || s.dm % 4 || s.D > FC_SAMPLE_MAXV)) return hipErrorInvalidValue;      // as launch_sample
    if (!queue_phase_ok(q) || s.B != q.S) return hipErrorInvalidValue;
    SampleArgs a{s.logits, s.K, s.nq, s.mode, s.ki, s.pf, s.seed, s.forced, s.max_steps, s.tokens, s.tok_stride, s.tok_off, s.n_gen,
                 s.done, s.n_done, s.pos, s.step, s.logp_out, s.score_out, s.cb, s.D, s.next_emb, s.B,
                 s.emb_wt, s.emb_bias, s.emb_g, s.emb_b, s.dm, s.emb_relu, s.xscale, s.xs, s.launch_seq,
                 s.rows, s.row_stride, 0, q.claims, q.qw + FC_QUEUE_NCLAIM};
    hipLaunchKernelGGL(sample_kernel<true>, dim3(q.S), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Slots of a decoding session moved to other rows (fc_laura_slots_move): after the launch row dst of every table line IS row src, and
// row src is a free row (done = 1, as a taken one).  Nothing is computed: every word the session keeps per slot is copied.
//   grid.y = layer l < NL: key / value positions [0, pos[src]] of the layer -- K rows of pad4(pos + 1) floats, the first (pos + 1) * d
//                          floats of V -- in kv_chunk_copy's chunks of FC_PREFIX_VPT x 256 16-byte vectors, the loads of a chunk
//                          in flight together, clamped loads and predicated stores;
//   grid.y = NL:           the token, forced-token (a slot that follows them), score and log-probability rows (the latter as far as the
//                          slot's max_steps, what slot_reset_kernel zeroed and a take reads), the step's and the kept prefix logits, the
//                          pending LM input row and next-embedding row; block 0's thread 0 the counters, the position, the prompt length
//                          and the row of the sampling table, and done[src] = 1.
// The grid is fixed and strides over (table line x chunk), like the queue phase's copy kernels.  The sources and the destinations are
// disjoint sets (checked by the host before the table is written), so no block reads a word another block of the launch writes:
// pos[src] and rows[src] are only read, done[src] is read and written by the one thread.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void slot_moves_put_kernel(int* table, SlotMoveLines l) {
    const int i = threadIdx.x;
    if (i == 0) table[0] = l.n;
    if (i < l.n && i < FC_SLOT_MOVES_MAX) { table[1 + 2 * i] = l.src[i]; table[2 + 2 * i] = l.dst[i]; }
}

__global__ __launch_bounds__(256) void slot_move_kernel(SlotMoves m) {
    int n = m.table[0];
    n = n < FC_SLOT_MOVES_MAX ? n : FC_SLOT_MOVES_MAX;
    const int tid = threadIdx.x;
    if ((int)blockIdx.y == m.NL) {
        const size_t t0 = (size_t)blockIdx.x * 256 + tid, nth = (size_t)gridDim.x * 256;
        const size_t tok_row = (size_t)m.R * m.nq;                        // int64 per row: even (R % 4 == 0)
        for (int c = 0; c < n; ++c) {
            const int src = m.table[1 + 2 * c], dst = m.table[2 + 2 * c];
            const SampleRow* sr = m.rows + src;
            const int max_steps = sr->max_steps < m.R ? sr->max_steps : m.R, forced_on = sr->forced_on;
            const i64x2* ts = (const i64x2*)(m.tokens + (size_t)src * tok_row);
            i64x2* td = (i64x2*)(m.tokens + (size_t)dst * tok_row);
            for (size_t i = t0; i < (tok_row >> 1); i += nth) td[i] = ts[i];
            if (forced_on) {
                const i64x2* fs = (const i64x2*)(m.forced + (size_t)src * tok_row);
                i64x2* fd = (i64x2*)(m.forced + (size_t)dst * tok_row);
                for (size_t i = t0; i < (tok_row >> 1); i += nth) fd[i] = fs[i];
            }
            if (m.score) {
                const f32x4* ss = (const f32x4*)(m.score + (size_t)src * m.R);
                f32x4* sd = (f32x4*)(m.score + (size_t)dst * m.R);
                for (size_t i = t0; i < (size_t)(m.R >> 2); i += nth) sd[i] = ss[i];
            }
            if (m.logp) {                                                 // a row starts at slot * R * V floats: 16-byte aligned (R % 4 == 0)
                const size_t nl = (size_t)(max_steps > 0 ? max_steps : 0) * m.V;
                const float* ls = m.logp + (size_t)src * m.R * m.V;
                float* ld = m.logp + (size_t)dst * m.R * m.V;
                for (size_t i = t0; i < (nl >> 2); i += nth) ((f32x4*)ld)[i] = ((const f32x4*)ls)[i];
                for (size_t i = (nl & ~(size_t)3) + t0; i < nl; i += nth) ld[i] = ls[i];
            }
            for (size_t v = t0; v < (size_t)m.V; v += nth) {              // V need not be a multiple of 4: scalar, 2 x V floats
                m.lg[(size_t)dst * m.V + v] = m.lg[(size_t)src * m.V + v];
                m.lg0[(size_t)dst * m.V + v] = m.lg0[(size_t)src * m.V + v];
            }
            for (size_t i = t0; i < (size_t)(m.d >> 2); i += nth)
                ((f32x4*)(m.xs + (size_t)dst * m.d))[i] = ((const f32x4*)(m.xs + (size_t)src * m.d))[i];
            for (size_t i = t0; i < (size_t)m.D; i += nth) m.nemb[(size_t)dst * m.D + i] = m.nemb[(size_t)src * m.D + i];
            if (t0 == 0) {
                m.n_gen[dst] = m.n_gen[src]; m.done[dst] = m.done[src]; m.step[dst] = m.step[src]; m.pos[dst] = m.pos[src];
                m.tok_off[dst] = m.tok_off[src];
                m.rows[dst] = *sr;
                m.done[src] = 1;
            }
        }
        return;
    }
    const int l = blockIdx.y;
    const size_t row = (size_t)m.d * m.Tcap;                             // floats of one slot's row of a layer, K and V alike
    for (int c = 0; c < n; ++c) {
        const int src = m.table[1 + 2 * c], dst = m.table[2 + 2 * c];
        int P = m.pos[src] + 1;                                           // positions [0, pos]
        P = P < 1 ? 1 : (P > m.Tcap ? m.Tcap : P);                        // pad4(P) <= Tcap (Tcap % 4 == 0)
        const size_t os = ((size_t)l * m.S + src) * row, od = ((size_t)l * m.S + dst) * row;
        const int nchunk = kv_chunks(m.d, P);
        for (int chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x)
            kv_chunk_copy(m.kc + os, m.vc + os, m.kc + od, m.vc + od, m.Tcap, m.Tcap, m.d, P, chunk, tid);
    }
}

hipError_t launch_slot_moves(const SlotMoves& m, const SlotMoveLines& lines, hipStream_t st) {
    if (!m.table || !m.kc || !m.vc || !m.n_gen || !m.done || !m.step || !m.pos || !m.tok_off || !m.rows || !m.tokens || !m.forced || !m.lg ||
        !m.lg0 || !m.xs || !m.nemb)
        return hipErrorInvalidValue;
    if (m.NL < 1 || m.S < 2 || m.S > 64 || m.d < 4 || m.d % 4 || m.Tcap < 4 || m.Tcap % 4 || m.R != m.Tcap || m.V < 1 || m.nq < 1 || m.D < 1)
        return hipErrorInvalidValue;
    if ((long long)m.d * m.Tcap > 0x7fffffff) return hipErrorInvalidValue;       // a row's vectors are counted in int
    if (lines.n < 1 || lines.n > FC_SLOT_MOVES_MAX || lines.n > m.S) return hipErrorInvalidValue;
    unsigned long long srcs = 0, dsts = 0;                                        // distinct rows, disjoint sides
    for (int i = 0; i < lines.n; ++i) {
        const int a = lines.src[i], b = lines.dst[i];
        if (a < 0 || a >= m.S || b < 0 || b >= m.S) return hipErrorInvalidValue;
        if (((srcs | dsts) >> a & 1ull) || ((srcs | dsts) >> b & 1ull) || a == b) return hipErrorInvalidValue;
        srcs |= 1ull << a; dsts |= 1ull << b;
    }
    hipLaunchKernelGGL(slot_moves_put_kernel, dim3(1), dim3(64), 0, st, m.table, lines);
    hipLaunchKernelGGL(slot_move_kernel, dim3(64, m.NL + 1), dim3(256), 0, st, m);
    return hipGetLastError();
}

}  // namespace laura
}  // namespace fc
