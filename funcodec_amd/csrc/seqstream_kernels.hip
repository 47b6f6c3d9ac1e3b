// gfx950 (MI355X / CDNA4) attention of a streaming push of the SEANet transformer bottleneck (seq_kernels.h, SeqAttnCached): the
// push's n queries (1 .. 25 frames, typically) against the keys and values of everything the utterance has pushed so far, which live
// in the session's cache.  Query i of a push that begins at frame `pos` sees keys 0 .. pos + i (transformer.py:172-177).
//
// The arithmetic is seq_attn_kernel's (seq_kernels.hip): both products on v_mfma_f32_16x16x4_f32 in the transposed orientation (the
// query on the lane), exact online softmax in fp32, a masked key has probability exactly 0 and stays out of the running maximum.  What
// differs is the split of the work.  Attention with few queries is bound by the read of K and V, and one wave walking 1500 keys alone
// would leave the device idle, so the 16-key tiles a query tile can see are dealt out in contiguous runs to `units` waves
// (seq_attn_cached_units).  Every unit writes its partial (m, l, O) to a workspace buffer and seq_attn_merge_kernel folds the units by
// the log-sum-exp rule in unit order: no atomics, so a result is a function of (inputs, pos, n) alone.  A push of more than
// kSeqCachedSplitMaxQueries frames has enough query tiles to fill the device by itself: units = 1, the wave normalises and stores its
// own result and nothing is merged.
//
// Bounds: a key index is clamped to kend - 1 < pos + n before every load, and a tile that reaches past kend loads V element by element
// through the same clamp, so what lies behind pos + n in the cache (stale frames of an earlier utterance, anything at all) never reaches
// a register that an MFMA reads, and no load leaves a cache row.
//
// A slot push (seq_kernels.h, SeqAttnRows) runs the same unit per row: seq_attn_rows_kernel reads every row's own (n_b, pos_b) from the
// push's table and deals the row's work exactly as a one-row lock-step push (n_b, pos_b) deals it, so one launch holds rows of both
// forms and idle rows, and a row's result does not depend on the rows beside it.
#include "seq_kernels.h"
#include "device_common.h"

namespace fc {

namespace {

// partial of unit u of (row b, head h): [DK + 2][16 queries]: rows 0 .. DK - 1 the unnormalised O^T, row DK the running maximum m,
// row DK + 1 the sum of exponentials l
//
// The work of one wave, stated once for the lock-step kernel and the row-wise one: unit u of `units` of query tile i0 / 16 of one
// (row, head).  qb: the head's q rows of the chunk (pitch nz), kb / vb: its cache rows (pitch Fz), ob: its rows of `out` (pitch
// nz), part: the partials, this unit's at slot pslot + u, or null when the wave normalises and stores its own result.
template <int DK>
__device__ __forceinline__ void seq_attn_cached_unit(const float* __restrict__ qb, const float* __restrict__ kb, const float* __restrict__ vb,
                                                     float* __restrict__ ob, float* __restrict__ part, size_t pslot, int n, size_t nz, int pos,
                                                     size_t Fz, int units, int u, int i0, float scale) {
    constexpr int NC = DK / 4;     // k steps of Q . K (4 dims each)
    constexpr int ND = DK / 16;    // 16-dim tiles of the output
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    const int iq = i0 + r;                                   // this lane's query (rows past n are computed on a clamped copy, not written)
    const int iqc = iq < n ? iq : n - 1;
    float qf[NC];                                            // B operand of step c: Q[query r][dim 4 c + g]
#pragma unroll
    for (int c = 0; c < NC; ++c) qf[c] = qb[(size_t)(4 * c + g) * nz + iqc];
    f32x4 o[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float NEG_INF = -__builtin_inff();
    float m = NEG_INF, l = 0.f;
    const int kend = pos + (i0 + 16 < n ? i0 + 16 : n);      // keys [0, kend) are visible to some query of the tile; kend <= pos + n <= F
    const int tiles = (kend + 15) >> 4, per = (tiles + units - 1) / units;
    const int t0 = u * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    for (int j0 = t0 * 16; j0 < t1 * 16; j0 += 16) {
        const int jk = j0 + r < kend ? j0 + r : kend - 1;
        // ---- S^T = K . Q^T (two accumulation chains, as seq_attn_kernel)
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
        for (int c = 0; c < NC; c += 2) {
            s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[(size_t)(4 * c + g) * Fz + jk], qf[c], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[(size_t)(4 * c + 4 + g) * Fz + jk], qf[c + 1], s1, 0, 0, 0);
        }
        // ---- online softmax: lane (g, r) holds keys j0 + 4 g + v of query r
        float p[4];
        unsigned vis = 0;
        float tmax = NEG_INF;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + 4 * g + v;
            const bool ok = j < kend && j <= pos + iq;
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
        const bool full = j0 + 16 <= kend;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const float* vrow = vb + (size_t)(16 * d + r) * Fz;
            f32x4 vv;
            if (full) {
                vv = *(const f32x4*)(vrow + j0 + 4 * g);     // F % 16 == 0 and the caches are 16-byte aligned
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int j = j0 + 4 * g + v;
                    vv[v] = vrow[j < kend ? j : kend - 1];   // finite stand-in for a key behind the push: its probability is exactly 0
                }
            }
            o[d] *= alpha;
#pragma unroll
            for (int v = 0; v < 4; ++v) o[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[v], p[v], o[d], 0, 0, 0);
        }
    }
    if (part) {                                              // the few-query form: one query tile, the merge normalises
        float* pb = part + (pslot + u) * (size_t)(DK + 2) * 16;
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int v = 0; v < 4; ++v) pb[(16 * d + 4 * g + v) * 16 + r] = o[d][v];
        if (g == 0) { pb[DK * 16 + r] = m; pb[(DK + 1) * 16 + r] = l; }
        return;
    }
    if (iq >= n) return;
    const float inv = 1.f / l;
    ob += iq;
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int v = 0; v < 4; ++v) ob[(size_t)(16 * d + 4 * g + v) * nz] = o[d][v] * inv;
}

template <int DK>
__global__ __launch_bounds__(256) void seq_attn_cached_kernel(const float* __restrict__ qkv, const float* __restrict__ kc,
                                                              const float* __restrict__ vc, float* __restrict__ out, float* __restrict__ part,
                                                              int H, int n, int pos, int F, int units, float scale) {
    const int w = threadIdx.x >> 6;
    const int QT = (n + 15) >> 4;
    const int unit = blockIdx.x * 4 + w;                     // (query tile, unit of its keys)
    if (unit >= QT * units) return;
    const int qt = unit / units, u = unit - qt * units;
    const int h = blockIdx.y, b = blockIdx.z, C = H * DK;
    const size_t nz = (size_t)n, Fz = (size_t)F;
    const size_t kr = ((size_t)b * C + (size_t)h * DK);
    seq_attn_cached_unit<DK>(qkv + ((size_t)b * 3 * C + (size_t)h * DK) * nz, kc + kr * Fz, vc + kr * Fz, out + kr * nz,
                             part, ((size_t)b * H + h) * units, n, nz, pos, Fz, units, u, qt * 16, scale);
}

// The row-wise form (seq_kernels.h, SeqAttnRows): row b = blockIdx.z reads its own (n_b, pos_b) once -- a uniform address, so both are
// scalars of the wave -- and its waves do what the lock-step kernel's waves do for a one-row push (n_b, pos_b); a wave beyond its row's
// work exits, and so does every wave of a row whose (n_b, pos_b) would leave the chunk or the cache (the host refuses such a push before
// it is enqueued; this is the device's own bound).
template <int DK>
__global__ __launch_bounds__(256) void seq_attn_rows_kernel(const float* __restrict__ qkv, const float* __restrict__ kc,
                                                            const float* __restrict__ vc, float* __restrict__ out, float* __restrict__ part,
                                                            const int* __restrict__ lens, int div, int mul, int add,
                                                            const int* __restrict__ posv, int H, int T, int F, float scale) {
    const int w = threadIdx.x >> 6;
    const int h = blockIdx.y, b = blockIdx.z, C = H * DK;
    const int len = lens[b];
    const int n = len > 0 ? ragged_cols(len, div, mul, add) : 0, pos = posv[b];
    if (n < 1 || n > T || pos < 0 || pos > F - n) return;
    const int QT = (n + 15) >> 4;
    const int units = seq_attn_cached_units(n, pos);
    const int unit = blockIdx.x * 4 + w;
    if (unit >= QT * units) return;
    const int qt = unit / units, u = unit - qt * units;
    const size_t Tz = (size_t)T, Fz = (size_t)F;
    const size_t kr = ((size_t)b * C + (size_t)h * DK);
    const bool split = n <= kSeqCachedSplitMaxQueries;
    seq_attn_cached_unit<DK>(qkv + ((size_t)b * 3 * C + (size_t)h * DK) * Tz, kc + kr * Fz, vc + kr * Fz, out + kr * Tz,
                             split ? part : nullptr, ((size_t)b * H + h) * kSeqCachedMaxUnits, n, Tz, pos, Fz, units, u, qt * 16, scale);
}

// The units of one (row, head) folded in unit order: M = max m_u;  out = sum_u O_u exp(m_u - M) / sum_u l_u exp(m_u - M).  A unit none
// of whose keys a query sees has m = -inf, l = 0 and weighs exactly 0; unit 0 holds key 0, which every query sees, so M is finite.
// One thread per output (query, dim); the loops over the units are unrolled to kSeqCachedMaxUnits so that the loads of all units are
// in flight together (a rolled loop waits for one load per unit, which made the merge cost more than the attention itself).
__device__ __forceinline__ float seq_attn_merge_one(const float* __restrict__ pb, size_t stride, int DK, int units, int d, int q) {
    const float NEG_INF = -__builtin_inff();
    float mu[kSeqCachedMaxUnits], lu[kSeqCachedMaxUnits], ou[kSeqCachedMaxUnits];
#pragma unroll
    for (int u = 0; u < kSeqCachedMaxUnits; ++u) {
        const bool live = u < units;
        const float* pu = pb + (live ? u : 0) * stride;
        mu[u] = live ? pu[DK * 16 + q] : NEG_INF;
        lu[u] = live ? pu[(DK + 1) * 16 + q] : 0.f;
        ou[u] = live ? pu[d * 16 + q] : 0.f;
    }
    float M = NEG_INF;
#pragma unroll
    for (int u = 0; u < kSeqCachedMaxUnits; ++u) M = fmaxf(M, mu[u]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int u = 0; u < kSeqCachedMaxUnits; ++u) {
        const float wgt = mu[u] == NEG_INF ? 0.f : expf(mu[u] - M);
        L += lu[u] * wgt;
        O += ou[u] * wgt;
    }
    return O / L;
}

__global__ __launch_bounds__(256) void seq_attn_merge_kernel(const float* __restrict__ part, float* __restrict__ out, int H, int DK, int n,
                                                             int units) {
    const int h = blockIdx.x, b = blockIdx.y, C = H * DK;
    const size_t stride = (size_t)(DK + 2) * 16;
    const float* pb = part + ((size_t)b * H + h) * units * stride;
    const int idx = blockIdx.z * 256 + threadIdx.x;
    const int q = idx & 15, d = idx >> 4;
    if (d >= DK || q >= n) return;
    out[((size_t)b * C + (size_t)h * DK + d) * n + q] = seq_attn_merge_one(pb, stride, DK, units, d, q);
}

// The second launch of the row-wise form, one thread per (query of a tile, dim) of every (row, head): the merge of a split row, with the
// row's own unit count, and for every row -- split, unsplit or idle -- the zeros of the columns [n_b, T) of `out`, which no other wave
// writes.  Thread q zeroes the columns n_b + q, n_b + q + 16, ...; the attention kernel's stores end at column n_b - 1.
__global__ __launch_bounds__(256) void seq_attn_rows_merge_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                  const int* __restrict__ lens, int div, int mul, int add,
                                                                  const int* __restrict__ posv, int H, int DK, int T, int F) {
    const int h = blockIdx.x, b = blockIdx.y, C = H * DK;
    const int idx = blockIdx.z * 256 + threadIdx.x;
    const int q = idx & 15, d = idx >> 4;
    if (d >= DK) return;
    const int len = lens[b], pos = posv[b];
    int n = len > 0 ? ragged_cols(len, div, mul, add) : 0;
    if (n > T || pos < 0 || pos > F - n) n = 0;               // a row the attention kernel refused: all zeros
    float* orow = out + ((size_t)b * C + (size_t)h * DK + d) * T;
    if (n > 0 && n <= kSeqCachedSplitMaxQueries && q < n) {
        const size_t stride = (size_t)(DK + 2) * 16;
        orow[q] = seq_attn_merge_one(part + ((size_t)b * H + h) * kSeqCachedMaxUnits * stride, stride, DK, seq_attn_cached_units(n, pos), d, q);
    }
    for (int t = n + q; t < T; t += 16) orow[t] = 0.f;
}

__global__ __launch_bounds__(256) void seq_cache_append_kernel(const float* __restrict__ qkv, float* __restrict__ kc, float* __restrict__ vc,
                                                               int B, int C, int n, int pos, int F) {
    const size_t total = (size_t)B * 2 * C * n;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int t = (int)(idx % n);
    const size_t row = idx / n;
    const int b = (int)(row / (2 * C)), rc = (int)(row % (2 * C));
    const float v = qkv[((size_t)b * 3 * C + C + rc) * n + t];
    float* dst = rc < C ? kc : vc;
    dst[((size_t)b * C + (rc < C ? rc : rc - C)) * F + pos + t] = v;
}

// the row-wise append: row b's first n_b columns (pitch T) to frames [pos_b, pos_b + n_b) of its own cache rows; n_b == 0 writes nothing
__global__ __launch_bounds__(256) void seq_cache_append_rows_kernel(const float* __restrict__ qkv, float* __restrict__ kc, float* __restrict__ vc,
                                                                    const int* __restrict__ lens, int div, int mul, int add,
                                                                    const int* __restrict__ posv, int S, int C, int T, int F) {
    const size_t total = (size_t)S * 2 * C * T;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int t = (int)(idx % T);
    const size_t row = idx / T;
    const int b = (int)(row / (2 * C)), rc = (int)(row % (2 * C));
    const int len = lens[b], pos = posv[b];
    const int n = len > 0 ? ragged_cols(len, div, mul, add) : 0;
    if (t >= n || n > T || pos < 0 || pos > F - n) return;
    const float v = qkv[((size_t)b * 3 * C + C + rc) * T + t];
    float* dst = rc < C ? kc : vc;
    dst[((size_t)b * C + (rc < C ? rc : rc - C)) * F + pos + t] = v;
}

template <int DK>
void enqueue_cached(const SeqAttnCached& a, int units, float* part, hipStream_t st) {
    const int QT = (a.n + 15) / 16;
    const dim3 grid((QT * units + 3) / 4, a.H, a.B), block(256);
    const float scale = 1.f / sqrtf((float)DK);
    hipLaunchKernelGGL(seq_attn_cached_kernel<DK>, grid, block, 0, st, a.qkv, a.kc, a.vc, a.out, part, a.H, a.n, a.pos, a.F, units, scale);
}

template <int DK>
void enqueue_rows(const SeqAttnRows& a, hipStream_t st) {
    const SeqRows& r = a.rows;
    const dim3 grid((r.max_waves + 3) / 4, a.H, r.S), block(256);
    const float scale = 1.f / sqrtf((float)DK);
    hipLaunchKernelGGL(seq_attn_rows_kernel<DK>, grid, block, 0, st, a.qkv, a.kc, a.vc, a.out, a.part, r.len.lens, r.len.div, r.len.mul, r.len.add,
                       r.pos, a.H, r.T, r.F, scale);
}

bool rows_ok(const SeqRows& r) {
    return r.len.lens && r.pos && r.S >= 1 && r.S <= 65535 && r.T >= 1 && r.F >= 16 && !(r.F & 15) && r.len.div >= 1 && r.max_waves >= 0 &&
           r.max_waves <= (r.T + 15) / 16 * kSeqCachedMaxUnits;
}

}  // namespace

const char* seq_attn_cached_kernel_name(int DK) {
    switch (DK) {
        case 16: return "seq_attn_cached_kernel<16>";
        case 32: return "seq_attn_cached_kernel<32>";
        case 64: return "seq_attn_cached_kernel<64>";
        case 128: return "seq_attn_cached_kernel<128>";
        default: return "seq_attn_cached_kernel<256>";
    }
}

hipError_t launch_seq_attn_cached(const SeqAttnCached& a, hipStream_t st) {
    if (!a.qkv || !a.kc || !a.vc || !a.out || a.B < 1 || a.H < 1 || a.n < 1 || a.pos < 0 || !seq_attn_supported(a.DK)) return hipErrorInvalidValue;
    if ((a.F & 15) || (long long)a.pos + a.n > a.F || (((uintptr_t)a.kc | (uintptr_t)a.vc) & 15)) return hipErrorInvalidValue;
    const bool split = a.n <= kSeqCachedSplitMaxQueries;
    if (split && !a.part) return hipErrorInvalidValue;
    const int units = seq_attn_cached_units(a.n, a.pos);
    float* part = split ? a.part : nullptr;
    switch (a.DK) {
        case 16: enqueue_cached<16>(a, units, part, st); break;
        case 32: enqueue_cached<32>(a, units, part, st); break;
        case 64: enqueue_cached<64>(a, units, part, st); break;
        case 128: enqueue_cached<128>(a, units, part, st); break;
        default: enqueue_cached<256>(a, units, part, st); break;
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !split) return err;
    hipLaunchKernelGGL(seq_attn_merge_kernel, dim3(a.H, a.B, (a.DK * 16 + 255) / 256), dim3(256), 0, st, a.part, a.out, a.H, a.DK, a.n, units);
    return hipGetLastError();
}

const char* seq_attn_rows_kernel_name(int DK) {
    switch (DK) {
        case 16: return "seq_attn_rows_kernel<16>";
        case 32: return "seq_attn_rows_kernel<32>";
        case 64: return "seq_attn_rows_kernel<64>";
        case 128: return "seq_attn_rows_kernel<128>";
        default: return "seq_attn_rows_kernel<256>";
    }
}

hipError_t launch_seq_attn_rows(const SeqAttnRows& a, hipStream_t st) {
    const SeqRows& r = a.rows;
    if (!a.qkv || !a.kc || !a.vc || !a.out || !a.part || a.H < 1 || !seq_attn_supported(a.DK) || !rows_ok(r)) return hipErrorInvalidValue;
    if ((((uintptr_t)a.kc | (uintptr_t)a.vc) & 15)) return hipErrorInvalidValue;
    if (r.max_waves > 0) {
        switch (a.DK) {
            case 16: enqueue_rows<16>(a, st); break;
            case 32: enqueue_rows<32>(a, st); break;
            case 64: enqueue_rows<64>(a, st); break;
            case 128: enqueue_rows<128>(a, st); break;
            default: enqueue_rows<256>(a, st); break;
        }
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(seq_attn_rows_merge_kernel, dim3(a.H, r.S, (a.DK * 16 + 255) / 256), dim3(256), 0, st, a.part, a.out, r.len.lens, r.len.div,
                       r.len.mul, r.len.add, r.pos, a.H, a.DK, r.T, r.F);
    return hipGetLastError();
}

hipError_t launch_seq_cache_append_rows(const SeqCacheAppendRows& a, hipStream_t st) {
    const SeqRows& r = a.rows;
    if (!a.qkv || !a.kc || !a.vc || a.C < 1 || !rows_ok(r)) return hipErrorInvalidValue;
    const size_t total = (size_t)r.S * 2 * a.C * r.T;
    hipLaunchKernelGGL(seq_cache_append_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.qkv, a.kc, a.vc, r.len.lens,
                       r.len.div, r.len.mul, r.len.add, r.pos, r.S, a.C, r.T, r.F);
    return hipGetLastError();
}

hipError_t launch_seq_cache_append(const SeqCacheAppend& a, hipStream_t st) {
    if (!a.qkv || !a.kc || !a.vc || a.B < 1 || a.C < 1 || a.n < 1 || a.pos < 0 || (long long)a.pos + a.n > a.F) return hipErrorInvalidValue;
    const size_t total = (size_t)a.B * 2 * a.C * a.n;
    hipLaunchKernelGGL(seq_cache_append_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.qkv, a.kc, a.vc, a.B, a.C, a.n, a.pos, a.F);
    return hipGetLastError();
}

}  // namespace fc
