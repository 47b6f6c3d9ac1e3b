// Length-aware (ragged) pass (fc_*_ragged): the kernels that respect a row's own end.  See ragged_kernels.h for the contract.
// All of them are LDS-free streaming kernels (the reductions keep a few doubles in LDS), vector stores only, no atomics: every element
// has exactly one writer, and every summation order depends on the row's own length alone, never on the batch around it.
#include "ragged_kernels.h"
#include "device_common.h"

namespace fc {

namespace {

__global__ __launch_bounds__(256) void ragged_lengths_kernel(const int32_t* __restrict__ in, int B, int Tmax, int* __restrict__ lens,
                                                             unsigned* status) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int v = in[b];
    const int c = v < 1 ? 1 : (v > Tmax ? Tmax : v);
    lens[b] = c;
    if (c != v && status) status[FC_STATUS_BAD_LENGTH] = 1u;
}

struct StageArgs {
    const float *s0, *a0, *div, *s1, *a1;
    float* buf;
    const int* lens;
    int ldiv, lmul, ladd;
    int C, ld0, ld1, Tp, k, pt, stride, causal, transposed, elu;
    float alpha;
};

constexpr int kStageSeg = 2048;      // staged columns per workgroup row

// One workgroup = one (utterance, channel quad, column segment), one wave per channel row; a lane takes four staged columns at a time: where
// all four are the row's own columns they move as one 16-byte load and one 16-byte store (dword-aligned vector accesses), the padding
// columns and the row's end as single dwords.
__global__ __launch_bounds__(256) void ragged_stage_kernel(const StageArgs p) {
    const int lane = threadIdx.x & 63, c = 4 * blockIdx.x + (threadIdx.x >> 6), b = blockIdx.y;
    if (c >= p.C) return;
    const int n = ragged_cols(p.lens[b], p.ldiv, p.lmul, p.ladd);
    int padL, padR, Leff;
    if (p.transposed) { padL = 1; padR = 0; Leff = n; }
    else {
        padL = p.causal ? p.pt : p.pt - p.pt / 2;
        padR = (p.causal ? 0 : p.pt / 2) + ragged_extra(n, p.k, p.pt, p.stride);
        const int maxpad = padL > padR ? padL : padR;
        Leff = n > maxpad ? n : maxpad + 1;      // pad1d zero-extends a row not longer than the padding before it reflects
    }
    const size_t row = (size_t)b * p.C + c;
    const float* x0 = p.s0 + row * p.ld0;
    const float* x1 = p.s1 ? p.s1 + row * p.ld1 : nullptr;
    float* out = p.buf + row * p.Tp;
    const float dv = p.div ? p.div[b] : 1.f;
    const float2 A0 = p.a0 ? ((const float2*)p.a0)[row] : make_float2(1.f, 0.f);
    const float2 A1 = p.a1 ? ((const float2*)p.a1)[row] : make_float2(1.f, 0.f);
    auto act = [&](float v, float w) __attribute__((always_inline)) {
        if (p.a0) v = fmaf(v, A0.x, A0.y);
        if (p.div) v = v / dv;
        if (x1) v = v + (p.a1 ? fmaf(w, A1.x, A1.y) : w);
        if (p.elu) v = elu_f(v, p.alpha);
        return v;
    };
    auto col = [&](int q) __attribute__((always_inline)) {      // staged column q
        const int rel = q - padL;
        if (rel >= n + padR) return 0.f;
        int src = rel < 0 ? -rel : rel;
        if (!p.transposed && src >= Leff) src = 2 * (Leff - 1) - src;
        if (src < 0 || src >= n || (p.transposed && rel < 0)) return 0.f;
        return act(x0[src], x1 ? x1[src] : 0.f);
    };
    const int q_end = min(p.Tp, (int)(blockIdx.z + 1) * kStageSeg);
    for (int q0 = blockIdx.z * kStageSeg + 4 * lane; q0 < q_end; q0 += 256) {
        const int rel = q0 - padL;
        if (rel >= 0 && rel + 3 < n && q0 + 3 < q_end) {
            const f32x4 a = *(const f32x4u*)(x0 + rel);
            const f32x4 w = x1 ? (f32x4)(*(const f32x4u*)(x1 + rel)) : a;
            f32x4 y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = act(a[j], w[j]);
            *(f32x4u*)(out + q0) = y;
        } else {
            for (int j = 0; j < 4 && q0 + j < q_end; ++j) out[q0 + j] = col(q0 + j);
        }
    }
}

constexpr int kGnSeg = 4096;         // columns per partial: fixed, so that a row's summation order does not depend on the batch's width

// one wave per (utterance, channel, segment): fp64 sums of x and x^2 over the segment's valid columns, lanes strided, then a butterfly
__global__ __launch_bounds__(256) void ragged_gn_partials_kernel(const float* __restrict__ x, int C, int ld, int nseg, const int* __restrict__ lens,
                                                                 int ldiv, int lmul, int ladd, double* __restrict__ partials) {
    const int lane = threadIdx.x & 63, c = 4 * blockIdx.x + (threadIdx.x >> 6), b = blockIdx.y, sg = blockIdx.z;
    if (c >= C) return;
    const int n = ragged_cols(lens[b], ldiv, lmul, ladd);
    const int t0 = sg * kGnSeg, t1 = min(n, t0 + kGnSeg);
    if (t0 >= n) return;
    const float* r = x + ((size_t)b * C + c) * ld;
    double s1 = 0.0, s2 = 0.0;
    for (int t = t0 + lane; t < t1; t += 64) {
        const double v = (double)r[t];
        s1 += v; s2 += v * v;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
        const size_t slot = (((size_t)b * C + c) * nseg + sg) * 2;
        partials[slot] = s1; partials[slot + 1] = s2;
    }
}

__global__ __launch_bounds__(256) void ragged_gn_finalize_kernel(const double* __restrict__ partials, int C, int nseg, const int* __restrict__ lens,
                                                                 int ldiv, int lmul, int ladd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, float* __restrict__ aff) {
    __shared__ double sh[2][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = ragged_cols(lens[b], ldiv, lmul, ladd);
    const int ns = (n + kGnSeg - 1) / kGnSeg;                  // the row's own segments
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < C * ns; i += 256) {
        const size_t slot = (((size_t)b * C + i / ns) * nseg + i % ns) * 2;
        s1 += partials[slot]; s2 += partials[slot + 1];
    }
    sh[0][tid] = s1; sh[1][tid] = s2;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) { sh[0][tid] += sh[0][tid + o]; sh[1][tid] += sh[1][tid + o]; }
        __syncthreads();
    }
    const double count = (double)C * (double)n;
    const double mean = sh[0][0] / count;
    double var = sh[1][0] / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float meanf = (float)mean;
    for (int c = tid; c < C; c += 256) {
        const float a = rstd * gamma[c];
        ((float2*)aff)[(size_t)b * C + c] = make_float2(a, fmaf(-a, meanf, beta[c]));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ragged_mask_kernel(T* __restrict__ p, int B, int M, int Tn, int Dn, size_t total, const int* __restrict__ lens,
                                                          int ldiv, int lmul, int ladd) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / Dn;
        const int t = (int)(r % Tn);
        const int b = (int)((r / Tn / M) % B);
        if (t >= ragged_cols(lens[b], ldiv, lmul, ladd)) p[i] = (T)0;
    }
}

template <typename T>
hipError_t launch_mask(T* p, int O, int B, int M, int Tn, int Dn, const RagLen& len, hipStream_t st) {
    if (O <= 0 || B <= 0 || M <= 0 || Tn <= 0 || Dn <= 0 || !len.lens) return hipErrorInvalidValue;
    const size_t total = (size_t)O * B * M * Tn * Dn;
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(ragged_mask_kernel<T>, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, p, B, M, Tn, Dn, total, len.lens,
                       len.div, len.mul, len.add);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ragged_lengths(const int32_t* in, int B, int Tmax, int* lens, unsigned* status, hipStream_t st) {
    if (B <= 0 || Tmax <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ragged_lengths_kernel, dim3((B + 255) / 256), dim3(256), 0, st, in, B, Tmax, lens, status);
    return hipGetLastError();
}

hipError_t launch_ragged_stage(const RaggedStage& s, hipStream_t st) {
    // Tp holds the longest row with its padding: the row's columns and its right padding end at padL + ceil(n / stride) * stride at most
    if (s.B <= 0 || s.B > 65535 || s.C <= 0 || s.Tin <= 0 || s.pt < 0 || s.stride < 1 || !s.len.lens || s.s1.div) return hipErrorInvalidValue;
    if (s.transposed ? s.Tp < s.Tin + 2 : s.Tp < s.pt + s.Tin + ragged_extra(s.Tin, s.k, s.pt, s.stride)) return hipErrorInvalidValue;
    StageArgs a;
    a.s0 = s.s0.ptr; a.a0 = s.s0.aff; a.div = s.s0.div; a.s1 = s.s1.ptr; a.a1 = s.s1.aff; a.buf = s.buf;
    a.lens = s.len.lens; a.ldiv = s.len.div; a.lmul = s.len.mul; a.ladd = s.len.add;
    a.C = s.C; a.ld0 = s.s0.ld ? s.s0.ld : s.Tin; a.ld1 = s.s1.ld ? s.s1.ld : s.Tin; a.Tp = s.Tp;
    a.k = s.k; a.pt = s.pt; a.stride = s.stride; a.causal = s.causal; a.transposed = s.transposed; a.elu = s.elu; a.alpha = s.alpha;
    hipLaunchKernelGGL(ragged_stage_kernel, dim3((s.C + 3) / 4, s.B, (s.Tp + kStageSeg - 1) / kStageSeg), dim3(256), 0, st, a);
    return hipGetLastError();
}

int ragged_gn_segments(int cols) { return (cols + kGnSeg - 1) / kGnSeg; }

hipError_t launch_ragged_gn_partials(const float* x, int B, int C, int ld, const RagLen& len, double* partials, hipStream_t st) {
    if (B <= 0 || B > 65535 || C <= 0 || ld <= 0 || !len.lens) return hipErrorInvalidValue;
    const int nseg = ragged_gn_segments(ld);
    if (nseg > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ragged_gn_partials_kernel, dim3((C + 3) / 4, B, nseg), dim3(256), 0, st, x, C, ld, nseg, len.lens, len.div, len.mul, len.add,
                       partials);
    return hipGetLastError();
}

hipError_t launch_ragged_gn_finalize(const double* partials, int B, int C, int ld, const RagLen& len, const float* gamma, const float* beta,
                                     float eps, float* aff, hipStream_t st) {
    if (B <= 0 || C <= 0 || ld <= 0 || !len.lens) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ragged_gn_finalize_kernel, dim3(B), dim3(256), 0, st, partials, C, ragged_gn_segments(ld), len.lens, len.div, len.mul, len.add,
                       gamma, beta, eps, aff);
    return hipGetLastError();
}

hipError_t launch_ragged_mask_f32(float* p, int O, int B, int M, int T, int Dn, const RagLen& len, hipStream_t st) {
    return launch_mask<float>(p, O, B, M, T, Dn, len, st);
}
hipError_t launch_ragged_mask_i64(int64_t* p, int O, int B, int M, int T, int Dn, const RagLen& len, hipStream_t st) {
    return launch_mask<int64_t>(p, O, B, M, T, Dn, len, st);
}

}  // namespace fc
