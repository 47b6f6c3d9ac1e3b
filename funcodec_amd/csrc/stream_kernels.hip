// Streaming session (fc_stream_*): the staging pass in front of every causal conv of a push.  See stream_kernels.h for the contract.
#include "stream_kernels.h"
#include "device_common.h"

namespace fc {

namespace {

struct StageArgs {
    const float *s0, *s1, *div, *carry_in;
    float *carry_out, *buf;
    int C, Tc, pt, padR, left, elu;
    float alpha;
};

// One workgroup = one (utterance, channel quad) row band, one wave per channel row; the lanes sweep the row's columns: the chunk body
// moves in 16-byte pieces (dword-aligned vector accesses, which global memory takes), the few context / padding / carry columns as
// single dwords, reflected ones in descending order.  A one-frame push at the deep layers keeps only pt + 1 lanes of a wave busy, which
// does not matter while a push is bound by its launches.  Vector stores only, no atomics: every column has exactly one writer.
__global__ __launch_bounds__(256) void stream_stage_kernel(const StageArgs p) {
    const int lane = threadIdx.x & 63, c = 4 * blockIdx.x + (threadIdx.x >> 6), b = blockIdx.y;
    if (c >= p.C) return;
    const int Tc = p.Tc, pt = p.pt, Tp = pt + Tc + p.padR;
    const size_t row = (size_t)b * p.C + c;
    const float* x0 = p.s0 + row * Tc;
    const float* x1 = p.s1 ? p.s1 + row * Tc : nullptr;
    const float* cin = p.carry_in + row * pt;
    float* cout = p.carry_out + row * pt;
    float* out = p.buf + row * Tp;
    const float dv = p.div ? p.div[b] : 1.f;
    auto act = [&](float v, float w) __attribute__((always_inline)) {
        if (p.div) v = v / dv;
        if (x1) v = v + w;
        if (p.elu) v = elu_f(v, p.alpha);
        return v;
    };
    auto chunk_at = [&](int t) __attribute__((always_inline)) { return act(x0[t], x1 ? x1[t] : 0.f); };
    // column q of [left context | chunk]
    auto left_at = [&](int q) __attribute__((always_inline)) {
        if (p.left == 0) return cin[q];
        const int src = pt - q;                               // reflection about chunk column 0; a chunk shorter than that reads as zero-extended
        return (p.left == 1 && src < Tc) ? chunk_at(src) : 0.f;
    };
    auto concat_at = [&](int q) __attribute__((always_inline)) { return q < pt ? left_at(q) : chunk_at(q - pt); };

    for (int q = lane; q < pt; q += 64) out[q] = left_at(q);
    const int T4 = Tc >> 2;
    for (int g = lane; g < T4; g += 64) {
        const f32x4 a = *(const f32x4u*)(x0 + 4 * g);
        const f32x4 w = x1 ? (f32x4)(*(const f32x4u*)(x1 + 4 * g)) : a;
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = act(a[j], w[j]);
        *(f32x4u*)(out + pt + 4 * g) = y;
    }
    for (int t = 4 * T4 + lane; t < Tc; t += 64) out[pt + t] = chunk_at(t);
    const int last = pt + Tc - 1;
    for (int q = pt + Tc + lane; q < Tp; q += 64) {
        const int src = 2 * last - q;                         // host-checked: padR <= pt + Tc - 1, so src >= 0
        out[q] = concat_at(src);
    }
    for (int j = lane; j < pt; j += 64) cout[j] = concat_at(Tc + j);
}

}  // namespace

hipError_t launch_stream_stage(const StreamStage& s, hipStream_t st) {
    if (s.B <= 0 || s.C <= 0 || s.Tc <= 0 || s.pt < 0 || s.padR < 0 || s.padR > s.pt + s.Tc - 1 || s.s0.aff || s.s1.aff || s.s1.div)
        return hipErrorInvalidValue;
    StageArgs a;
    a.s0 = s.s0.ptr; a.s1 = s.s1.ptr; a.div = s.s0.div; a.carry_in = s.carry_in; a.carry_out = s.carry_out; a.buf = s.buf;
    a.C = s.C; a.Tc = s.Tc; a.pt = s.pt; a.padR = s.padR; a.left = s.left; a.elu = s.elu; a.alpha = s.alpha;
    hipLaunchKernelGGL(stream_stage_kernel, dim3((s.C + 3) / 4, s.B), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace fc
