// Slot session (fc_slots_*): the staging pass in front of every causal conv of a push whose rows start, continue, end and idle
// independently, and the per-row start of an utterance.  See slots_kernels.h for the contract.
// LDS-free streaming kernels, vector stores only, no atomics: every element has exactly one writer.
#include "slots_kernels.h"
#include "device_common.h"

namespace fc {

namespace {

struct StageArgs {
    const float *s0, *s1, *div, *carry_in;
    float *carry_out, *buf;
    const int *lens, *flags;
    int ldiv, lmul;
    int C, T, Tp, k, pt, stride, transposed, elu;
    float alpha;
};

constexpr int kStageSeg = 2048;      // staged columns per workgroup row

// One workgroup = one (slot, channel quad, column segment), one wave per channel row; a lane takes four staged columns at a time: where all
// four are the row's own columns they move as one 16-byte load and one 16-byte store (dword-aligned vector accesses), the context, the
// padding and the row's end as single dwords.  The first segment's workgroup also writes the row's new carry.
__global__ __launch_bounds__(256) void slots_stage_kernel(const StageArgs p) {
    const int lane = threadIdx.x & 63, c = 4 * blockIdx.x + (threadIdx.x >> 6), b = blockIdx.y;
    if (c >= p.C) return;
    const int pt = p.pt, len = p.lens[b], fl = p.flags[b];
    const int n = len > 0 ? min(ragged_cols(len, p.ldiv, p.lmul, 0), p.T) : 0;      // host-checked: never beyond T
    const bool start = (fl & kSlotStart) != 0;
    int extra = (n > 0 && !p.transposed && (fl & kSlotFinal)) ? ragged_extra(n, p.k, pt, p.stride) : 0;
    if (extra > p.Tp - pt - n) extra = p.Tp - pt - n;                               // host-checked: it fits
    const size_t row = (size_t)b * p.C + c;
    const float* x0 = p.s0 + row * p.T;
    const float* x1 = p.s1 ? p.s1 + row * p.T : nullptr;
    const float* cin = p.carry_in + row * pt;
    float* cout = p.carry_out + row * pt;
    float* out = p.buf + row * p.Tp;
    const float dv = p.div ? p.div[b] : 1.f;
    auto act = [&](float v, float w) __attribute__((always_inline)) {
        if (p.div) v = v / dv;
        if (x1) v = v + w;
        if (p.elu) v = elu_f(v, p.alpha);
        return v;
    };
    auto chunk_at = [&](int t) __attribute__((always_inline)) { return act(x0[t], x1 ? x1[t] : 0.f); };
    // column q of [left context | row]; q < pt + n
    auto left_at = [&](int q) __attribute__((always_inline)) {
        if (!start) return cin[q];
        const int src = pt - q;                               // reflection about the row's column 0; a row shorter than that reads as zero-extended
        return (!p.transposed && src < n) ? chunk_at(src) : 0.f;
    };
    auto concat_at = [&](int q) __attribute__((always_inline)) { return q < pt ? left_at(q) : chunk_at(q - pt); };
    const int end = pt + n, last = end - 1;
    auto col = [&](int q) __attribute__((always_inline)) {    // staged column q
        if (n == 0 || q >= end + extra) return 0.f;
        if (q < end) return concat_at(q);
        const int src = 2 * last - q;                         // the FINAL row's extra_padding: reflection about its last column
        return src >= 0 ? concat_at(src) : 0.f;
    };
    const int q_end = min(p.Tp, (int)(blockIdx.z + 1) * kStageSeg);
    for (int q0 = blockIdx.z * kStageSeg + 4 * lane; q0 < q_end; q0 += 256) {
        if (q0 >= pt && q0 + 3 < end && q0 + 3 < q_end) {
            const int t = q0 - pt;
            const f32x4 a = *(const f32x4u*)(x0 + t);
            const f32x4 w = x1 ? (f32x4)(*(const f32x4u*)(x1 + t)) : a;
            f32x4 y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = act(a[j], w[j]);
            *(f32x4u*)(out + q0) = y;
        } else {
            for (int j = 0; j < 4 && q0 + j < q_end; ++j) out[q0 + j] = col(q0 + j);
        }
    }
    if (blockIdx.z == 0)
        for (int j = lane; j < pt; j += 64) cout[j] = n == 0 ? cin[j] : concat_at(n + j);
}

// one workgroup per slot; a row that does not start is left alone
__global__ __launch_bounds__(256) void slots_start_kernel(const int* __restrict__ flags, int S, float* __restrict__ lstm, int L, int H,
                                                          const float* __restrict__ scale_in, float* __restrict__ scale_out) {
    const int b = blockIdx.x;
    if (!(flags[b] & kSlotStart)) return;
    if (lstm)
        for (int i = threadIdx.x; i < 3 * L * H; i += 256) lstm[((size_t)(i / H) * S + b) * H + i % H] = 0.f;      // h [L][2][S][H] | c [L][S][H]
    if (scale_out && threadIdx.x == 0) scale_out[b] = scale_in ? scale_in[b] : 1.f;
}

}  // namespace

hipError_t launch_slots_stage(const SlotsStage& s, hipStream_t st) {
    if (s.S <= 0 || s.S > 65535 || s.C <= 0 || s.T <= 0 || s.pt < 0 || s.stride < 1 || !s.len.lens || !s.flags || s.len.add != 0) return hipErrorInvalidValue;
    if (s.s0.aff || s.s1.aff || s.s1.div || s.s0.ld || s.s1.ld || (s.pt > 0 && (!s.carry_in || !s.carry_out))) return hipErrorInvalidValue;
    if (s.transposed ? (s.pt != 1 || s.Tp < 1 + s.T) : s.Tp < s.pt + s.T + ragged_extra(s.T, s.k, s.pt, s.stride)) return hipErrorInvalidValue;
    StageArgs a;
    a.s0 = s.s0.ptr; a.s1 = s.s1.ptr; a.div = s.s0.div; a.carry_in = s.carry_in; a.carry_out = s.carry_out; a.buf = s.buf;
    a.lens = s.len.lens; a.flags = s.flags; a.ldiv = s.len.div; a.lmul = s.len.mul;
    a.C = s.C; a.T = s.T; a.Tp = s.Tp; a.k = s.k; a.pt = s.pt; a.stride = s.stride; a.transposed = s.transposed; a.elu = s.elu; a.alpha = s.alpha;
    hipLaunchKernelGGL(slots_stage_kernel, dim3((s.C + 3) / 4, s.S, (s.Tp + kStageSeg - 1) / kStageSeg), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_slots_start(const int* flags, int S, float* lstm, int L, int H, const float* scale_in, float* scale_out, hipStream_t st) {
    if (!flags || S <= 0 || (lstm && (L < 1 || H < 1))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(slots_start_kernel, dim3(S), dim3(256), 0, st, flags, S, lstm, L, H, scale_in, scale_out);
    return hipGetLastError();
}

}  // namespace fc
