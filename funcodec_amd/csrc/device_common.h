// Device-side pieces that several translation units must state identically: the 16-byte vector types, the ELU every pass applies,
// and the workgroup reduction behind a GroupNorm partial slot.  Device code only; depends on nothing but the HIP runtime header.
#pragma once
#include <hip/hip_runtime.h>

namespace fc {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // 16-byte accesses at dword alignment (global memory takes them)

// ELU(alpha) on the hardware exp2: exp(v) = 2^(v*log2 e).  For v <= 0 the rounding of the product contributes
// |v|*log2(e)*2^-24 relative error to e^v, i.e. at most 3e-8 absolute on the ELU output (below one fp32 ulp of the
// result), so no compensated product is needed.  fp32 MFMA and fp32 VALU share the SIMD's FMA lanes on gfx950
// (tests/micro/mfma_valu_overlap.hip: the two do not overlap), so every VALU instruction here is paid in full.
// The one definition: the conv kernels' fused prologue and the stream / ragged / slot staging kernels all call it, so a layer sees the
// same activation in every kind of pass.
__device__ __forceinline__ float elu_f(float v, float alpha) {
    const float e = __builtin_amdgcn_exp2f(v * 1.44269504088896341f);
    return v > 0.f ? v : fmaf(e, alpha, -alpha);
}

// The epilogue contract of every 256-thread kernel that feeds a GroupNorm(1, C): a lane's fp32 (sum, sum of squares) become fp64, a wave
// butterfly 32 -> 1 adds the 64 lanes, the four wave totals meet in `red` and thread 0 adds them as ((w0 + w1) + w2) + w3.  Every thread of
// the workgroup calls it (it holds a barrier); only thread 0 gets `true` and the two totals, every other thread `false` and zeros.  The
// partial slot they go to is the caller's.
__device__ __forceinline__ bool gn_partial_reduce(float s1v, float s2v, double (&red)[2][4], double& s1, double& s2) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double d1 = (double)s1v, d2 = (double)s2v;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        d1 += __shfl_xor(d1, off, 64);
        d2 += __shfl_xor(d2, off, 64);
    }
    if (lane == 0) { red[0][wid] = d1; red[1][wid] = d2; }
    __syncthreads();
    s1 = s2 = 0.0;          // threads other than 0 get zeros, not garbage
    if (tid != 0) return false;
    s1 = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    s2 = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    return true;
}

// |x|^2 of one residual row by four lanes j = 0 .. 3 (consecutive lanes): chain j over d in [j D/4, (j + 1) D/4) with the square rounded
// separately, the chains combined (p0 + p1) + (p2 + p3); lane j = 0 writes the result
template <int D>
__device__ __forceinline__ void rvq_row_norm(const float* row, int j, float* xn_row) {
    float s = 0.f;
#pragma unroll 8
    for (int d = j * (D / 4); d < (j + 1) * (D / 4); ++d) {
        const float v = row[d];
        s = __fadd_rn(s, __fmul_rn(v, v));
    }
    const float s_pair = __fadd_rn(s, __shfl_xor(s, 1, 64));          // p0+p1 | p2+p3
    const float s_all = __fadd_rn(s_pair, __shfl_xor(s_pair, 2, 64));  // (p0+p1)+(p2+p3)
    if (j == 0) *xn_row = s_all;
}

}  // namespace fc
