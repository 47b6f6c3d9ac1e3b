// Residual vector quantiser: beam search over the stages (specification: rvq_beam_kernels.h), the dispatch.  The kernel is the template
// of rvq_beam_kernel.h; its 18 instantiations live in the rvq_beam_w*.hip units, and this unit only declares them.
#include "rvq_beam_kernels.h"
#include "rvq_beam_kernel.h"

namespace fc {

#define FC_BEAM_D(DD) FC_BEAM_ELSEWHERE(DD, 2) FC_BEAM_ELSEWHERE(DD, 4) FC_BEAM_ELSEWHERE(DD, 8)
FC_BEAM_D(16)
FC_BEAM_D(32)
FC_BEAM_D(64)
FC_BEAM_D(128)
FC_BEAM_D(256)
FC_BEAM_D(512)
#undef FC_BEAM_D

namespace {

size_t beam_lds_bytes(int D, int nq) { return ((size_t)2 * 16 * (D + 4) + (size_t)nq * 16) * sizeof(float); }

// the most stages one launch takes: the back-pointers of 256 stages are 16 KiB of LDS next to at most 65 KiB of residual rows
constexpr int kMaxStages = 256;

template <typename Fn>
hipError_t for_shape(int D, int W, Fn&& fn) {
#define FC_BEAM_W(DD)                                      \
    switch (W) {                                           \
        case 2: return fn(rvq_beam_kernel<DD, 2>);         \
        case 4: return fn(rvq_beam_kernel<DD, 4>);         \
        case 8: return fn(rvq_beam_kernel<DD, 8>);         \
        default: return hipErrorInvalidValue;              \
    }
    switch (D) {
        case 16: FC_BEAM_W(16)
        case 32: FC_BEAM_W(32)
        case 64: FC_BEAM_W(64)
        case 128: FC_BEAM_W(128)
        case 256: FC_BEAM_W(256)
        case 512: FC_BEAM_W(512)
        default: return hipErrorInvalidValue;
    }
#undef FC_BEAM_W
}

}  // namespace

hipError_t rvq_beam_prepare(int D, int W) {
    return for_shape(D, W, [&](auto kernel) {
        return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)beam_lds_bytes(D, kMaxStages));
    });
}

hipError_t launch_rvq_beam(const float* x, int N, int D, int K, int nq, int W, const float* cb, const float* cb_frag, const float* enorm,
                           int64_t* codes, int64_t* paths, float* errors, int Tf, hipStream_t st, const int* nq_rows) {
    if (N <= 0) return hipSuccess;
    if (!rvq_beam_width_ok(W) || K % 16 != 0 || K <= 0 || K >= (1 << 24) || nq < 1 || nq > kMaxStages) return hipErrorInvalidValue;
    if (nq_rows && (Tf <= 0 || N % Tf != 0)) return hipErrorInvalidValue;      // the table is indexed by n / Tf
    if (hipError_t er = rvq_beam_prepare(D, W); er != hipSuccess) return er;
    const int F = 16 / W;
    return for_shape(D, W, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((N + F - 1) / F), dim3(512), beam_lds_bytes(D, nq), st, x, N, K, nq, cb, cb_frag, enorm, codes, paths,
                           errors, Tf > 0 ? Tf : N, nq_rows);
        return hipGetLastError();
    });
}

}  // namespace fc
