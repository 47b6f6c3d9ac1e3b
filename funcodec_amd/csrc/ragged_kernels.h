// Launch interface of the length-aware (ragged) pass (ragged_kernels.hip), used by engine.hip: a batch [B][..][Tmax] with one length per
// row, every row computed as the offline call computes that row alone (fc_*_ragged, include/funcodec_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

namespace fc {

// ---- the per-layer row-length rule, stated once.  Every strided SConv1d of the reference pads its input up to a whole number of strides
// (get_extra_padding_for_conv1d, conv.py:57-64), so a row of n columns leaves a stride-s conv with ceil(n / s) columns, and nested ceilings
// collapse: a row of `len` samples has ceil(len / rate) columns at an encoder layer whose input rate is `rate`, ceil(len / hop) frames at
// the bottleneck, frames * rate columns at a decoder layer.  `add`: the untrimmed output of a transposed conv, which is what its GroupNorm
// sees (conv.py:287-303), has one more group of `stride` columns than the trimmed one.
struct RagLen {
    const int* lens = nullptr;    // device [B], already clamped to [1, Tmax] (launch_ragged_lengths)
    int div = 1, mul = 1, add = 0;
};
__host__ __device__ inline int ragged_cols(int len, int div, int mul, int add) { return (len + div - 1) / div * mul + add; }
// frames of batch row b of a quantiser call: all Tf, or the row's own in a length-aware call
__device__ __forceinline__ int row_frames(const RagLen& rows, int b, int Tf) {
    if (!rows.lens) return Tf;
    const int f = ragged_cols(rows.lens[b], rows.div, rows.mul, rows.add);
    return f < Tf ? f : Tf;
}

// ---- how many quantiser stages frame row n = b Tf + t takes, stated once (rvq_rate_kernels.h): a count per batch row, a count per frame,
// or nq everywhere.  The kernels that sum, decode or zero codes by a count read it through stage_count; the codes behind it are not read.
struct StageCounts {
    const int32_t* rows = nullptr;      // device [B], indexed n / Tf
    const int32_t* frames = nullptr;    // device [B][Tf], indexed n; wins over rows
};                                      // both null: nq everywhere
__device__ __forceinline__ int stage_count(const StageCounts& c, int n, int b, int nq) {
    const int k = c.frames ? c.frames[n] : (c.rows ? c.rows[b] : nq);
    return k < 0 ? 0 : (k > nq ? nq : k);      // clamped to [0, nq]
}

// SConv1d's extra_padding for a row of n columns (conv.py:57-64); conv_geom in engine.hip calls it for the whole batch width
__host__ __device__ inline int ragged_extra(int n, int k, int pt, int stride) {
    const int num = n - k + pt;
    const int nfr = num >= 0 ? (num + stride - 1) / stride : -((-num) / stride);
    return nfr * stride + (k - pt) - n;
}

// lens[b] = clamp(in[b], 1, Tmax); a length outside that range raises FC_STATUS_BAD_LENGTH
hipError_t launch_ragged_lengths(const int32_t* in, int B, int Tmax, int* lens, unsigned* status, hipStream_t st);

// The staging pass in front of a conv of a ragged pass, sibling of stream_stage_kernel: applies the consumer's prologue
// act(aff0(s0 / div) + aff1(s1)) and writes, per row, [left padding | the row's n columns | right padding incl. the row's own extra_padding
// | zeros] into buf [B][C][Tp]: reflection, or the zero-extended reflection of pad1d for rows not longer than the padding (conv.py:82-99),
// by the row's OWN length n = ragged_cols(len).  Nothing behind a row's n columns is read, so what the producer (or the caller) left there
// never reaches an output; what is written there is zero, which keeps every later layer's discarded columns finite.
// transposed: [0 | the row's n columns | zeros]: nothing leaks into the row's last `stride` output columns.
struct RaggedStage {
    Src s0, s1;                       // [B][C][ld] each (Src.ld; 0 = Tin)
    int elu = 0; float alpha = 1.f;
    int B = 0, C = 0, Tin = 0, Tp = 0;
    int k = 1, pt = 0, stride = 1;    // the SConv1d's kernel, padding_total and stride
    int causal = 0, transposed = 0;
    RagLen len;
    float* buf = nullptr;
};
hipError_t launch_ragged_stage(const RaggedStage& s, hipStream_t st);

// GroupNorm(1, C) over a row's valid columns only: x [B][C][ld], columns [0, ragged_cols(len)) of every channel; fp64, a summation order
// that depends on (C, the row's columns) alone.  aff [B][C][2] = (scale, shift), as launch_gn_finalize writes it.
// partials: [B][C][ragged_gn_segments(ld)][2] doubles, written by the first launch and summed per row by the second.
int ragged_gn_segments(int cols);
hipError_t launch_ragged_gn_partials(const float* x, int B, int C, int ld, const RagLen& len, double* partials, hipStream_t st);
hipError_t launch_ragged_gn_finalize(const double* partials, int B, int C, int ld, const RagLen& len, const float* gamma, const float* beta,
                                     float eps, float* aff, hipStream_t st);

// Zero everything behind a row's valid part of a final output viewed as [O][B][M][T][Dn]: element (o, b, m, t, d) with t >= ragged_cols(len_b).
// Stores only; what is valid is not touched.
hipError_t launch_ragged_mask_f32(float* p, int O, int B, int M, int T, int Dn, const RagLen& len, hipStream_t st);
hipError_t launch_ragged_mask_i64(int64_t* p, int O, int B, int M, int T, int Dn, const RagLen& len, hipStream_t st);

}  // namespace fc
