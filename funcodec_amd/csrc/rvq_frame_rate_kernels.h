// Residual vector quantiser: a stage count per FRAME chosen on the device by a target SNR (launched by rvq_frame_rate_kernels.hip).
// A residual quantiser is a prefix code per frame and nothing is carried from frame to frame, so a count per frame is exact.  The
// reference has no such mode: this header is its specification; funcodec_amd/engine.py::rate_pick_frames restates the pick on the host.
//
// Inputs: the stage errors err [nq + 1][N = B Tf] fp32 and the fp64 row sums E [B][nq + 1] of rvq_rate_kernels.h, unchanged; the ratio
// rho_b = 10^(-target_b / 10) (a double made by the host); the row's cap cap_b (nq_rows, else nq); the row's own frame count F_b (Tf, or
// the row's frames in a length-aware call); the floor lo = min_nq clamped to [0, cap_b] -- in frame mode a frame may take no stage at all.
//   * thr_b = E_b[0] * rho_b: the one IEEE double product of the row rule;
//   * a row whose E_b[0 .. cap_b] are not all finite: every frame of it takes cap_b (what the plain call gives it);
//   * a row with E_b[0] == 0 (digital silence): every frame takes lo;
//   * else frame t takes the smallest k in [lo, cap_b] with (double)err[k][b, t] * (double)F_b <= thr_b -- products only, no division, so
//     a host restates it operation by operation;
//   * if no k qualifies: the k in that range with the smallest err[k][b, t], first on ties (the curve is not monotone on real codebooks);
//   * frames behind a row's frames get count 0, and nothing of them is read.
// If every frame of a row meets its threshold then sum_t err[k_t][b, t] <= thr_b up to the rounding of the sum: every frame is quantised
// down to the same noise floor thr_b / F_b, however loud it is.  A constant noise floor per row is reverse water-filling, the
// rate-distortion optimum for independent components; the row rule instead spends the loudest frame's stages on a silent one.
// Outputs, all on the device: n_q_frames [B][Tf] i32; n_q_rows [B] i32, the row's largest frame count; n_codes_rows [B] i32 = sum_t k_t;
// achieved [B] f64 = sum_t err[k_t][b, t] in the order E_b is summed (256 partial sums, partial j takes t = j, j + 256, ... in rising
// order, added as a binary tree).
// The caller then sums the first k_t code vectors of every frame (launch_rvq_frame_codes_sum: stage order from 0, the running sum of
// launch_rvq_codes_sum) and zeroes codes[k_t:] (launch_rvq_frame_zero_codes).  For greedy codes frame (b, t) is then bit for bit the call
// with n_q = k_t; for the search it is the first k_t codes of the full-depth path.  A frame with k_t = 0 has quantized exactly 0.
// The per-frame forms index their table by frame row n = b Tf + t, not by n / Tf; a count is clamped to [0, nq]; codes behind a frame's
// count are not read and never raise FC_STATUS_BAD_CODE.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ragged_kernels.h"

namespace fc {

// One workgroup per batch row.  err [nq + 1][B Tf]; row_err [B][nq + 1] (launch_rvq_rate_rows wrote it on the same stream); nq_rows [B] (caps)
// or null; rows.lens null: every row has Tf frames.  n_q_frames [B][Tf] never null; the three row outputs may be null.
hipError_t launch_rvq_rate_frames(const float* err, const double* row_err, int B, int Tf, int nq, const int* nq_rows, const RagLen& rows,
                                  const double* ratio /* dev [B] */, int min_nq, int32_t* n_q_frames, int32_t* n_q_rows_out, int32_t* n_codes_out,
                                  double* achieved, hipStream_t st);

// launch_rvq_codes_sum with a count per frame: k_frames [N], clamped to [0, nq]
hipError_t launch_rvq_frame_codes_sum(const int64_t* codes /* [nq][N] */, int N, int D, int K, int nq, const float* cb, float* quant, float* quant_bdt,
                                      float* subq, int Tf, const int32_t* k_frames, hipStream_t st);

// codes[i][n] = 0 for every i >= k_frames[n]
hipError_t launch_rvq_frame_zero_codes(int64_t* codes /* [nq][N] */, int N, int nq, const int32_t* k_frames, hipStream_t st);

// launch_rvq_decode with a count per frame: codes [B][Tf][nq], k_frames [B][Tf] clamped to [0, nq]; a frame behind its row's frames
// (rows.lens given) counts 0 stages whatever the table holds
hipError_t launch_rvq_frame_decode(const int64_t* codes, int B, int Tf, int nq, int D, int K, const float* cb, float* emb, float* emb_bdt,
                                   unsigned* status, const int32_t* k_frames, const RagLen& rows, hipStream_t st);

}  // namespace fc
