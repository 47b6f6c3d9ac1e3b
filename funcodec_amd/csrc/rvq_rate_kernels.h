// Residual vector quantiser: a stage count per row chosen on the device by a target SNR (launched by rvq_rate_kernels.hip).  The
// reference has no such mode: this header is its specification; funcodec_amd/engine.py::rate_pick restates the pick on the host.
//
// Input rows x [N = B Tf][D] (what launch_rvq_encode was handed) and the codes c [nq][N] the call found at the cap, whoever found them
// (the greedy kernel, or the search of rvq_beam_kernels.h at its full depth).
//   * stage errors err [nq + 1][N] fp32:  r_0 = x[n];  r_{i+1} = r_i - E_i[c_i[n]] element-wise in fp32;  err[i][n] = |r_i|^2 in the fixed
//     order of rvq_row_norm (device_common.h): four chains over D / 4, squares rounded separately, (p0 + p1) + (p2 + p3) -- compiled here
//     with contraction off, so every multiply and add rounds by itself (the encode kernels' own copy fuses square and add; their
//     errors may differ from these in the last bit).  err[0] is the input energy.  A row stops at its cap (nq_rows, else nq): err[i]
//     behind it is 0.  So are all errors of a frame behind the row's frames in a length-aware call (nothing of such a frame is read).
//     An index outside [0, K) is read as 0, as rvq_codes_sum_kernel does;
//   * row errors E [B][nq + 1] fp64:  E_b[i] = sum over the row's frames t of err[i][b, t], in an order that depends on the row's frame
//     count alone: 256 partial sums (partial j takes t = j, j + 256, ... in rising order) added as a binary tree;
//   * the pick, with ratio rho_b = 10^(-target_b / 10) (a double made by the host), floor min_nq and cap cap_b:
//       - a row whose E_b[0 .. cap_b] are not all finite takes cap_b (what the plain call gives it);
//       - a row with E_b[0] == 0 (digital silence) takes min_nq;
//       - else k_b = the smallest k in [min_nq, cap_b] with E_b[k] <= E_b[0] * rho_b (one IEEE double product);
//       - if no k reaches the target: the k in that range with the smallest E_b[k], first on ties -- the curve is not monotone on real
//         codebooks, and a missed target must never cost more bits for a worse result.  A target of +inf (rho = 0) therefore means
//         "the best k".
// The caller then sums the first k_b code vectors of every row (launch_rvq_codes_sum with the chosen table: stage order from 0, the greedy
// kernel's running sum) and zeroes codes[k_b:] (launch_rvq_rate_zero_codes).  For greedy codes row b is then bit for bit the call with
// n_q = k_b.  For the search it is the first k_b codes of the full-depth path, which is NOT the search over k_b stages.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ragged_kernels.h"

namespace fc {

// err [nq + 1][N].  nq_rows [N / Tf] (caps) or null; rows.lens null: every row has Tf frames.  D in {16, 32, 64, 128, 256, 512}.
hipError_t launch_rvq_stage_errors(const float* x /* [N][D] */, const int64_t* codes /* [nq][N] */, int N, int D, int K, int nq, const float* cb,
                                   float* err, int Tf, const int* nq_rows, const RagLen& rows, hipStream_t st);

// One workgroup per batch row: row_err [B][nq + 1] (never null), then the pick into k_table [B] and n_q_out [B] (either may be null).
hipError_t launch_rvq_rate_rows(const float* err /* [nq + 1][B Tf] */, int B, int Tf, int nq, const int* nq_rows, const RagLen& rows,
                                const double* ratio /* dev [B] */, int min_nq, int* k_table, int32_t* n_q_out, double* row_err, hipStream_t st);

// codes[i][n] = 0 for every i >= k_table[n / Tf]
hipError_t launch_rvq_rate_zero_codes(int64_t* codes /* [nq][N] */, int N, int Tf, int nq, const int* k_table, hipStream_t st);

}  // namespace fc
