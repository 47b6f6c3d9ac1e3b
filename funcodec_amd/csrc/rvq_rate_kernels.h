// Residual vector quantiser: how many stages a piece of audio takes.  A count per row or per frame, given by the caller or chosen on the
// device by a target SNR (launched by rvq_rate_kernels.hip; the sum and the decode by a count are rvq_kernels.hip).  The reference has no
// such mode: this header is its specification; funcodec_amd/engine.py::rate_pick and ::rate_pick_frames restate the picks on the host.
//
// THE COUNT (StageCounts, ragged_kernels.h).  Frame row n = b Tf + t takes k stages: frames[n] if a count per frame is given, else
// rows[n / Tf] if a count per row is, else nq; a count is clamped to [0, nq].  A residual quantiser is a prefix code per frame and nothing
// is carried from frame to frame, so either count is exact: the frame is what the call with n_q = k gives it.  The kernels that sum
// (launch_rvq_codes_sum), decode (launch_rvq_decode) or zero (launch_rvq_rate_zero_codes) by a count read it through stage_count; codes
// behind a count are not read and never raise FC_STATUS_BAD_CODE.
//
// THE ROW RULE.  Input rows x [N = B Tf][D] (what launch_rvq_encode was handed) and the codes c [nq][N] the call found at the cap, whoever
// found them (the greedy kernel, or the search of rvq_beam_kernels.h at its full depth).
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
//
// THE FRAME RULE, in terms of the row rule.  Inputs: the stage errors err and the fp64 row sums E above, unchanged; rho_b and cap_b as
// above; the row's own frame count F_b (Tf, or the row's frames in a length-aware call); the floor lo = min_nq clamped to [0, cap_b] -- in
// frame mode a frame may take no stage at all.
//   * thr_b = E_b[0] * rho_b: the one IEEE double product of the row rule;
//   * a row whose E_b[0 .. cap_b] are not all finite: every frame of it takes cap_b (what the plain call gives it);
//   * a row with E_b[0] == 0 (digital silence): every frame takes lo;
//   * else frame t takes the smallest k in [lo, cap_b] with (double)err[k][b, t] * (double)F_b <= thr_b -- products only, no division, so
//     a host restates it operation by operation;
//   * if no k qualifies: the k in that range with the smallest err[k][b, t], first on ties (the scan of the row rule, on the frame's
//     fp32 errors);
//   * frames behind a row's frames get count 0, and nothing of them is read.
// If every frame of a row meets its threshold then sum_t err[k_t][b, t] <= thr_b up to the rounding of the sum: every frame is quantised
// down to the same noise floor thr_b / F_b, however loud it is.  A constant noise floor per row is reverse water-filling, the
// rate-distortion optimum for independent components; the row rule instead spends the loudest frame's stages on a silent one.
// Outputs, all on the device: n_q_frames [B][Tf] i32; n_q_rows [B] i32, the row's largest frame count; n_codes_rows [B] i32 = sum_t k_t;
// achieved [B] f64 = sum_t err[k_t][b, t] in the order E_b is summed.
// The caller then sums and zeroes as above with the counts per frame: for greedy codes frame (b, t) is bit for bit the call with
// n_q = k_t; for the search it is the first k_t codes of the full-depth path.  A frame with k_t = 0 has quantized exactly 0.
//
// THE PUSH RULE, in terms of the row rule: the count of a row of ONE encode push of a session (fc_stream_encode, fc_slots_encode), chosen
// inside the push by an absolute noise floor (fc_engine_set_floor).  A push sees a few frames of an utterance, so a ratio to the input
// energy would follow every pause of the speaker; the floor is a level that does not move.  Inputs: the stage errors err and the fp64 sums
// E_b above, over the F_b frames the row has in THIS push (every row's Tf in a lock-step session; ceil(samples_b / hop) in a slot push),
// from the codes found at the cap; cap_b as above (the row's or slot's current n_q); lo = min_nq in [1, cap_b] (a mode-0 packet needs
// k >= 1); and a floor per row, floor_b, a double made by the host: floor_b = D * 10^(noise_floor_db_b / 10), D the quantiser's input
// width -- the floor reads as "mean-square residual per element, in dB re 1".  It is neither negative nor NaN.
//   * thr_b = floor_b * (double)F_b: one IEEE double product, no division;
//   * a row whose E_b[0 .. cap_b] are not all finite takes cap_b (what the plain push gives it);
//   * a row with E_b[0] <= thr_b takes lo: its input is already at or below the floor -- silence, the discontinuous-transmission case;
//   * else k_b = the smallest k in [lo, cap_b] with E_b[k] <= thr_b;
//   * if there is none: the k in that range with the smallest E_b[k], first on ties (the scan of the row rule).  A floor of 0
//     (noise_floor_db = -inf) therefore means "the best k", a floor of +inf means lo;
//   * a row that emits no frame in the push (F_b == 0: an idle slot) is neither read nor written: its entry of the count table stays;
//   * a row switched off (fc_engine_set_floor_form; on the device its floor reads -1, a value no caller can give) takes cap_b: a slot
//     without a floor beside slots that have one.
// The rule is stateless: a row's count depends on that row's frames of that push and on nothing else.  The row is then summed and zeroed as
// for the row rule: for greedy codes row b of the push is bit for bit the push with n_q = k_b and zeros in codes[k_b:]; for the search it is
// the first k_b codes of the full-depth path.
// Two forms, bit for bit the same outputs.  The chain: launch_rvq_stage_errors, launch_rvq_rate_rows with `floor`, launch_rvq_codes_sum,
// launch_rvq_rate_zero_codes -- any width.  The fused form, launch_rvq_push_floor: ONE launch for pushes of at most 256 frames per row
// (every partial of the fp64 sum then holds at most one term), which runs the same device steps in the same order.  Both read frames,
// caps and floors from device memory only, so a captured push replays unchanged when a floor changes.
//
// THE PUSH FRAME RULE, in terms of the push rule: a count per FRAME of one encode push of a session, chosen inside the push by the same
// absolute floor (fc_engine_set_floor, then fc_engine_set_floor_frames).  The push rule takes one count for all frames of a push -- one loud
// frame buys every stage for 99 silent ones, and the count follows how the caller cuts the audio into pushes.  An absolute floor per frame
// needs no sum over frames: no fp64 tree, no F_b in the threshold.  Inputs: the fp32 stage errors err[k][b, t] above (same order,
// contraction off) from the codes found at the cap; cap_b; floor_b = D * 10^(noise_floor_db_b / 10), the host's double; lo = min_nq clamped
// to [0, cap_b] -- in frame mode a frame may take no stage at all.  For frame t < F_b of a row that has frames in the push:
//   * a row switched off (its floor reads -1 on the device) takes cap_b in every frame;
//   * a frame whose err[0 .. cap_b] are not all finite takes cap_b (what the plain push gives it);
//   * a frame with (double)err[0] <= floor_b takes lo: silence, at frame granularity;
//   * else the frame takes the smallest k in [lo, cap_b] with (double)err[k] <= floor_b -- comparisons only, no product, no division;
//   * if there is none: the k in that range with the smallest err[k], first on ties (the scan of the row rule on the frame's fp32 errors).
// Frames t >= F_b of such a row take 0 and nothing of them is read: their codes are zeroed, their quantized and sub_quants are 0.  A row
// with F_b == 0 (an idle slot) has its row of the count table left unwritten, as in the push rule.
// A frame's count is a function of that frame's quantiser input, its row's cap and floor alone: not of the push's width, the row, the slot
// or the chunking.  For greedy codes frame (b, t) is bit for bit the push with n_q = k_t and zeros in codes[k_t:]; for the search it is the
// first k_t codes of the full-depth path.
// For F_b = 1 and min_nq >= 1 this rule IS the push rule: floor_b * 1.0 is floor_b, and the one-term sum 0.0 + (double)err is (double)err.
// Two forms, bit for bit the same outputs on every row that has frames.  The fused form, launch_rvq_push_floor_frames: ONE launch, a
// workgroup per tile of 16 frames of a row, any width.  The chain: launch_rvq_stage_errors, launch_rvq_floor_frames, launch_rvq_codes_sum
// and launch_rvq_rate_zero_codes with the counts per frame.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ragged_kernels.h"

namespace fc {

// err [nq + 1][N].  nq_rows [N / Tf] (caps) or null; rows.lens null: every row has Tf frames.  D in {16, 32, 64, 128, 256, 512}.
hipError_t launch_rvq_stage_errors(const float* x /* [N][D] */, const int64_t* codes /* [nq][N] */, int N, int D, int K, int nq, const float* cb,
                                   float* err, int Tf, const int* nq_rows, const RagLen& rows, hipStream_t st);

// One workgroup per batch row: row_err [B][nq + 1] (never null), then the pick into k_table [B] and n_q_out [B] (either may be null).
// floor (dev [B], or null): the absolute threshold of the push rule in place of the ratio, which is then not read; a row without frames
// writes nothing.
hipError_t launch_rvq_rate_rows(const float* err /* [nq + 1][B Tf] */, int B, int Tf, int nq, const int* nq_rows, const RagLen& rows,
                                const double* ratio /* dev [B] */, int min_nq, int* k_table, int32_t* n_q_out, double* row_err, hipStream_t st,
                                const double* floor = nullptr);

// The push rule in one launch: stage errors, row sums, pick, zeros and sum of one push, one workgroup per batch row.  codes [nq][B Tf] are
// rewritten in place; n_q_out [B] never null; quant [B Tf][D], quant_bdt [B][D][Tf], subq [nq][B][D][Tf], row_err [B][nq + 1] and serr_out
// [nq + 1][B Tf] may each be null.  rvq_push_floor_fits: whether the launch exists for this shape (Tf <= 256, nq <= 64, its LDS fits);
// where it does not the caller runs the chain.
constexpr int kPushFloorMaxFrames = 256, kPushFloorMaxStages = 64;
bool rvq_push_floor_fits(int Tf, int D, int nq);
hipError_t launch_rvq_push_floor(const float* x /* [B Tf][D] */, int64_t* codes, int B, int Tf, int D, int K, int nq, const float* cb,
                                 const int* nq_rows, const RagLen& rows, const double* floor /* dev [B] */, int min_nq, int32_t* n_q_out, float* quant,
                                 float* quant_bdt, float* subq, double* row_err, float* serr_out, hipStream_t st);

// The push frame rule in one launch: one workgroup per tile of 16 frames of a batch row, any Tf.  codes [nq][B Tf] are rewritten in place;
// n_q_frames [B][Tf] never null; quant [B Tf][D], quant_bdt [B][D][Tf], subq [nq][B][D][Tf] and serr_out [nq + 1][B Tf] may each be null.
// nq <= kPushFloorFramesMaxStages, B <= 65535, D in {16, 32, 64, 128, 256, 512}.
constexpr int kPushFloorFramesMaxStages = 64;
hipError_t launch_rvq_push_floor_frames(const float* x /* [B Tf][D] */, int64_t* codes, int B, int Tf, int D, int K, int nq, const float* cb,
                                        const int* nq_rows, const RagLen& rows, const double* floor /* dev [B] */, int min_nq, int32_t* n_q_frames,
                                        float* quant, float* quant_bdt, float* subq, float* serr_out, hipStream_t st);
// The pick of its chain form, one thread per frame: err [nq + 1][B Tf] (launch_rvq_stage_errors wrote it on the same stream) -> n_q_frames [B][Tf].
hipError_t launch_rvq_floor_frames(const float* err, int B, int Tf, int nq, const int* nq_rows, const RagLen& rows, const double* floor /* dev [B] */,
                                   int min_nq, int32_t* n_q_frames, hipStream_t st);

// One workgroup per batch row.  err [nq + 1][B Tf]; row_err [B][nq + 1] (launch_rvq_rate_rows wrote it on the same stream); nq_rows [B] (caps)
// or null; rows.lens null: every row has Tf frames.  n_q_frames [B][Tf] never null; the three row outputs may be null.
hipError_t launch_rvq_rate_frames(const float* err, const double* row_err, int B, int Tf, int nq, const int* nq_rows, const RagLen& rows,
                                  const double* ratio /* dev [B] */, int min_nq, int32_t* n_q_frames, int32_t* n_q_rows_out, int32_t* n_codes_out,
                                  double* achieved, hipStream_t st);

// codes[i][n] = 0 for every i >= the count of frame row n (one of k's tables is set)
hipError_t launch_rvq_rate_zero_codes(int64_t* codes /* [nq][N] */, int N, int Tf, int nq, const StageCounts& k, hipStream_t st);

// ---- rvq_kernels.hip
// codes [B][Tf][nq] (i64) -> emb [B][Tf][D] and/or emb_bdt [B][D][Tf]: out = ((0 + E_0[i0]) + E_1[i1]) + ... over the frame's first k codes
// status: host-visible engine status words (FC_STATUS_*), or null; an index outside [0, K) sets FC_STATUS_BAD_CODE
// rows (lens given): a frame behind its row's frames counts 0 stages whatever the tables hold
hipError_t launch_rvq_decode(const int64_t* codes, int B, int Tf, int nq, int D, int K, const float* cb, float* emb, float* emb_bdt,
                             unsigned* status, const StageCounts& k, const RagLen& rows, hipStream_t st);
// What the quantiser returns besides codes, from the final codes [nq][N]: quant [N][D] = ((0 + E_0[c0]) + E_1[c1]) + ... (the order of
// launch_rvq_decode and of the greedy kernel, so bit for bit what decoding those codes gives), quant_bdt [B][D][Tf], subq [nq][B][D][Tf]
// (E_i[c_i]; 0 behind a frame's count).  Each may be null.
hipError_t launch_rvq_codes_sum(const int64_t* codes, int N, int D, int K, int nq, const float* cb, float* quant, float* quant_bdt, float* subq,
                                int Tf, const StageCounts& k, hipStream_t st);

}  // namespace fc
