// Residual vector quantiser: a beam search over the stages (launched by rvq_beam_kernels.hip, the kernel: rvq_beam_kernel.h).  The bit stream and the decoder stay as they are; only
// the choice of codes changes.  The reference has no such search: this header is its specification.
//
// Per frame x, stages 0 .. k-1, width W in {2, 4, 8}; slots 0 .. W-1:
//   * a hypothesis is a path of codes and its residual r = x - sum of the path's code vectors, updated per stage as r <- r - E_i[c]
//     element-wise in fp32;
//   * stage i: every hypothesis h and code c give a candidate with score |r_h - E_i[c]|^2, ranked by the expansion
//     (|r_h|^2 - (2 r_h).e_c) + |e_c|^2 on the MFMAs (the greedy kernel's arithmetic).  Slot 0 of the next stage is ALWAYS the greedy
//     path: parent slot 0, code g[i] (the caller's `codes`, written by launch_rvq_encode).  Slots 1 .. W-1 take the best remaining
//     candidates by (score, parent slot, code), ascending.  Stage 0 has one hypothesis;
//   * after the last stage every slot's error is recomputed as sum_d r[d]^2 in one fixed fp32 order (rvq_row_norm, device_common.h; no
//     expansion).  The smallest wins, ties go to the lowest slot: a frame is never coded worse than greedy under that formula.
//     A frame of all zeros (digital silence) keeps its greedy codes, whatever the slots' errors.
// Nothing is carried between frames.
//
// Per-row stage counts (nq_rows): a row with count k runs the SEARCH over k stages and picks among the slots after stage k - 1.  That is
// not a prefix of the search over more stages: the pick after stage k - 1 is not the path that wins later.  (The kept sets of the stages
// are the same in both; only the pick differs.)  Codes and paths of the stages behind a row's count are 0.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fc {

// widths the search is built for
inline bool rvq_beam_width_ok(int W) { return W == 2 || W == 4 || W == 8; }

// Sets what the instantiation for (D, W) needs before its first launch (its LDS may pass 64 KiB); launch_rvq_beam calls it too.  Not a
// stream operation: call it outside a stream capture at least once per shape.
hipError_t rvq_beam_prepare(int D, int W);

// codes [nq][N]: the greedy codes on entry, the chosen path on exit.  paths [W][nq][N] / errors [W][N] (or null): every slot's final
// path and its fixed-order error.  LDS only, no workspace.  D in {16, 32, 64, 128, 256, 512}; K a multiple of 16 below 2^24.
hipError_t launch_rvq_beam(const float* x /* [N][D] */, int N, int D, int K, int nq, int W, const float* cb, const float* cb_frag /* or null */,
                           const float* enorm, int64_t* codes, int64_t* paths, float* errors, int Tf, hipStream_t st,
                           const int* nq_rows /* [N / Tf] or null */ = nullptr);

}  // namespace fc
