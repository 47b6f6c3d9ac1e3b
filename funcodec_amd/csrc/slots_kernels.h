// Launch interface of the slot session's kernels (slots_kernels.hip), used by engine.hip: a push over [S][C][T] in which every row (slot)
// has its own count of columns and its own place in its utterance (fc_slots_*, include/funcodec_amd.h).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "ragged_kernels.h"

namespace fc {

// flags of a row in a push (the C ABI's FC_SLOT_START / FC_SLOT_FINAL)
constexpr int kSlotStart = 1, kSlotFinal = 2;

// The materialised input of one causal conv of a slot push: the union of the streaming pass (stream_kernels.h: left context and carry) and
// the length-aware one (ragged_kernels.h: every row ends at its own column).  Row b has n_b = ragged_cols(len_b) columns (RagLen's rule:
// exact for whole-hop pushes, the ceiling for a FINAL row; len_b = 0: an idle row) and flags_b:
//   buf[b][c][p], p in [0, Tp):
//     p <  pt                 the left context: carry_in, or for a START row what the offline call pads with -- the reflection
//                             act(x)[pt - p] of the row's own columns, or zeros in front of a transposed conv
//     p <  pt + n_b           act(x)[p - pt],  act(x) = [elu](s0 / div + s1)
//     p <  pt + n_b + extra_b a FINAL row's own extra_padding (ragged_extra(n_b)): the reflection of the columns in front of it, which may
//                             reach back into the left context
//     else                    zeros
//   carry_out[b][c][j] = [left | row][n_b + j], j in [0, pt): the last pt columns of [left context | row].
// An idle row stages zeros throughout and copies carry_in to carry_out, so that the ping-pong parity of the carries is one number for the
// whole session.  Nothing behind a row's n_b columns is read from s0 / s1; carry_in of a START row is not read either.
// carry_in and carry_out are different buffers: every element has one writer and no reader of a location another thread writes.
struct SlotsStage {
    Src s0, s1;                       // [S][C][T] each; no pending affines (causal nets have no GroupNorm); s0.div: the slots' scale [S]
    int elu = 0; float alpha = 1.f;
    int S = 0, C = 0, T = 0, Tp = 0;  // Tp >= pt + T + ragged_extra(T) (1 + T for a transposed conv)
    int k = 1, pt = 0, stride = 1, transposed = 0;
    RagLen len;                       // lens: device [S], 0 = idle (NOT clamped, unlike a ragged pass)
    const int* flags = nullptr;       // device [S]
    const float* carry_in = nullptr;  // [S][C][pt]
    float* carry_out = nullptr;       // [S][C][pt]
    float* buf = nullptr;             // [S][C][Tp]
};
hipError_t launch_slots_stage(const SlotsStage& s, hipStream_t st);

// The rows that START an utterance in this push: their (h, c) of one side's LSTM block -- lstm = h [L][2][S][H] | c [L][S][H], or null --
// are cleared, and with scale_out their volume scale is set: scale_out[b] = scale_in ? scale_in[b] : 1.  Other rows are not touched.
hipError_t launch_slots_start(const int* flags, int S, float* lstm, int L, int H, const float* scale_in, float* scale_out, hipStream_t st);

}  // namespace fc
