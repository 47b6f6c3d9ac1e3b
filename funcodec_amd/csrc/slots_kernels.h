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

// ---- The slot record: everything one utterance in flight owns, as a flat run of floats (fc_slotrec_export / fc_slotrec_import /
// fc_slotrec_export_stream, include/funcodec_amd.h; funcodec_amd/stream.py slot_record_segments restates the list).  THE SPECIFICATION:
//
//   [scale: 1 float]
//   per side, encoder then decoder:
//     per conv that stream_layout gives a carry, in for_each_conv order: its cin * pt floats [cin][pt], taken from the ping-pong half
//       that the side's NEXT push reads (carry_pair(.., n).in: the half at the parity of the n pushes the side has taken)
//     per LSTM layer: h then c, H floats each; h is the half the next push reads, parity 1 (run_lstm leaves it there after every push)
//     in a session with a key / value cache, per transformer block: K then V as [C][Fr], Fr = seq_cache_pitch(frames of that side);
//       columns [frames, Fr) are zeros
//   a side that is not Running (never started, or its FINAL push taken) contributes zeros, and its frame count is 0.
//
// The record is canonical: a pure function of the utterance's pushes.  Nothing of it depends on the session's S, the slot index,
// max_frames (the cache pitch of the record follows the frames held, not the session's bound), max_chunk, the parity of the session's
// push counters (the record holds the read half only), graph replay, or what the other slots hold.  Its length is
// slot_record_floats(); beside it travels a host struct (fc_slot_meta): the phases and frame counts of both sides and `layout`, a
// fingerprint of the segment list (slot_record_layout) by which a record of another architecture is recognised.
//
// On the device the list is a table of segments, built once per session.  A segment is `rows` rows of the slot: one row of `len` floats
// (scale, carry, h, c) or, for a cache plane, C rows of which `frames` columns are in use.
struct SlotSeg {
    long long st_off;      // float offset in the session state of slot 0, row 0 (for a carry: in ping-pong half 0)
    long long half;        // floats from half 0 to half 1 of a carry (the half read is chosen by the side's parity); 0 otherwise
    long long rec_fixed;   // floats of the record in front of this segment, cache planes not counted
    int slot_stride;       // floats from one slot to the next in the state
    int rows, len;         // a plain segment: rows = 1, len floats.  A cache plane: rows = C, len = 0 (its rows are Fr wide in the record)
    int st_pitch;          // a cache plane: the session's frame pitch F = seq_cache_pitch(max_frames)
    int side;              // 0 encoder, 1 decoder, -1 the scale (it belongs to neither: always copied)
    int enc_cols, dec_cols;  // cache rows (C per plane) of either side that lie in front of this segment in the record
};
// one named slot of a call: what the host knows of it
struct SlotRef {
    int slot;
    int enc_frames, dec_frames;      // frames either side's cache holds (0 without a cache or when the side is not Running)
    int bits;                        // bit 0 / 1: the parity half the encoder / decoder side's next push reads; bit 2 / 3: that side is Running
};
constexpr int kSlotRecEncLive = 4, kSlotRecDecLive = 8;
constexpr int kSlotRecChunk = 4096;  // floats of one segment that one workgroup moves

// kinds of a segment in the fingerprint
enum SlotSegKind { kSegScale = 0, kSegCarry = 1, kSegH = 2, kSegC = 3, kSegK = 4, kSegV = 5 };
// FNV-1a over (kind, side, length) of every segment in record order, a cache plane's length being its C; bit 0 says whether the
// list holds cache planes, so that a record without a cache is told from one with a cache by the fingerprint alone
inline uint32_t slot_record_layout_step(uint32_t h, int kind, int side, int len) {
    const uint32_t v[3] = {(uint32_t)kind, (uint32_t)(side + 1), (uint32_t)len};
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 4; ++i) { h ^= (v[j] >> (8 * i)) & 255u; h *= 16777619u; }
    return h;
}
constexpr uint32_t kSlotRecordLayoutSeed = 2166136261u;

// Export (IMPORT = false): records[i] (dev, `pitch` floats apart) = the record of slot refs[i].slot; the state is only read.
// Import (IMPORT = true): the inverse scatter into the halves that refs[i].bits name -- the DESTINATION's read halves -- and from the
// record's cache pitch Fr to the session's F; only columns [0, frames) of a cache row are written, a side that is not Running is left
// alone, and no float of any other slot is touched.  One launch for the n slots: grid = chunks x segments x n.  max_floats: the longest
// segment of any named slot in record floats (it sizes the grid's x).  16-byte vector loads and stores for the groups of four floats
// that begin at a 16-byte boundary of the record and lie whole inside one row and its frames in use (the state side dword-aligned
// where its row offset is no multiple of four floats), single floats at heads, tails, row ends and zero columns.  segs, refs: device.
hipError_t launch_slot_record(bool import, float* state, const SlotSeg* segs, int n_segs, const SlotRef* refs, int n, float* records, size_t pitch,
                              long long max_floats, hipStream_t st);

}  // namespace fc
