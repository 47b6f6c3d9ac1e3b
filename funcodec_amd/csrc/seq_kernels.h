// Launch interface of the SEANet transformer bottleneck's attention kernel (seq_kernels.hip).
//
// seq_model: transformer (funcodec/modules/normed_modules/transformer.py:26-208) is a plain pre-LayerNorm transformer encoder over
// the bottleneck frames: no positional encoding, no length mask, optionally causal.  Its Linears run on the implicit-GEMM conv kernel
// and its LayerNorms on the LauraTTS feature-major LayerNorm (engine.hip run_transformer); this kernel is the attention.
#pragma once
#include <hip/hip_runtime.h>

#include "ragged_kernels.h"

namespace fc {

struct SeqAttn {
    const float* qkv = nullptr;     // [B][3 C][T] channel-major: rows [0, C) q, [C, 2 C) k, [2 C, 3 C) v; head h owns rows h DK .. h DK + DK - 1
    float* out = nullptr;           // [B][C][T]: softmax(q k^T / sqrt(DK)) v per head, heads concatenated
    int B = 0, H = 0, DK = 0, T = 0;
    int causal = 0;                 // key j is visible to query i iff j <= i (transformer.py:172-177)
};
// DK in {16, 32, 64, 128, 256}; any T >= 1.  Flash-style: no buffer grows with T.
bool seq_attn_supported(int DK);
hipError_t launch_seq_attn(const SeqAttn& a, hipStream_t st);
const char* seq_attn_kernel_name(int DK);

// ---- the attention of a streaming push (seqstream_kernels.hip): few queries against the session's key / value cache ----
// The cache of one block is channel-major like the operands above, [B][C][F] for K and the same for V, with the frame pitch F a
// multiple of 16 (seq_cache_pitch): the fragment loads are those of seq_attn_kernel, a push appends n contiguous floats per channel,
// and a 16-key vector load of V is aligned and never leaves a row.
struct SeqAttnCached {
    const float* qkv = nullptr;     // the chunk's [B][3 C][n]; only its q rows are read
    const float* kc = nullptr;      // [B][C][F]: frames [0, pos + n) hold the utterance's keys, this push's included (SeqCacheAppend)
    const float* vc = nullptr;      // [B][C][F]: the values
    float* out = nullptr;           // [B][C][n]; query i sees keys 0 .. pos + i
    float* part = nullptr;          // seq_attn_cached_part_floats() floats of scratch: the partial (m, l, O) of the key split
    int B = 0, H = 0, DK = 0, n = 0, pos = 0, F = 0;
};
// The thresholds between the forms.  A push of at most kSeqCachedSplitMaxQueries frames is one 16-query tile per (row, head): its keys
// are split over `units` waves, kSeqCachedTilesPerUnit 16-key tiles each until kSeqCachedMaxUnits waves are reached, and the partials
// are merged in unit order by a second launch.  A longer push runs one wave per 16 queries over the whole cache (units = 1, no merge).
constexpr int kSeqCachedSplitMaxQueries = 16;
constexpr int kSeqCachedTilesPerUnit = 2;
constexpr int kSeqCachedMaxUnits = 16;
inline int seq_cache_pitch(int max_frames) { return (max_frames + 15) & ~15; }
__host__ __device__ inline int seq_attn_cached_units(int n, int pos) {
    if (n > kSeqCachedSplitMaxQueries) return 1;
    const int tiles = (pos + n + 15) / 16, u = (tiles + kSeqCachedTilesPerUnit - 1) / kSeqCachedTilesPerUnit;
    return u < 1 ? 1 : (u > kSeqCachedMaxUnits ? kSeqCachedMaxUnits : u);
}
inline size_t seq_attn_cached_part_floats(int B, int H, int DK) { return (size_t)B * H * kSeqCachedMaxUnits * (DK + 2) * 16; }
hipError_t launch_seq_attn_cached(const SeqAttnCached& a, hipStream_t st);
const char* seq_attn_cached_kernel_name(int DK);

// K and V of a push into the cache: rows [C, 3 C) of the chunk's qkv [B][3 C][n] to frames [pos, pos + n) of kc / vc [B][C][F]
struct SeqCacheAppend {
    const float* qkv = nullptr;
    float* kc = nullptr;
    float* vc = nullptr;
    int B = 0, C = 0, n = 0, pos = 0, F = 0;
};
hipError_t launch_seq_cache_append(const SeqCacheAppend& a, hipStream_t st);

// ---- the row-wise forms (a slot push): every row b of the chunk [S][3 C][T] has its own frame count n_b = ragged_cols(len_b) in [0, T]
// (RagLen's rule; 0: an idle row) and its own position pos_b, the frames its utterance has cached.  Row b is computed exactly as the
// lock-step launches compute a one-row push (n_b, pos_b): the same tile loop, the same split (seq_attn_cached_units(n_b, pos_b) waves for
// a row of at most kSeqCachedSplitMaxQueries frames, merged in unit order; one wave per 16 queries above), so its result depends on its
// own inputs and (n_b, pos_b) alone -- not on S, on T or on the other rows.  The pitch of the chunk and of `out` is T; columns [n_b, T)
// of `out` are written as zeros.  The device reads n_b and pos_b once per wave; the host passes what only sizes the grid.
struct SeqRows {
    RagLen len;                     // lens: device [S]; n_b = ragged_cols(lens[b], div, mul, add)
    const int* pos = nullptr;       // device [S]
    int S = 0, T = 0, F = 0;
    int max_waves = 0;              // host: the largest seq_attn_rows_waves(n_b, pos_b) of the push (0: every row is idle)
};
inline int seq_attn_rows_waves(int n, int pos) { return (n + 15) / 16 * seq_attn_cached_units(n, pos); }
struct SeqAttnRows {
    const float* qkv = nullptr;     // [S][3 C][T]
    const float* kc = nullptr;      // [S][C][F]
    const float* vc = nullptr;
    float* out = nullptr;           // [S][C][T]
    float* part = nullptr;          // seq_attn_cached_part_floats(S, H, DK) floats: row b, head h, unit u at ((b H + h) kSeqCachedMaxUnits + u)
    int H = 0, DK = 0;
    SeqRows rows;
};
// two launches: the attention of every row, then the merge of the split rows together with the zeros behind every row's count
hipError_t launch_seq_attn_rows(const SeqAttnRows& a, hipStream_t st);
const char* seq_attn_rows_kernel_name(int DK);

struct SeqCacheAppendRows {
    const float* qkv = nullptr;
    float* kc = nullptr;
    float* vc = nullptr;
    int C = 0;
    SeqRows rows;
};
hipError_t launch_seq_cache_append_rows(const SeqCacheAppendRows& a, hipStream_t st);

}  // namespace fc
