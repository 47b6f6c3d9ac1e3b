// Launch interface between the LauraTTS engine (laura.hip) and its gfx950 kernels (laura_kernels.hip).
//
// Two execution forms of the same rel-pos self-attention stacks (funcodec/models/encoder/conformer_encoder.py,
// transformer_encoder.py, funcodec/modules/attention.py:212-308):
//   * FULL-SEQUENCE form (text encoder, LM prefix / teacher forcing, fine codec predictor): activations are FEATURE-MAJOR
//     [B][C][T] (time contiguous), so every Linear is a k = 1 layer of the codec's implicit-GEMM conv kernel (fp32-input MFMA,
//     conv_kernel.h) and attention reads Q / K / V rows as [d][t] slabs;
//   * STEP form (autoregressive decoding with a KV cache): B <= 64 new tokens per step, TOKEN-MAJOR vectors [B][C]; every
//     Linear is a weight-streaming GEMV on 16x16x4 MFMAs (weights in fragment order, one contiguous 1 KiB per wave load;
//     rows beyond 16 as further column blocks of 16 on grid.y, each the 16-column kernel on its own rows),
//     LayerNorm / activation / residual / cache scatter fused into its prologue / epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fc {
namespace laura {

// ---- full-sequence form -------------------------------------------------------------------------------------------------
// y = [relu](LayerNorm_C(x [+ add])) * post_scale;  sum_out (may alias x) receives x + add.  x, add, y: [B][C][T]
hipError_t launch_layernorm_fm(const float* x, const float* add, float* sum_out, const float* gamma, const float* beta, float eps,
                               int relu, float post_scale, float* y, int B, int C, int T, hipStream_t st);
// in-place activation over n floats: 1 = relu, 2 = swish (x * sigmoid(x))
hipError_t launch_act(float* x, size_t n, int act, hipStream_t st);

struct AttnFull {
    const float* qkv = nullptr;     // [B][3 d][T]: rows [0, d) q, [d, 2d) k, [2d, 3d) v
    const float* ptab = nullptr;    // [d][PR]: linear_pos(pe(r)) at column r + R - 1
    const float* bias_u = nullptr;  // [d] (= [h][dk])
    const float* bias_v = nullptr;
    const int* lens = nullptr;      // device [B]: keys >= lens[b] are masked
    const int* bidir = nullptr;     // device [B] or null: with causal, rows and columns < bidir[b] see each other
    int causal = 0;
    float* ctx = nullptr;           // [B][d][T]
    int B = 0, H = 0, DK = 64, T = 0, R = 0, PR = 0;
};
size_t attn_full_lds_bytes(int T);
hipError_t launch_attn_full(const AttnFull& a, hipStream_t st);

// [B][L][D] token-major (rows t >= lens[b] ignored) -> [B][D][T] feature-major, zero for t >= lens[b]
hipError_t launch_tm_to_fm(const float* in, const int* lens, int B, int L, int D, int T, float* out, hipStream_t st);
// [B][D][T] -> [B][L][D], rows t >= lens[b] zero
hipError_t launch_fm_to_tm(const float* in, const int* lens, int B, int D, int T, int L, float* out, hipStream_t st);
// token ids [B][L] (i64, < 0 = padding) -> table rows, feature-major [B][D][T]
hipError_t launch_token_embed_fm(const int64_t* ids, const float* table, int vocab, int B, int L, int D, int T, float* out, hipStream_t st);

// LM input (LauraGenModel.build_llm_io, laura_model.py:204-247): [sos, text, task_id, codec embeddings] per utterance.
//   text_fm [B][D][Tt]; lm_emb [2][D]; cb [nq_all][K][D]; codec [B][Cmax][nq] (i64) or null; out [B][D][T]; seq_len[b] written
hipError_t launch_lm_assemble(const float* text_fm, int Tt, const int* text_lens, const float* lm_emb, const float* cb, int K, int nq,
                              const int64_t* codec, const int* codec_lens, int Cmax, int B, int D, int T, float* out, int* seq_len,
                              int* bidir_len, hipStream_t st);
// fine-predictor input (cal_codec_emb, laura_model.py:296-322): [text, sum of the first nq codebook rows]; split: each part gets
// x * sqrt(D) + pe_abs[position within the part]
hipError_t launch_nar_assemble(const float* text_fm, int Tt, const int* text_lens, const float* cb, int K, int nq, const int64_t* codec,
                               const int* codec_lens, int Cmax, int codec_stride_nq, const float* pe_abs, int split, int B, int D, int T,
                               float* out, int* seq_len, hipStream_t st);
// out [B][Cmax][D] token-major = in [B][D][T] columns text_lens[b] .. text_lens[b] + codec_lens[b] - 1 (zero rows past it)
hipError_t launch_nar_extract(const float* in, const int* text_lens, const int* codec_lens, int B, int D, int T, int Cmax, float* out,
                              hipStream_t st);
// log-softmax over the V rows of every column: in [B][V][T] -> out [B][L][V] (rows t >= lens[b] zero)
hipError_t launch_logsoftmax_fm(const float* in, const int* lens, int B, int V, int T, int L, float* out, hipStream_t st);
// K / V rows of a full-sequence QKV buffer into the step form's caches: kc [B][d][Tcap] (feature-major), vc [B][Tcap][d]
hipError_t launch_kv_store(const float* qkv, const int* lens, int B, int d, int T, int Tcap, float* kc, float* vc, hipStream_t st);
// x_last[b][c] = x[b][c][lens[b] - 1]   ([16][C] token-major, rows >= B untouched)
hipError_t launch_gather_last(const float* x, const int* lens, int B, int C, int T, float* out, hipStream_t st);

// A prefix pass of n DIFFERENT prompts for a decoding session (fc_laura_slots_start_many): batch row b belongs to session slot
// slot[b].  By value in the kernel arguments, like the lengths.
struct RowSlots {
    int n = 0;
    int slot[16] = {};
};
// launch_kv_store with a destination slot per batch row: kc [S][d][Tcap], vc [S][Tcap][d] are one layer's caches of the session
hipError_t launch_kv_store_slots(const float* qkv, const int* lens, const RowSlots& rs, int S, int d, int T, int Tcap, float* kc, float* vc,
                                 hipStream_t st);
// xs[slot[b]][c] = x[b][c][lens[b] - 1] and pos[slot[b]] = lens[b]   (xs [S][C] token-major, pos [S]; other slots untouched)
hipError_t launch_gather_last_slots(const float* x, const int* lens, const RowSlots& rs, int S, int C, int T, float* xs, int* pos,
                                    hipStream_t st);

// ---- step form ------------------------------------------------------------------------------------------------------------
struct Gemv {
    const float* x = nullptr;       // [B][K] token-major
    const float* wf = nullptr;      // fragment order [ceil(N/16)][K/16][64 lanes][4]
    const float* bias = nullptr;    // [N]
    const float *gamma = nullptr, *beta = nullptr;   // LayerNorm over K applied to x first (null: none)
    float eps = 0.f;
    int act = 0;                    // 0 none, 1 relu, 2 swish
    int mode = 0;                   // 0: y[b][n] = v   1: y[b][n] += v   2: q / K-cache / V-cache scatter
    float* y = nullptr;             // [B][ldy]
    int ldy = 0;
    // mode 2: n < d -> y[b][n];  d <= n < 2d -> kc[b][n - d][pos[b]];  else vc[b][pos[b]][n - 2d]
    float *kc = nullptr, *vc = nullptr;
    const int* pos = nullptr;
    int d = 0, Tcap = 0;
    int B = 0, K = 0, N = 0;
    // x given as the key-range partials of the step attention (combined while staging): [B][H][NS][DK + 2], K = H * DK
    const float* apart = nullptr;
    int H = 0, DK = 0, NS = 0;
    // how x is staged in LDS: 0 = one stage when (16 + 1) x (K + 4) floats fit, else windows of <= 1024 columns (x as given, modes 0 / 1);
    // test hooks: 1 = one stage whatever the batch allows, 2 = at least two windows
    int stage = 0;
    // the instantiations over column blocks (gemv_column_block) also when B <= 16 leaves grid.y = 1: a launch cut to the first blocks of a
    // wider step (fc_laura_slots_set_elastic) runs the kernels of the full launch, whatever the cut
    int wide = 0;
};
// 1 <= B <= 64.  The stage form, the waves per workgroup and the window count follow from K alone, as for 16 rows: a row's accumulation
// order does not depend on B or on the row's column block.
hipError_t launch_gemv(const Gemv& g, hipStream_t st);
// rows of x [B][C] in place: [relu](LayerNorm(x)) * post_scale
hipError_t launch_layernorm_rows(float* x, const float* gamma, const float* beta, float eps, int relu, float post_scale, int B, int C,
                                 hipStream_t st);

struct AttnStep {
    const float* q = nullptr;       // [B][d]
    const float *kc = nullptr, *vc = nullptr;   // caches of this layer: [B][d][Tcap], [B][Tcap][d]
    const float *ptab = nullptr, *bias_u = nullptr, *bias_v = nullptr;
    const int* pos = nullptr;       // device [B]: position of the query (keys 0 .. pos[b])
    float* part = nullptr;          // [B][H][NS][DK + 2]: per key range the unnormalised context, running max, sum of exponentials
    int NS = 1;                     // key ranges per (utterance, head): B * H * NS workgroups
    int B = 0, H = 0, DK = 64, Tcap = 0, R = 0, PR = 0;
};
hipError_t launch_attn_step(const AttnStep& a, hipStream_t st);

// per-row sampling parameters of a decoding session (device table [B]): what a decode_codec call fixes for all its rows
struct SampleRow {
    int mode, ki;
    float pf;
    int max_steps;
    unsigned long long seed;
    int forced_on;                  // 0: this row samples even when the launch has a forced-token buffer
    unsigned rng_row;               // second word of the row's Philox counter (decode_codec: the batch row)
    // the slot's sampling rules (fc_laura_slots_set_rules; the defaults are the neutral rules: the sampler without them, bit for bit)
    float temperature = 1.f;        // logits are divided by it, finite and > 0
    int min_length = 0;             // <eos> is -inf in every group while fewer tokens than this are generated
    float top_p = 0.f;              // mode 2 only, 0 = none: the top-k candidates cut to the nucleus of top_p
    int repeat_window = 0;          // 0 = off, <= 256: a drawn id that fills the last repeat_window generated tokens of its group ...
    int repeat_count = 1;           // ... at least repeat_count times is drawn again from the whole group
};

struct Sample {
    const float* logits = nullptr;  // [B][V], V = nq * (K + 1)
    int B = 0, K = 0, nq = 0;
    int mode = 0;                   // 0 greedy, 1 softmax, 2 top-k (ki), 3 nucleus (pf)
    int ki = 0; float pf = 0.f;
    unsigned long long seed = 0;
    const int64_t* forced = nullptr;    // [B][max_steps][nq] or null: teacher forcing (the sampled ids are replaced)
    int max_steps = 0;
    int64_t* tokens = nullptr;      // [B][tok_stride][nq]; generated token g of b goes to row tok_off[b] + g
    int tok_stride = 0;
    const int* tok_off = nullptr;   // device [B]
    int* n_gen = nullptr;           // device [B]: tokens generated so far (incremented here)
    int* done = nullptr;            // device [B]
    int* n_done = nullptr;          // device [1]: number of finished utterances (host polls a copy)
    int* pos = nullptr;             // device [B]: cache fill, incremented for utterances still running
    int* step = nullptr;            // device [B]: samples drawn so far per utterance (RNG stream position), incremented
    float* logp_out = nullptr;      // [B][max_steps][V] or null: log-softmax the step sampled from
    float* score_out = nullptr;     // [B][max_steps] or null: the log-probability of the step's final picks (see sample_kernel)
    const float* cb = nullptr;      // [nq_all][K][D] codebook table: next LM input = sum_k cb[k][tok_k]
    int D = 0;
    float* next_emb = nullptr;      // [B][D]
    // optional fusion of the LM's input layer for the next step: xs[b] = [relu](LayerNorm_1e-5(W e + bias)) * xscale
    const float *emb_wt = nullptr, *emb_bias = nullptr, *emb_g = nullptr, *emb_b = nullptr;   // emb_wt [D][dm] = W transposed
    int dm = 0, emb_relu = 0;
    float xscale = 1.f;
    float* xs = nullptr;            // [B][dm]
    unsigned* launch_seq = nullptr; // device word incremented once per launch (the persistent step kernel's launch number), or null
    // decoding session: mode / ki / pf / seed / max_steps / forced on-off / Philox row word per row instead of the fields above; forced,
    // logp_out and score_out then have row_stride steps per row.  null: exactly the launch a decode_codec call makes
    const SampleRow* rows = nullptr;
    int row_stride = 0;
    int row0 = 0, nrows = 0;        // rows row0 .. row0 + nrows - 1 only (nrows 0: all B)
};
hipError_t launch_sample(const Sample& s, hipStream_t st);

struct SlotReset {                  // see slot_reset_kernel
    int slot = 0, free_slot = 0;    // free_slot: leave the slot ended (done = 1), as a never-started one is
    int *n_gen = nullptr, *done = nullptr, *step = nullptr, *pos = nullptr, *tok_off = nullptr;
    SampleRow* rows = nullptr;
    SampleRow row{};
    float* xs = nullptr;
    int dm = 0;
    int64_t* tokens = nullptr;      // [S][tok_stride][nq]
    int tok_stride = 0, nq = 0, cont_len = 0;
    const int64_t* continual = nullptr;   // [cont_len][nq]
    int64_t* forced = nullptr;      // [S][tok_stride][nq]
    const int64_t* forced_src = nullptr;  // [row.max_steps][nq] or null
    float* logp = nullptr;          // [S][tok_stride][V] or null
    int V = 0;
    float* score = nullptr;         // [S][tok_stride] or null
};
hipError_t launch_slot_reset(const SlotReset& r, hipStream_t st);

struct PrefixImport {               // see prefix_import_kernel: a slot's prefix into a slot of the same or another session of one engine
    const float *kc_src = nullptr, *vc_src = nullptr;   // the source session's caches [NL][S_src][d][Tcap_src], [NL][S_src][Tcap_src][d]
    float *kc_dst = nullptr, *vc_dst = nullptr;         // the destination session's, with S_dst and Tcap_dst
    const float* lg0_src = nullptr; // [S_src][V] logits every source slot's prefix ended with
    float *lg_dst = nullptr, *lg0_dst = nullptr;        // [S_dst][V]
    int* pos_dst = nullptr;         // device [S_dst]
    int NL = 0, d = 0, V = 0;
    int S_src = 0, Tcap_src = 0, S_dst = 0, Tcap_dst = 0;
    int P = 0;                      // prefix positions of the source's prompt
    int src = 0, dst = 0;
};
hipError_t launch_prefix_import(const PrefixImport& c, hipStream_t st);

struct SlotBranch {                 // see slot_branch_kernel
    int S = 0, dst = 0, src = 0;    // dst == src: in place
    int keep = 0;                   // generated tokens of the source that stay, >= 1
    int P = 0;                      // prefix positions of the prompt (text_len + 2 + cont_len)
    int *n_gen = nullptr, *done = nullptr, *step = nullptr, *pos = nullptr, *tok_off = nullptr;
    SampleRow* rows = nullptr;
    SampleRow row{};                // dst's own; forced_on is the source's
    int64_t* tokens = nullptr;      // [S][tok_stride][nq]
    int tok_stride = 0, nq = 0, cont_len = 0;
    int64_t* forced = nullptr;      // [S][tok_stride][nq]
    int forced_rows = 0;            // rows of the source's forced tokens (its max_length)
    float* logp = nullptr;          // [S][tok_stride][V] or null
    int V = 0;
    float* score = nullptr;         // [S][tok_stride] or null
    // the LM's next input from kept token keep - 1: the fields of Sample of the same names
    const float* cb = nullptr;
    int K = 0, D = 0;
    float* next_emb = nullptr;
    const float *emb_wt = nullptr, *emb_bias = nullptr, *emb_g = nullptr, *emb_b = nullptr;
    int dm = 0, emb_relu = 0;
    float xscale = 1.f;
    float* xs = nullptr;
};
hipError_t launch_slot_branch(const SlotBranch& r, hipStream_t st);

struct SlotMoves {                  // see slot_move_kernel: slots of a decoding session moved to other rows, all in one launch
    int* table = nullptr;           // device [1 + 2 * 64] ints: the line count n, then n lines (src, dst); written by launch_slot_moves_put
    float *kc = nullptr, *vc = nullptr;   // the session's caches [NL][S][d][Tcap], [NL][S][Tcap][d]
    int *n_gen = nullptr, *done = nullptr, *step = nullptr, *pos = nullptr, *tok_off = nullptr;
    SampleRow* rows = nullptr;
    int64_t *tokens = nullptr, *forced = nullptr;       // [S][R][nq]
    float* logp = nullptr;          // [S][R][V] or null
    float* score = nullptr;         // [S][R] or null
    float *lg = nullptr, *lg0 = nullptr;                // [S][V]
    float *xs = nullptr, *nemb = nullptr;               // [S][d], [S][D]
    int NL = 0, S = 0, d = 0, Tcap = 0, V = 0, R = 0, nq = 0, D = 0;
};
enum { FC_SLOT_MOVES_MAX = 64, FC_SLOT_MOVES_WORDS = 1 + 2 * FC_SLOT_MOVES_MAX };
struct SlotMoveLines { int n = 0; int src[FC_SLOT_MOVES_MAX] = {}, dst[FC_SLOT_MOVES_MAX] = {}; };
// the lines into the device table (one small launch, the lines by value in the kernel arguments, like a queue ticket), then the copy
hipError_t launch_slot_moves(const SlotMoves& m, const SlotMoveLines& lines, hipStream_t st);

hipError_t launch_fill_i32(int* p, int v, int n, hipStream_t st);

// ---- the refill phase of a QUEUED decoding session (fc_laura_slots_create_queued) -------------------------------------------------
// A ticket waits in a ring of descriptors; at the start of every step the session retires its ended slots into a result ring and
// claims waiting tickets into its free slots, all from device memory: the launches and their arguments never change, so the phase is
// part of the captured step.  No kernel of the phase waits on anything; the order comes from the launches.
struct QueueTicket {                // one waiting ticket, written by queue_put_kernel
    int row = 0;                    // the row of the source session that holds the prompt
    int P = 0, cont_len = 0;        // its prefix positions and continual prompt length, as the host knew them at the submit
    int entry = 0;                  // the result entry the ticket retires into
    SampleRow srow{};               // the slot's row of the sampling table (mode, seed, max_length, rules)
};
struct QueueClaim { int slot, row, P, cont_len; };      // a claim of this step: the ticket's prompt into `slot`
struct QueueRetire { int slot, entry, n_tok, pad; };    // a slot retired in this step: its first n_tok token rows into `entry`

// words of the queue block (device ints, read back with every step): the counters, then the ticket each slot runs (-1: none) and the
// result entry that ticket retires into, 64 slots each; behind them FC_QUEUE_META words per result entry
enum { FC_QUEUE_HEAD = 0, FC_QUEUE_TAIL = 1, FC_QUEUE_FINISHED = 2, FC_QUEUE_NRETIRE = 3, FC_QUEUE_NCLAIM = 4, FC_QUEUE_SLOT_TICKET = 16,
       FC_QUEUE_SLOT_ENTRY = 80, FC_QUEUE_WORDS = 144 };
// a result entry's words: state (0 free, 1 waiting or running, 2 finished), ticket, token rows (prompt + generated), generated tokens,
// ended on <eos>, the order of finishing (0, 1, ...)
enum { FC_QUEUE_META = 8, FC_QMETA_STATE = 0, FC_QMETA_TICKET = 1, FC_QMETA_NTOK = 2, FC_QMETA_NGEN = 3, FC_QMETA_EOS = 4, FC_QMETA_SEQ = 5 };

struct QueuePhase {
    int* qw = nullptr;              // the queue block: FC_QUEUE_WORDS + Q * FC_QUEUE_META ints
    QueueTicket* ring = nullptr;    // [Q]: ticket t waits at t % Q
    QueueClaim* claims = nullptr;   // [64]
    QueueRetire* retires = nullptr; // [64]
    int Q = 0, S = 0;
    // the queued session: counters, sampling table, rows (R positions per slot), caches
    int *n_gen = nullptr, *done = nullptr, *step = nullptr, *pos = nullptr, *tok_off = nullptr;
    SampleRow* rows = nullptr;
    int64_t* tokens = nullptr;      // [S][R][nq]
    float* score = nullptr;         // [S][R] or null
    float* xs = nullptr;            // [S][dm]
    float *kc = nullptr, *vc = nullptr, *lg = nullptr, *lg0 = nullptr;
    int R = 0, nq = 0, dm = 0, NL = 0, d = 0, V = 0;
    int64_t* ring_tokens = nullptr; // [Q][R][nq]
    float* ring_score = nullptr;    // [Q][R] or null
    // the source session (never this one): caches, prefix logits, token rows
    const float *kc_src = nullptr, *vc_src = nullptr, *lg0_src = nullptr;
    const int64_t* tokens_src = nullptr;
    int S_src = 0, R_src = 0;
};
// ticket number `ticket` into the ring (one thread; the ticket by value in the kernel arguments, like the lengths)
hipError_t launch_queue_put(const QueuePhase& q, const QueueTicket& t, int ticket, hipStream_t st);
// the phase: queue_turn_kernel (retire, and with claim != 0 claim), queue_retire_copy_kernel, and with claim != 0 queue_claim_copy_kernel
hipError_t launch_queue_phase(const QueuePhase& q, int claim, hipStream_t st);
// launch_sample over the slots claimed in this step: block i samples row claims[i].slot, blocks >= the claim count exit at once
hipError_t launch_sample_claims(const Sample& s, const QueuePhase& q, hipStream_t st);

// ---- step form as ONE persistent launch (laura_persist.hip) ------------------------------------------------------------------------
struct StepLayer {          // constant device pointers of one block (fragment-order weights of the step form, biases padded to row tiles)
    const float *wqkv, *bqkv, *wout, *bout, *wff1, *bff1, *wff2, *bff2;
    const float *n1g, *n1b, *n2g, *n2b, *bu, *bv, *ptab;
};
struct StepPersistArgs {
    const StepLayer* layers;        // device [NL]
    const float *wdec, *bdec;       // output layer (fragment order), bias
    const float *ag, *ab;           // after_norm
    const float* xs;                // [16][d]: LM input of this step (written by the sampler of the previous step)
    float* logits;                  // [16][V]
    float* edge;                    // NL x edge_stride floats: per block q [16][d] | partials [B][H][NS][DK + 4] | xm [16][d] | h [16][ff] | x_out [KS2][16][d]
    float *kc, *vc;                 // KV caches [NL][B][d][Tcap] / [NL][B][Tcap][d]
    const int* pos;                 // device [B]
    unsigned* sync;                 // arrival counters (step_persist_sync_words), zeroed once per decode call
    const unsigned* seq;            // device word: number of this launch within the call (1, 2, ...), incremented by the sampler
    size_t edge_stride;
    int o_q, o_ap, o_xm, o_hb, o_xo;
    int B, d, ff, H, DK, NL, V, Tcap, R, PR, NS, act, G;
    int KS2;                        // k slices of w_2 (step_persist_ksplit)
    int wtile;                      // floats of one LDS weight tile (set by launch_step_persist)
    unsigned long long* trace;      // tuning aid (FC_LAURA_TRACE): [G][64 units][8] s_memtime stamps of the last launch, or null
    int test_timeout;               // test hook (FC_LAURA_PERSIST_TEST=timeout): behave as if a hand-off had timed out
};
int step_persist_ksplit(int d, int ff);
size_t step_persist_sync_words(int NL);
size_t step_persist_lds_bytes(int B, int d, int ff, int H, int DK);
bool step_persist_supported(int B, int d, int ff, int H, int DK, int V, int NS);
int step_persist_grid(int device, int d, int ff);          // workgroups of the persistent launch (0: not launchable here)
hipError_t launch_step_persist(const StepPersistArgs& a, hipStream_t st);

}  // namespace laura
}  // namespace fc
