// Engine: layer plan, checkpoint ingestion / weight re-layout, workspace planning and the C ABI
// (include/funcodec_amd.h).  All device work is enqueued on the caller's stream; nothing here
// synchronises with the host after fc_engine_finalize().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/funcodec_amd.h"
#include "kernels.h"
#include "rvq_beam_kernels.h"
#include "rvq_rate_kernels.h"
#include "laura_kernels.h"
#include "ragged_kernels.h"
#include "seq_kernels.h"
#include "slots_kernels.h"
#include "stream_kernels.h"

namespace {

thread_local std::string g_err;

int fail(const std::string& msg) { g_err = msg; return 1; }
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

struct HostTensor {
    std::vector<int64_t> dims;
    std::vector<float> data;
    bool set = false;
};

struct DevBuf {
    float* p = nullptr;
    size_t n = 0;
};

// One SConv1d / SConvTranspose1d (+ its GroupNorm) of the plan.
struct ConvLayer {
    std::string prefix;     // e.g. "encoder.model.3.conv" / "decoder.model.3.convtr"
    bool transposed = false;
    int cin = 0, cout = 0, k = 1, stride = 1, dil = 1;
    bool has_norm = true;   // GroupNorm(1, cout) after the conv
    bool wnorm = false;     // checkpoint stores weight_g / weight_v (torch.nn.utils.weight_norm)
    bool causal = false;
    bool dual = false;      // the plan feeds it two summed sources (residual sum / LSTM skip)
    bool small_n = false;   // runs at the bottleneck frame rate: few columns per utterance
    // 2-D layers (STFT-domain codec), frequency-major layout: a Conv2d (kf x k, stride sf x stride) over c2d channels is the 1-D
    // conv (k, stride) over cin = kf * c2d channels of the virtual utterance starting at frequency row fo * sf
    int kf = 1, sf = 1, c2d = 0;
    bool extra_left = false;    // SConv2d puts the "extra" time padding on the LEFT (conv.py:377), SConv1d on the right
    bool valid = false;         // no padding at all (the STFT GEMM)
    int zpadL = -1, zpadR = -1; // explicit ZERO padding (the inverse-STFT GEMM); -1: reference padding rules
    bool synthetic = false;     // weights generated at finalize (DFT matrices), not part of the checkpoint
    int groups = 1;             // grouped Conv2d / ConvTranspose2d (conv_group_ratio > 0): dense block-diagonal weight at finalize
    float* w_group = nullptr;   // grouped Conv2d with 2 / 4 channels per group: torch-layout weights for the direct kernel (freq_kernels.hip)
    bool force_plain = false;   // the slab of the fused-prologue variants does not fit (large strides): materialise the input first
    bool unsupported = false;   // no variant fits (stride > ~17): refused at fc_engine_create
    // GEMM view
    int M = 0, gk = 1, gstride = 1;    // rows, taps, stride of the implicit GEMM
    int BM = 128, BN = 128, CC = 2, nchunk = 1, Mpad = 0;
    bool row = false;       // stride-1 row staging (kernels.hip)
    float* w_plain = nullptr;   // device [cin][k] when cout == 1 (FMA kernel instead of a 32-row MFMA tile)
    float bias0 = 0.f;
    float *wt = nullptr, *bias = nullptr, *gamma = nullptr, *beta = nullptr;   // device
    int* koff = nullptr;                                                        // device
};

struct LstmLayer {
    ConvLayer inproj;       // W_ih as a k=1 GEMM with permuted rows, bias = b_ih + b_hh
    float* whh = nullptr;   // [4H][H] rows permuted to (blk, unit, gate)
    float* wcat = nullptr;  // layers >= 1: [4H][2H] = [W_ih | W_hh], same row permutation (wavefront kernel)
    float* bperm = nullptr; // layers >= 1: permuted b_ih + b_hh
};

struct LstmBlock {
    std::string prefix;     // "encoder.model.16.lstm"
    int H = 0;
    std::vector<LstmLayer> layers;
};

// TransformerEncoder at the bottleneck (seq_model: transformer; normed_modules/transformer.py:26-208): pre-LayerNorm blocks, every
// Linear a k = 1 layer of the implicit-GEMM conv kernel over feature-major [B][C][T] activations
struct TfLayer {
    ConvLayer qkv;          // linear_q | linear_k | linear_v as ONE GEMM of 3 C rows (weights concatenated at pack time)
    ConvLayer out, ff1, ff2;    // linear_out, feed_forward.w_1, feed_forward.w_2
    float *n1g = nullptr, *n1b = nullptr, *n2g = nullptr, *n2b = nullptr;   // norm1, norm2
};

struct TfBlock {
    std::string prefix;     // "encoder.model.16"
    int C = 0, heads = 4, ff = 2048;
    std::vector<TfLayer> layers;
    float *ag = nullptr, *ab = nullptr;   // after_norm
};

struct Act {               // raw tensor [B][C][T] + pending GroupNorm affine (null = already final)
    float* raw = nullptr;
    float* aff = nullptr;
    int C = 0, T = 0;
    bool normed = false;   // has a pending affine (valid in dry-run planning too, where pointers are null)
    int ld = 0;            // row pitch when it is not T (ragged pass: the untrimmed output of a transposed conv)
};

int ceil_div_i(int a, int b) { return (a + b - 1) / b; }

const char* kLstmPersistClass = "lstm_persist_kernel<NS> (whole recurrence of one SLSTM block, one launch)";
const char* kLstmWaveClass = "lstm_wave_kernel<NS> (whole recurrence of one SLSTM block: T + L - 1 launches incl. gaps)";
const char* kRvqClass = "rvq_encode_kernel<D, RS> (all stages of the residual quantiser)";
const char* kRvqBeamClass = "rvq_beam_kernel<D, W> (beam search over the stages of the residual quantiser)";

}  // namespace

struct fc_engine {
    fc_arch arch;
    int device = 0;
    bool finalized = false;
    std::vector<std::pair<std::string, std::vector<int64_t>>> expected;   // checkpoint contract, in plan order
    std::map<std::string, HostTensor> host;
    // plan
    ConvLayer enc_first, enc_last, dec_first, dec_last;
    struct ResBlock {                                                     // SEANetResnetBlock: shortcut(x) + block(x)
        ConvLayer shortcut, block1, block3;
        bool fused_head = false;                // shortcut + block.1 in one launch (thin blocks, kernels.hip 1c)
        float *wsc = nullptr, *wb1 = nullptr;   // LDS images of the two weight matrices for that kernel
        float *bsc = nullptr, *bb1 = nullptr;
    };
    struct Stage { std::vector<ResBlock> res; ConvLayer resample; };      // n_residual_layers blocks; resample = down (enc) / up (dec)
    std::vector<Stage> enc_stages, dec_stages;
    LstmBlock enc_lstm, dec_lstm;
    TfBlock enc_tf, dec_tf;                                               // seq_model 1 (transformer) instead of the LSTMs
    std::map<std::string, TfBlock*> tf_by_prefix;
    std::map<std::string, ConvLayer*> by_prefix;
    std::map<std::string, ResBlock*> res_by_prefix;
    // STFT-domain codec (arch.model_type == 1)
    ConvLayer enc2_first, dec2_last, stft, istft;
    ConvLayer q_in, q_out;                                                 // CostumeQuantizer.input_proj / output_proj as k = 1 GEMMs (codec_dim != dimension)
    bool q_proj = false;
    int cdim() const { return q_proj ? arch.codec_dim : arch.dimension; }
    // audio channels of the time-domain codec (wav / recon buffers are [B][C][T]); FreqCodec is mono (codec_freq.py squeezes dim 1)
    int audio_ch() const { return arch.model_type == 0 && arch.input_channels == 2 ? 2 : 1; }
    std::vector<std::vector<ConvLayer>> dec_up_phases;                    // decoder stage s: one transposed 1-D GEMM per frequency phase
    int halo2 = 3;                                                        // frequency halo rows of the 2-D activations
    float* win2 = nullptr;                                                // squared Hann window [n_fft] (istft envelope)                       // "encoder.model.1" -> block (fc_resblock_forward)
    std::map<std::string, LstmBlock*> lstm_by_prefix;
    // quantiser
    float *cb = nullptr, *enorm = nullptr;   // [nq][K][D], [nq][K]
    float* cb_frag = nullptr;                // the codebooks in MFMA B-fragment order (rvq_kernels.hip rvq_encode_kernel), or null
    std::vector<void*> dev_allocs;
    // status words written by kernels (host-pinned, device-mapped; kernels.h FC_STATUS_*), read at the next call without a sync
    volatile unsigned* status_host = nullptr;
    unsigned* status_dev = nullptr;
    // per-row stage counts of the calls that follow (fc_engine_set_row_nq): the host copy (empty = none set) and the device table the
    // quantiser kernels index by batch row; the table only grows, so a launch still in flight never loses it
    std::vector<int32_t> row_nq;
    int* row_nq_dev = nullptr;
    size_t row_nq_cap = 0;
    int rvq_beam = 1;                        // width of the quantiser's search over the stages for the calls that follow (fc_engine_set_rvq_beam); 1: greedy
    // a stage count per row chosen on the device by a target SNR, for the offline calls that follow (fc_engine_set_rate; csrc/rvq_rate_kernels.h
    // states the rule): the host copy of the ratios (empty = none set), their device copy and the table of chosen counts -- NOT row_nq_dev,
    // which still holds the caps the first pass read.  Both tables only grow, like row_nq_dev.  The three outputs are the caller's.
    struct Rate {
        std::vector<double> ratio;
        int min_nq = 1;
        double* ratio_dev = nullptr;
        int* k_dev = nullptr;
        size_t cap = 0;
        int32_t* n_q_out = nullptr;
        double* row_err_out = nullptr;
        float* stage_err_out = nullptr;
        // frame mode (fc_engine_set_rate_frames; the frame rule of csrc/rvq_rate_kernels.h): a count per frame; min_nq may then be 0
        bool frames = false;
        int32_t* nq_frames_out = nullptr;
        int32_t* n_codes_out = nullptr;
        double* achieved_out = nullptr;
        bool on() const { return !ratio.empty(); }
        void clear_frames() { frames = false; nq_frames_out = nullptr; n_codes_out = nullptr; achieved_out = nullptr; }
    } rate;
    // a stage count per row chosen on the device by a noise floor, for the encode pushes of sessions that follow (fc_engine_set_floor; the
    // push rule of csrc/rvq_rate_kernels.h): the host copy of the floors (empty = none set) and their device copy, which only grows.  The
    // count table is the caller's.  chain, row_err_out, stage_err_out: fc_engine_set_floor_form.
    struct Floor {
        std::vector<double> floor;
        int min_nq = 1;
        double* floor_dev = nullptr;
        size_t cap = 0;
        int32_t* n_q_out = nullptr;
        bool chain = false;
        double* row_err_out = nullptr;
        float* stage_err_out = nullptr;
        float* subq_out = nullptr;              // of the hook alone (a push has no sub_quants)
        // a count per frame of the push (fc_engine_set_floor_frames; the push frame rule): the caller's table [B][Tf of the push]; min_nq
        // may then be 0, and n_q_out is not written
        int32_t* nq_frames_out = nullptr;
        bool on() const { return !floor.empty(); }
        void clear_form() { chain = false; row_err_out = nullptr; stage_err_out = nullptr; subq_out = nullptr; }
    } floor;
    // a stage count per frame for the offline decode_codes calls that follow (fc_engine_set_frame_nq): the caller's device table, borrowed
    struct FrameNq { const int32_t* table = nullptr; int B = 0, Tf = 0; } frame_nq;
    // the same for the session decode pushes that follow (fc_engine_set_push_frame_nq): [B][Tfc of the push], borrowed
    FrameNq push_nq;
    bool lstm_persist_ok = true;             // cleared after a grid-barrier timeout: later calls take the per-step launch path
    int persist_checked_B = -1; bool persist_checked_val = false;
    // optional event timing
    bool profiling = false;
    struct Span { hipEvent_t a, b; int cls; double flops, bytes; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;
    size_t events_used = 0;
    std::vector<std::string> prof_names;     // class id -> kernel name as rocprofv3 prints it
    int prof_class(const std::string& name) {
        for (size_t i = 0; i < prof_names.size(); ++i)
            if (prof_names[i] == name) return (int)i;
        if ((int)prof_names.size() >= FC_PROF_CLASSES) return FC_PROF_CLASSES - 1;
        prof_names.push_back(name);
        return (int)prof_names.size() - 1;
    }
};

// What both kinds of session of a causal time-domain engine keep.  Everything that survives a push lives in `state`, ONE device allocation
// of the caller (fc_stream_state_bytes; stream_layout): [scale B] [per conv with a left context: carry [2][B][cin][pt], ping-pong on the
// parity of the side's push count] [encoder LSTM h [L][2][B][H] | c [L][B][H]] [decoder LSTM the same], and behind them, in a session
// opened with max_frames for a transformer bottleneck (fc_seqstream_create), the key / value caches: per side, per block, K [B][C][F]
// then V [B][C][F], F = seq_cache_pitch(max_frames).
struct Session {
    fc_engine* e = nullptr;
    int B = 0, max_chunk = 0, n_q = 0;              // B: the rows of a push (utterances in lock-step / slots)
    float* state = nullptr;
    size_t state_floats = 0;
    std::map<const ConvLayer*, size_t> carry;       // float offset of the layer's carry pair inside state
    size_t enc_lstm_off = 0, dec_lstm_off = 0;
    int max_frames = 0;                             // the bound of an utterance's frames per side; 0: no transformer in this session
    size_t enc_kv_off = 0, dec_kv_off = 0;          // float offsets of the two sides' key / value caches; carried_floats: what lies in front
    size_t carried_floats = 0;                      // of them and is cleared at reset (the caches are written before they are read)
    int enc_min_first = 0, dec_min_first = 0;       // shortest first push: samples (a hop multiple) / frames
    std::vector<float> ones;

    // Graph replay of the session's pushes (fc_graphstream_set, fc_graphslots_set; include/funcodec_amd.h).  The key of a captured push holds every host value
    // its enqueued work depends on (DESIGN.md section 8 lists the walk's host values and where each one lives); everything else the
    // launches read lies in device memory and is read at replay.
    struct GraphKey {
        int form = 0;                               // 0 encode, 1 decode_codes, 2 decode_emb (which also names the side)
        int width = 0, parity = 0, n_q = 0, use_scale = 0;
        std::array<const void*, 5> ptr{};           // inputs, outputs (null: absent) and the slot push's scale
        const void* ws = nullptr; size_t ws_bytes = 0;
        const void* stream = nullptr;
        const void* nq_table = nullptr; int nq_rows = 0;      // per-row stage counts: null / 0 when none are set
        int rvq_beam = 1;                           // width of the quantiser's search (fc_engine_set_rvq_beam): more launches above 1
        // the noise floor of an encode push (fc_engine_set_floor): its tables' addresses, min_nq and form; the floors themselves are device data
        const void* floor_table = nullptr; const void* floor_out = nullptr; int floor_min = 0, floor_chain = 0;
        const void* floor_frames = nullptr;         // frame mode (fc_engine_set_floor_frames): the count table per frame, else null
        const void* push_nq = nullptr;              // a decode push under a count per frame (fc_engine_set_push_frame_nq): its table
        bool operator==(const GraphKey& o) const {
            return form == o.form && width == o.width && parity == o.parity && n_q == o.n_q && use_scale == o.use_scale && ptr == o.ptr && ws == o.ws &&
                   ws_bytes == o.ws_bytes && stream == o.stream && nq_table == o.nq_table && nq_rows == o.nq_rows &&
                   rvq_beam == o.rvq_beam && floor_table == o.floor_table && floor_out == o.floor_out && floor_min == o.floor_min &&
                   floor_chain == o.floor_chain && floor_frames == o.floor_frames && push_nq == o.push_nq;
        }
    };
    struct Graph { GraphKey key; hipGraphExec_t exec = nullptr; unsigned long long used = 0; };
    static constexpr size_t kMaxGraphs = 16;
    bool graph_on = false;
    std::vector<Graph> graphs;                      // at most kMaxGraphs; the least recently used one is evicted
    unsigned long long graph_tick = 0;
    int64_t graph_counts[4] = {0, 0, 0, 0};         // replays, captures, evictions, fallbacks since create
    void drop_graphs() {
        for (Graph& g : graphs) (void)hipGraphExecDestroy(g.exec);
        graphs.clear();
    }

    // The slot record (slots_kernels.h states it): the session's segment table, built at create (record_layout) and held in device
    // memory, with room behind it for the named slots of one export / import call, which travel there in one copy in front of the launch.
    struct Record {
        std::vector<fc::SlotSeg> segs;
        uint32_t layout = 0;                        // the fingerprint of the segment list (fc_slot_meta.layout)
        size_t fixed = 0;                           // floats of a record without its cache planes
        int enc_cols = 0, dec_cols = 0;             // cache rows per side: a record holds enc_cols * Fr(enc frames) + dec_cols * Fr(dec frames) more
        int max_len = 0, max_rows = 0;              // the longest plain segment and the widest cache plane (they size the launch)
        fc::SlotSeg* segs_dev = nullptr;            // [segs.size()], and behind it
        fc::SlotRef* refs_dev = nullptr;            // [B]
        std::vector<fc::SlotRef> refs;              // the host side of the copy
        size_t floats(int enc_frames, int dec_frames) const {
            return fixed + (size_t)enc_cols * fc::seq_cache_pitch(enc_frames) + (size_t)dec_cols * fc::seq_cache_pitch(dec_frames);
        }
    } rec;
    Session() = default;
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    ~Session() {
        drop_graphs();
        if (rec.segs_dev) (void)hipFree(rec.segs_dev);
    }
};

// One streaming session (fc_stream_*): B utterances in lock-step.  The host side keeps only push counters.
struct fc_stream : Session {
    int enc_pushes = 0, dec_pushes = 0;
    int enc_frames = 0, dec_frames = 0;             // frames each side's transformer has taken since reset (the `pos` of its next push)
    bool enc_done = false;                          // the final push has been taken
    bool broken = false;                            // a push failed half-way: carries are a mix of old and new until the next reset
};

// One slot session (fc_slots_*): B = S rows that start, continue, end and idle independently in one push; the host keeps each slot's
// phase per side.
struct fc_slots : Session {
    enum Phase : char { Idle, Running, Ended, Poisoned };
    std::vector<char> enc_phase, dec_phase;         // [S]
    int enc_pushes = 0, dec_pushes = 0;             // the carries' ping-pong parity per side: idle rows copy theirs, so one number serves all
    std::vector<int32_t> push;                      // [3 S]: counts, flags, then the cache positions of the push being enqueued (the source of its one copy)
    // a session with a key / value cache (fc_seqslots_create): the frames each slot's utterance has cached per side, the `pos` of its next push
    std::vector<int32_t> enc_frames, dec_frames;    // [S]; empty without max_frames
};

namespace {

hipEvent_t prof_event(fc_engine* e) {
    if (e->events_used == e->event_pool.size()) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return nullptr;
        e->event_pool.push_back(ev);
    }
    return e->event_pool[e->events_used++];
}

// RAII: an event bracket from construction to scope exit, booked to the kernel class cls() names (called only when profiling)
struct ProfSpan {
    fc_engine* e; hipStream_t st; int idx = -1;
    template <typename Cls>
    ProfSpan(fc_engine* e_, hipStream_t st_, bool live, Cls&& cls, double flops, double bytes) : e(e_), st(st_) {
        if (!e->profiling || !live) return;
        fc_engine::Span s; s.cls = e->prof_class(cls()); s.a = prof_event(e); s.b = prof_event(e); s.flops = flops; s.bytes = bytes;
        if (!s.a || !s.b) return;
        (void)hipEventRecord(s.a, st);
        e->spans.push_back(s);
        idx = (int)e->spans.size() - 1;
    }
    ~ProfSpan() { if (idx >= 0) (void)hipEventRecord(e->spans[idx].b, st); }
};

// One pass of the layer drivers over the plan.  A dry pass (no workspace, no stream) sizes the workspace and counts the work; a live
// pass also enqueues.  Both run the same code, so the launch counts are the launch sequence itself.
struct Ctx {
    fc_engine* e = nullptr;
    int B = 0;
    hipStream_t st = nullptr;
    char* base = nullptr;
    size_t cap = 0, off = 256;       // the first buffer starts 256 bytes in: the grouped 3 x 3 conv reads one float in front of a row (freq_kernels.hip, FASTEDGE)
    bool dry = false;
    int err = 0;
    // where the walk of a ragged pass stands (run_encoder / run_decoder keep them): the side, and the columns of the layer's input per
    // encoder input sample / decoder frame (ConvVisit::rate); no_xq: the DMA-staged materialisation (MODE 5) is not used in a ragged pass
    bool dec_side = false, no_xq = false;
    int rate = 1;
    static constexpr size_t kTailSlack = 4096;
    int launches = 0, conv_launches = 0;
    double conv_flops = 0, conv_bytes = 0, lstm_flops = 0, rvq_flops = 0, attn_flops = 0;
    bool live() const { return !dry && !err; }
    void fail(const std::string& msg) {      // the first failure of the pass is the one reported
        if (!err) { err = 1; g_err = msg; }
    }
    template <typename T>
    T* alloc(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = dry ? nullptr : (T*)(base + off);
        off += n * sizeof(T);
        // every buffer ends at least kTailSlack bytes before the end of the workspace: kernels with unclamped row-end loads (the grouped
        // 3 x 3 / 8 x 2 convs, freq_kernels.hip FASTEDGE) and the DMA-staged conv (over-read of the last N tile) rely on it
        if (!dry && off + kTailSlack > cap) { fail("workspace too small (sizes from fc_engine_workspace_bytes include 4 KiB of tail slack)"); return nullptr; }
        return p;
    }
    // One kernel launch: counted in both passes, enqueued only in a live one.  enqueue() returns the launch's status; a failure is
    // reported as `what` of `layer`.
    template <typename Enqueue>
    void launch(const char* what, const char* layer, Enqueue&& enqueue) {
        ++launches;
        if (live()) check(enqueue(), what, layer);
    }
    // the same inside a profiler bracket that books `flops` and `bytes` to the kernel class cls() names
    template <typename Cls, typename Enqueue>
    void launch(const char* what, const char* layer, Cls&& cls, double flops, double bytes, Enqueue&& enqueue) {
        ++launches;
        if (!live()) return;
        ProfSpan sp(e, st, true, cls, flops, bytes);
        check(enqueue(), what, layer);
    }
    // a launch of a conv kernel (also counted in conv_launches)
    template <typename Cls, typename Enqueue>
    void conv_launch(const char* what, const char* layer, Cls&& cls, double flops, double bytes, Enqueue&& enqueue) {
        ++conv_launches;
        launch(what, layer, cls, flops, bytes, enqueue);
    }
    void check(hipError_t er, const char* what, const char* layer) {
        if (er != hipSuccess) fail(std::string(what) + " launch failed" + (*layer ? std::string(" (") + layer + ")" : "") + ": " + hipGetErrorString(er));
    }
};

Ctx make_ctx(fc_engine* e, int B, void* ws, size_t ws_bytes, void* stream) {
    Ctx cx;
    cx.e = e; cx.B = B; cx.st = (hipStream_t)stream; cx.base = (char*)ws; cx.cap = ws_bytes;
    return cx;
}

Ctx dry_ctx(fc_engine* e, int B) {
    Ctx cx = make_ctx(e, B, nullptr, 0, nullptr);
    cx.dry = true;
    return cx;
}

// a buffer position that stays null in a dry pass
template <typename T>
T* at(T* p, long long off) { return p ? p + off : nullptr; }

// ---- the time-domain SEANet's layer order, stated once (nn.Sequential order: seanet_encoder.py:109-160, seanet_decoder.py:111-164).
// The plan's contract, the weight packing, the streaming state layout and the forward walk (run_encoder / run_decoder) all follow it.
enum class Role { First, Shortcut, Block1, Block3, Resample, Last };
// a causal conv with k > 1 looks at columns to its left, which a streaming push must carry; the k = 1 convs of a block are pointwise
inline bool carries_context(Role r) { return r != Role::Shortcut && r != Role::Block3; }

struct ConvVisit {
    ConvLayer& L;
    bool dec;                     // decoder side
    Role role;
    int rate;                     // columns of L's input: one per `rate` encoder input samples / `rate` per decoder frame
    fc_engine::ResBlock* block;   // the residual block of a Shortcut / Block1 / Block3 layer, else null
};

// every conv of the 1-D nets in execution order.  The bottleneck sequence model sits in front of the encoder's Last and behind the
// decoder's First.
template <typename F>
void for_each_conv(fc_engine* e, F&& f) {
    auto blocks = [&](fc_engine::Stage& S, bool dec, int rate) {
        for (auto& R : S.res) {
            f(ConvVisit{R.shortcut, dec, Role::Shortcut, rate, &R});
            f(ConvVisit{R.block1, dec, Role::Block1, rate, &R});
            f(ConvVisit{R.block3, dec, Role::Block3, rate, &R});
        }
    };
    int div = 1;
    f(ConvVisit{e->enc_first, false, Role::First, div, nullptr});
    for (auto& S : e->enc_stages) {
        blocks(S, false, div);
        f(ConvVisit{S.resample, false, Role::Resample, div, nullptr});
        div *= S.resample.stride;
    }
    f(ConvVisit{e->enc_last, false, Role::Last, div, nullptr});
    int mul = 1;
    f(ConvVisit{e->dec_first, true, Role::First, mul, nullptr});
    for (auto& S : e->dec_stages) {
        f(ConvVisit{S.resample, true, Role::Resample, mul, nullptr});
        mul *= S.resample.stride;
        blocks(S, true, mul);
    }
    f(ConvVisit{e->dec_last, true, Role::Last, mul, nullptr});
}

// ---- plan construction (mirrors nn.Sequential indices: seanet_encoder.py:109-160, seanet_decoder.py:111-164)
void add_conv_expect(fc_engine* e, ConvLayer& L) {
    const std::string inner = L.transposed ? ".convtr" : ".conv";
    const int d0 = L.transposed ? L.cin : L.cout, d1 = L.transposed ? L.cout : L.cin;
    if (L.wnorm) {
        e->expected.push_back({L.prefix + inner + ".weight_g", {d0, 1, 1}});
        e->expected.push_back({L.prefix + inner + ".weight_v", {d0, d1, L.k}});
    } else {
        e->expected.push_back({L.prefix + inner + ".weight", {d0, d1, L.k}});
    }
    e->expected.push_back({L.prefix + inner + ".bias", {L.cout}});
    if (L.has_norm) {
        e->expected.push_back({L.prefix + ".norm.weight", {L.cout}});
        e->expected.push_back({L.prefix + ".norm.bias", {L.cout}});
    }
    e->by_prefix[L.prefix] = &L;
}

void choose_tiling(ConvLayer& L);

ConvLayer mk_conv(const std::string& prefix, int cin, int cout, int k, int stride, bool transposed = false,
                  bool dual = false, bool small_n = false, int dil = 1);
ConvLayer mk_conv_(const std::string& prefix, int cin, int cout, int k, int stride, bool transposed, bool dual, bool small_n, int dil);
ConvLayer mk_conv(const std::string& prefix, int cin, int cout, int k, int stride, bool transposed, bool dual, bool small_n, int dil) {
    ConvLayer L = mk_conv_(prefix, cin, cout, k, stride, transposed, dual, small_n, dil);
    if (getenv("FC_DUMP_PLAN"))     // tuning aid: the tiling every layer gets
        fprintf(stderr, "plan %-36s cin=%4d M=%4d k=%2d s=%d  tile %3dx%3d CC=%2d nchunk=%3d %s\n", L.prefix.c_str(), L.cin, L.M,
                L.gk, L.gstride, L.BM, L.BN, L.CC, L.nchunk, L.row ? "row" : "");
    return L;
}
ConvLayer mk_conv_(const std::string& prefix, int cin, int cout, int k, int stride, bool transposed, bool dual, bool small_n, int dil) {
    ConvLayer L;
    L.prefix = prefix; L.cin = cin; L.cout = cout; L.k = k; L.stride = stride; L.transposed = transposed; L.dil = dil;
    L.dual = dual; L.small_n = small_n;
    if (!transposed) { L.M = cout; L.gk = k; L.gstride = stride; }
    else { L.M = cout * stride; L.gk = 2; L.gstride = 1; }   // 2-tap GEMM over the r output phases
    choose_tiling(L);
    return L;
}

// ---- STFT-domain codec: SEANetEncoder2d / SEANetDecoder2d (seanet_encoder.py:252-363, seanet_decoder.py:244-360) ---------------
// Same Sequential indexing as the reference; every Conv2d is planned as a 1-D GEMM over kf * C channels (frequency-major layout).
// `groups` > 1 (conv_group_ratio > 0): the layer still runs as the dense GEMM over a block-diagonal weight built at finalize (the
// zero products add exactly nothing: same result as the grouped conv accumulated in the same order)
ConvLayer mk_conv2d(const std::string& prefix, int cin, int cout, int kf, int kt, int sf, int st, bool dual, int groups = 1) {
    ConvLayer L = mk_conv(prefix, kf * cin, cout, kt, st, false, dual, false, 1);
    L.kf = kf; L.sf = sf; L.c2d = cin; L.extra_left = true; L.groups = groups;
    return L;
}
inline int group_count(int n, int ratio) { return ratio > 0 ? n / 2 / ratio : 1; }

void add_conv2d_expect(fc_engine* e, ConvLayer& L) {
    const int cpg = L.c2d / (L.groups > 0 ? L.groups : 1);                         // groups < 1 is refused at create
    if (L.wnorm) {                                                                 // torch.nn.utils.weight_norm, dim 0 (conv.py:24-25)
        e->expected.push_back({L.prefix + ".conv.weight_g", {L.cout, 1, 1, 1}});
        e->expected.push_back({L.prefix + ".conv.weight_v", {L.cout, cpg, L.kf, L.k}});
    } else {
        e->expected.push_back({L.prefix + ".conv.weight", {L.cout, cpg, L.kf, L.k}});
    }
    e->expected.push_back({L.prefix + ".conv.bias", {L.cout}});
    if (L.has_norm) {
        e->expected.push_back({L.prefix + ".norm.weight", {L.cout}});
        e->expected.push_back({L.prefix + ".norm.bias", {L.cout}});
    }
    e->by_prefix[L.prefix] = &L;
}

// the weight a weight-normed 2-D layer computes in its forward pre-hook: v * (g / ||v||), the norm over every dim but 0 (`key` = prefix +
// ".conv" / ".convtr"; d0 = out channels of Conv2d, IN channels of ConvTranspose2d); the plain weight otherwise
std::vector<float> folded_weight_nd(fc_engine* e, const std::string& key, bool wnorm, size_t d0) {
    if (!wnorm) return e->host[key + ".weight"].data;
    const auto& V = e->host[key + ".weight_v"].data;
    const auto& G = e->host[key + ".weight_g"].data;
    const size_t inner_n = V.size() / d0;
    std::vector<float> folded(V.size());
    for (size_t r = 0; r < d0; ++r) {
        double ss = 0.0;
        for (size_t j = 0; j < inner_n; ++j) ss += (double)V[r * inner_n + j] * (double)V[r * inner_n + j];
        const float sc = G[r] / (float)sqrt(ss);
        for (size_t j = 0; j < inner_n; ++j) folded[r * inner_n + j] = V[r * inner_n + j] * sc;
    }
    return folded;
}

// CostumeQuantizer (costume_quantizer.py:7-55): the codebooks, and with codec_dim != input_size the two Linears around them
void add_quantizer_expect(fc_engine* e) {
    const fc_arch& a = e->arch;
    e->q_proj = a.codec_dim > 0 && a.codec_dim != a.dimension;
    if (e->q_proj) {
        e->q_in = mk_conv("quantizer.input_proj", a.dimension, a.codec_dim, 1, 1, false, false, true);
        e->q_out = mk_conv("quantizer.output_proj", a.codec_dim, a.dimension, 1, 1, false, false, true);
        e->q_in.has_norm = e->q_out.has_norm = false;
        e->expected.push_back({"quantizer.input_proj.weight", {a.codec_dim, a.dimension}});
        e->expected.push_back({"quantizer.input_proj.bias", {a.codec_dim}});
        e->expected.push_back({"quantizer.output_proj.weight", {a.dimension, a.codec_dim}});
        e->expected.push_back({"quantizer.output_proj.bias", {a.dimension}});
    }
    e->expected.push_back({"quantizer.rq.model.embed", {a.num_quantizers, a.codebook_size, e->cdim()}});
}

// TransformerEncoder's checkpoint contract, in state_dict order (EncoderLayer: self_attn, feed_forward, norm1, norm2; then after_norm)
void add_tf_expect(fc_engine* e, TfBlock& tb) {
    if (tb.C == 0) return;
    const fc_arch& a = e->arch;
    const int C = tb.C;
    tb.heads = a.seq_heads; tb.ff = a.seq_ff;
    tb.layers.resize(a.lstm_layers);
    for (int l = 0; l < a.lstm_layers; ++l) {
        const std::string p = tb.prefix + ".encoders." + std::to_string(l);
        TfLayer& L = tb.layers[l];
        L.qkv = mk_conv(p + ".self_attn.linear_qkv", C, 3 * C, 1, 1, false, false, true);
        L.out = mk_conv(p + ".self_attn.linear_out", C, C, 1, 1, false, false, true);
        L.ff1 = mk_conv(p + ".feed_forward.w_1", C, tb.ff, 1, 1, false, false, true);
        L.ff2 = mk_conv(p + ".feed_forward.w_2", tb.ff, C, 1, 1, false, false, true);
        for (ConvLayer* c : {&L.qkv, &L.out, &L.ff1, &L.ff2}) c->has_norm = false;
        for (const char* n : {"linear_q", "linear_k", "linear_v", "linear_out"}) {
            e->expected.push_back({p + ".self_attn." + n + ".weight", {C, C}});
            e->expected.push_back({p + ".self_attn." + n + ".bias", {C}});
        }
        e->expected.push_back({p + ".feed_forward.w_1.weight", {tb.ff, C}});
        e->expected.push_back({p + ".feed_forward.w_1.bias", {tb.ff}});
        e->expected.push_back({p + ".feed_forward.w_2.weight", {C, tb.ff}});
        e->expected.push_back({p + ".feed_forward.w_2.bias", {C}});
        for (const char* n : {"norm1", "norm2"}) {
            e->expected.push_back({p + "." + n + ".weight", {C}});
            e->expected.push_back({p + "." + n + ".bias", {C}});
        }
    }
    e->expected.push_back({tb.prefix + ".after_norm.weight", {C}});
    e->expected.push_back({tb.prefix + ".after_norm.bias", {C}});
    e->tf_by_prefix[tb.prefix] = &tb;
}

// SLSTM's checkpoint contract (torch.nn.LSTM names), and the input projection of every layer as a k = 1 GEMM
void add_lstm_expect(fc_engine* e, LstmBlock& lb) {
    if (lb.H == 0) return;
    lb.layers.resize(e->arch.lstm_layers);
    for (int l = 0; l < e->arch.lstm_layers; ++l) {
        const std::string sfx = "_l" + std::to_string(l);
        lb.layers[l].inproj = mk_conv(lb.prefix + ".inproj" + sfx, lb.H, 4 * lb.H, 1, 1, false, false, true);
        lb.layers[l].inproj.has_norm = false;
        e->expected.push_back({lb.prefix + ".weight_ih" + sfx, {4 * lb.H, lb.H}});
        e->expected.push_back({lb.prefix + ".weight_hh" + sfx, {4 * lb.H, lb.H}});
        e->expected.push_back({lb.prefix + ".bias_ih" + sfx, {4 * lb.H}});
        e->expected.push_back({lb.prefix + ".bias_hh" + sfx, {4 * lb.H}});
    }
    e->lstm_by_prefix[lb.prefix] = &lb;
}

void build_plan_2d(fc_engine* e) {
    const fc_arch& a = e->arch;
    const int nf = a.n_filters, nres = a.n_residual_layers;
    e->halo2 = std::max(std::max(a.kernel_size, a.last_kernel_size), a.residual_kernel_size) / 2;
    for (int s = 0; s < a.n_ratios; ++s) e->halo2 = std::max(e->halo2, (a.ratios_f[s] + 1) / 2);
    auto name = [](const char* side, int idx, const char* suffix) { return std::string(side) + ".model." + std::to_string(idx) + suffix; };
    auto add_res = [&](fc_engine::ResBlock& R, const char* side, int idx, int c, int j, int dil) {
        const int hid = c / a.compress, rk = a.residual_kernel_size;
        const int gr = side[0] == 'e' ? a.enc_conv_group_ratio : a.dec_conv_group_ratio;
        R.shortcut = mk_conv2d(name(side, idx, ".shortcut.conv"), c, c, 1, 1, 1, 1, j > 0, group_count(c, gr));
        R.block1 = mk_conv2d(name(side, idx, ".block.1.conv"), c, hid, rk, rk, 1, 1, j > 0, group_count(hid, gr));
        R.block1.dil = dil;                                   // dilation (1, dilation_base ** j): time axis only
        R.block3 = mk_conv2d(name(side, idx, ".block.3.conv"), hid, c, 1, 1, 1, 1, false, group_count(hid, gr));
    };
    // ---- encoder
    int idx = 0, mult = 1;
    e->enc2_first = mk_conv2d(name("encoder", idx, ".conv"), a.input_channels, nf, a.kernel_size, a.kernel_size, 1, 1, false);
    idx++;
    e->enc_stages.resize(a.n_ratios);
    for (int s = 0; s < a.n_ratios; ++s) {
        const int fr = a.ratios_f[a.n_ratios - 1 - s], tr = a.ratios[a.n_ratios - 1 - s];
        const int c = mult * nf;
        auto& S = e->enc_stages[s];
        S.res.resize(nres);
        for (int j = 0, dil = 1; j < nres; ++j, dil *= a.dilation_base) { add_res(S.res[j], "encoder", idx, c, j, dil); idx++; }
        idx++;                                                                    // ELU
        S.resample = mk_conv2d(name("encoder", idx, ".conv"), c, 2 * c, 2 * fr, 2 * tr, fr, tr, true, group_count(c, a.enc_conv_group_ratio));
        idx++;
        mult *= 2;
    }
    idx++;                                                                        // ReshapeModule (squeeze the frequency axis)
    const int cb = mult * nf;
    if (a.lstm_layers > 0 && a.seq_model == 1) { e->enc_tf.prefix = name("encoder", idx, ""); e->enc_tf.C = cb; idx++; }
    else if (a.lstm_layers > 0) { e->enc_lstm.prefix = name("encoder", idx, ".lstm"); e->enc_lstm.H = cb; idx++; }
    idx++;
    const bool skip_dual = a.lstm_layers > 0 && a.lstm_skip;
    e->enc_last = mk_conv(name("encoder", idx, ".conv"), cb, a.dimension, a.last_kernel_size, 1, false, skip_dual, true);
    // ---- decoder
    idx = 0;
    e->dec_first = mk_conv(name("decoder", idx, ".conv"), a.dimension, cb, a.kernel_size, 1, false, false, true);
    idx++;
    if (a.lstm_layers > 0 && a.seq_model == 1) { e->dec_tf.prefix = name("decoder", idx, ""); e->dec_tf.C = cb; idx++; }
    else if (a.lstm_layers > 0) { e->dec_lstm.prefix = name("decoder", idx, ".lstm"); e->dec_lstm.H = cb; idx++; }
    idx++;                                                                        // ReshapeModule (unsqueeze)
    e->dec_stages.resize(a.n_ratios);
    e->dec_up_phases.resize(a.n_ratios);
    for (int s = 0; s < a.n_ratios; ++s) {
        const int fr = a.ratios_f[s], tr = a.ratios[s];
        const int c = mult * nf, c2 = c / 2;
        auto& S = e->dec_stages[s];
        idx++;                                                                    // ELU
        // ConvTranspose2d(c -> c2, (2 fr, 2 tr), stride (fr, tr)): S.resample only carries the checkpoint contract; the launches
        // are one transposed 1-D GEMM (2 c channels = frequency rows fi - 1, fi) per output-frequency phase
        S.resample = ConvLayer();
        S.resample.prefix = name("decoder", idx, ".convtr");
        S.resample.transposed = true;
        S.resample.cin = c; S.resample.cout = c2; S.resample.c2d = c; S.resample.kf = 2 * fr; S.resample.sf = fr;
        S.resample.k = 2 * tr; S.resample.stride = tr; S.resample.groups = group_count(c, a.dec_tr_conv_group_ratio);
        for (int p = 0; p < fr; ++p)
            e->dec_up_phases[s].push_back(mk_conv(S.resample.prefix + ".phase" + std::to_string(p), 2 * c, c2, 2 * tr, tr, true, false, false));
        idx++;
        S.res.resize(nres);
        for (int j = 0, dil = 1; j < nres; ++j, dil *= a.dilation_base) { add_res(S.res[j], "decoder", idx, c2, j, dil); idx++; }
        mult /= 2;
    }
    idx++;
    e->dec2_last = mk_conv2d(name("decoder", idx, ".conv"), nf, a.input_channels, a.last_kernel_size, a.last_kernel_size, 1, 1, true);
    // ---- the STFT and its inverse as GEMMs over the hop-phase view of the signal (weights generated at finalize)
    const int F = a.n_fft / 2 + 1, taps = ceil_div_i(a.n_fft, a.stft_hop);
    e->stft = mk_conv("stft", a.stft_hop, 2 * F, taps, 1);
    e->stft.valid = true; e->stft.has_norm = false; e->stft.synthetic = true;
    {   // norm / causality of every layer of the nets (norm_type 0: GroupNorm(1, C) after each conv; 1: weight_norm, optionally causal in time)
        auto flag = [&](ConvLayer& L) { L.has_norm = a.norm_type == 0; L.wnorm = a.norm_type == 1; L.causal = a.causal != 0; };
        flag(e->enc2_first); flag(e->enc_last); flag(e->dec_first); flag(e->dec2_last);
        for (auto* stages : {&e->enc_stages, &e->dec_stages})
            for (auto& S : *stages) {
                flag(S.resample);
                for (auto& R : S.res) { flag(R.shortcut); flag(R.block1); flag(R.block3); }
            }
        for (auto& ph : e->dec_up_phases)
            for (auto& L : ph) flag(L);
    }
    e->istft = mk_conv("istft", 2 * F, a.stft_hop, taps, 1);
    e->istft.zpadL = taps - 1; e->istft.zpadR = taps - 1; e->istft.has_norm = false; e->istft.synthetic = true;
    // ---- checkpoint contract, in execution order
    add_conv2d_expect(e, e->enc2_first);
    for (auto& S : e->enc_stages) {
        for (auto& R : S.res) { add_conv2d_expect(e, R.block1); add_conv2d_expect(e, R.block3); add_conv2d_expect(e, R.shortcut); }
        add_conv2d_expect(e, S.resample);
    }
    add_lstm_expect(e, e->enc_lstm);
    add_tf_expect(e, e->enc_tf);
    add_conv_expect(e, e->enc_last);
    add_conv_expect(e, e->dec_first);
    add_lstm_expect(e, e->dec_lstm);
    add_tf_expect(e, e->dec_tf);
    for (auto& S : e->dec_stages) {
        const int opg_t = S.resample.cout / (S.resample.groups > 0 ? S.resample.groups : 1);
        if (S.resample.wnorm) {                                               // dim 0 of a ConvTranspose2d weight = its IN channels
            e->expected.push_back({S.resample.prefix + ".convtr.weight_g", {S.resample.c2d, 1, 1, 1}});
            e->expected.push_back({S.resample.prefix + ".convtr.weight_v", {S.resample.c2d, opg_t, S.resample.kf, S.resample.k}});
        } else {
            e->expected.push_back({S.resample.prefix + ".convtr.weight", {S.resample.c2d, opg_t, S.resample.kf, S.resample.k}});
        }
        e->expected.push_back({S.resample.prefix + ".convtr.bias", {S.resample.cout}});
        if (S.resample.has_norm) {
            e->expected.push_back({S.resample.prefix + ".norm.weight", {S.resample.cout}});
            e->expected.push_back({S.resample.prefix + ".norm.bias", {S.resample.cout}});
        }
        for (auto& R : S.res) { add_conv2d_expect(e, R.block1); add_conv2d_expect(e, R.block3); add_conv2d_expect(e, R.shortcut); }
    }
    add_conv2d_expect(e, e->dec2_last);
    add_quantizer_expect(e);
}

void build_plan(fc_engine* e) {
    if (e->arch.model_type == 1) { build_plan_2d(e); return; }
    const fc_arch& a = e->arch;
    const int nf = a.n_filters, nres = a.n_residual_layers;
    auto name = [](const char* side, int idx, const char* suffix) {
        return std::string(side) + ".model." + std::to_string(idx) + suffix;
    };
    // ---- encoder
    int idx = 0, mult = 1;
    e->enc_first = mk_conv(name("encoder", idx, ".conv"), e->audio_ch(), nf, a.kernel_size, 1);
    idx++;
    e->enc_stages.resize(a.n_ratios);
    for (int s = 0; s < a.n_ratios; ++s) {
        const int ratio = a.ratios[a.n_ratios - 1 - s];
        const int c = mult * nf, hid = c / a.compress;
        auto& S = e->enc_stages[s];
        S.res.resize(nres);
        for (int j = 0, dil = 1; j < nres; ++j, dil *= a.dilation_base) {      // dilations [dilation_base**j, 1] (seanet_encoder.py:127-133)
            auto& R = S.res[j];
            R.shortcut = mk_conv(name("encoder", idx, ".shortcut.conv"), c, c, 1, 1, false, j > 0);
            R.block1 = mk_conv(name("encoder", idx, ".block.1.conv"), c, hid, a.residual_kernel_size, 1, false, j > 0, false, dil);
            R.block3 = mk_conv(name("encoder", idx, ".block.3.conv"), hid, c, 1, 1);
            idx++;
        }
        idx++;                                                                    // ELU
        S.resample = mk_conv(name("encoder", idx, ".conv"), c, 2 * c, 2 * ratio, ratio, false, true, s == a.n_ratios - 1);
        idx++;
        mult *= 2;
    }
    const int cb = mult * nf;
    if (a.lstm_layers > 0 && a.seq_model == 1) {
        e->enc_tf.prefix = name("encoder", idx, "");
        e->enc_tf.C = cb;
        idx++;
    } else if (a.lstm_layers > 0) {
        e->enc_lstm.prefix = name("encoder", idx, ".lstm");
        e->enc_lstm.H = cb;
        idx++;
    }
    idx++;
    const bool skip_dual = a.lstm_layers > 0 && a.lstm_skip;
    e->enc_last = mk_conv(name("encoder", idx, ".conv"), cb, a.dimension, a.last_kernel_size, 1, false, skip_dual, true);
    // ---- decoder
    idx = 0;
    e->dec_first = mk_conv(name("decoder", idx, ".conv"), a.dimension, cb, a.kernel_size, 1, false, false, true);
    idx++;
    if (a.lstm_layers > 0 && a.seq_model == 1) {
        e->dec_tf.prefix = name("decoder", idx, "");
        e->dec_tf.C = cb;
        idx++;
    } else if (a.lstm_layers > 0) {
        e->dec_lstm.prefix = name("decoder", idx, ".lstm");
        e->dec_lstm.H = cb;
        idx++;
    }
    e->dec_stages.resize(a.n_ratios);
    mult = 1 << a.n_ratios;
    for (int s = 0; s < a.n_ratios; ++s) {
        const int ratio = a.ratios[s];
        const int c = mult * nf, c2 = c / 2, hid = c2 / a.compress;
        auto& S = e->dec_stages[s];
        idx++;
        S.resample = mk_conv(name("decoder", idx, ".convtr"), c, c2, 2 * ratio, ratio, true, s > 0 || skip_dual, s == 0);
        idx++;
        S.res.resize(nres);
        for (int j = 0, dil = 1; j < nres; ++j, dil *= a.dilation_base) {
            auto& R = S.res[j];
            R.shortcut = mk_conv(name("decoder", idx, ".shortcut.conv"), c2, c2, 1, 1, false, j > 0);
            R.block1 = mk_conv(name("decoder", idx, ".block.1.conv"), c2, hid, a.residual_kernel_size, 1, false, j > 0, false, dil);
            R.block3 = mk_conv(name("decoder", idx, ".block.3.conv"), hid, c2, 1, 1);
            idx++;
        }
        mult /= 2;
    }
    idx++;
    e->dec_last = mk_conv(name("decoder", idx, ".conv"), nf, e->audio_ch(), a.last_kernel_size, 1, false, true);

    // ---- per layer: the conv wrapper flavour of its SConv1d / SConvTranspose1d (conv.py:20-56) and its part of the checkpoint
    // contract, in execution order, the sequence models' tensors where they sit between the convs
    for_each_conv(e, [&](const ConvVisit& v) {
        v.L.has_norm = a.norm_type == 0;
        v.L.wnorm = a.norm_type == 1;
        v.L.causal = a.causal != 0;
        if (v.role == Role::Shortcut) {
            const std::string& sp = v.L.prefix;                          // "<side>.model.<i>.shortcut.conv"
            e->res_by_prefix[sp.substr(0, sp.size() - std::string(".shortcut.conv").size())] = v.block;
        }
        if (!v.dec && v.role == Role::Last) { add_lstm_expect(e, e->enc_lstm); add_tf_expect(e, e->enc_tf); }
        add_conv_expect(e, v.L);
        if (v.dec && v.role == Role::First) { add_lstm_expect(e, e->dec_lstm); add_tf_expect(e, e->dec_tf); }
    });
    add_quantizer_expect(e);
}

// ---- weight packing -------------------------------------------------------------------------------
void choose_tiling(ConvLayer& L) {  // NOLINT
    if (L.M > 64) {
        L.BM = 128; L.BN = 128;
        if (L.small_n && L.M <= 256) { L.BM = 32; L.BN = 128; }   // too few 128x128 tiles at the bottleneck rate
        // (256 x 128 tiles -- one 8-wave workgroup per CU, the slab staged once per 256 rows -- were measured in round 2: every layer
        // slower, 18.1 vs 16.9 ms per step.  Two workgroups per CU covering each other's barriers are worth more than the halved staging.)
    } else if (L.M > 32) { L.BM = 64; L.BN = 256; }
    else { L.BM = 32; L.BN = 256; }
    // channels per K-chunk: as many as fit (a) the register-staged slab, (b) K-chunk <= 64, (c) half of the LDS
    // (two workgroups per CU).  Layers with >= 3 M tiles get their input materialised (run_conv) and therefore
    // always run the PLAIN variant: no affine tables, and the 16-element staging variant has no register pressure.
    // large strides (> 4 on the 256-column tiles, > 8 two-source): the slab of even a 2-channel chunk exceeds the staging registers.
    // Narrower N tile first, then the materialised-input (plain, 18 slots) variant, else the layer is refused at create.
    {
        auto fits = [&](bool dual) { return fc::conv_slab_fits(L.gk, L.gstride, L.dil, 2, L.BN, L.BM, dual && ceil_div_i(L.M, L.BM) < 3); };
        if (!fits(L.dual) && L.BN == 256) {
            if (L.BM == 32) L.BN = 128;
            else { L.BM = 128; L.BN = 128; }
        }
        if (!fits(L.dual)) {
            if (fits(false)) L.force_plain = true;
            else L.unsupported = true;
        }
    }
    const bool plain = ceil_div_i(L.M, L.BM) >= 3 || L.force_plain;
    const bool dual_eff = L.dual && !plain;
    // LDS budget of one workgroup.  Layers at the bottleneck frame rate with M <= 1024 have at most one workgroup per CU at the
    // benchmark shape anyway (M/128 x 2 N tiles x 16 utterances <= 256): they take the whole CU's LDS, i.e. twice as deep K
    // chunks -> half as many per-item barriers / pipeline refills for the same MFMA work (FC_SMALLN_LDS=80 restores round 1)
    static const int smalln_lds = fc::ab_knob("FC_SMALLN_LDS", 160);
    const size_t lds_budget = (size_t)((L.small_n && L.M <= 1024) ? smalln_lds : 160 / fc::conv_wgs_per_cu(L.BM)) * 1024;
    int cin_p2 = 2;
    while (cin_p2 < L.cin) cin_p2 *= 2;
    int cc = 2;
    for (;;) {
        const int n = cc * 2;
        if (n > 32 || n > cin_p2 || n * L.gk > 64) break;
        if (!fc::conv_slab_fits(L.gk, L.gstride, L.dil, n, L.BN, L.BM, dual_eff)) break;
        if (fc::conv_lds_bytes_for(L.gk, L.gstride, L.dil, n, L.BM, L.BN, L.cin, plain ? 0 : (L.dual ? 2 : 1), 0) > lds_budget) break;
        cc = n;
    }
    // stride-1 layers: row staging (16-byte loads and LDS stores) lifts the register bound on the chunk; take it when
    // it allows at least the same chunk
    static const int row_env = fc::deploy_switch("FC_ROW", 1);
    L.row = false;
    if (row_env && L.gstride == 1) {
        int best = 0;
        for (int n = 4; n <= 64 && n <= L.cin; n *= 2) {
            if (!fc::conv_row_ok(L.gk, L.gstride, L.dil, n, L.BM, L.BN, L.cin, dual_eff)) continue;
            if (fc::conv_lds_bytes_for(L.gk, L.gstride, L.dil, n, L.BM, L.BN, L.cin, plain ? 0 : (L.dual ? 2 : 1), 1) > lds_budget) continue;
            best = n;
        }
        if (best > cc || (best == cc && !plain)) { L.row = true; cc = best; }   // equal chunk + no prologue: the general
                                                                                // path's two register sets win
    }
    L.CC = cc;
    L.nchunk = ceil_div_i(L.cin, cc);
    L.Mpad = ceil_div_i(L.M, L.BM) * L.BM;
}

template <typename T>
int upload(fc_engine* e, const std::vector<T>& h, T** out) {
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, h.size() * sizeof(T) + 16));
    HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    e->dev_allocs.push_back(d);
    *out = (T*)d;
    return 0;
}

// gemm weight accessor: w(m, ci, tap) and bias(m)
int pack_gemm(fc_engine* e, ConvLayer& L, const std::vector<float>& wg /*[M][cin][gk]*/, const std::vector<float>& bg) {
    const int mtiles = L.Mpad / L.BM;
    const int wbuf = fc::conv_wbuf_floats(L.gk, L.CC, L.BM);   // chunk image exactly as it sits in LDS
    std::vector<float> packed((size_t)mtiles * L.nchunk * wbuf, 0.f);
    for (int mt = 0; mt < mtiles; ++mt)
        for (int ch = 0; ch < L.nchunk; ++ch)
            for (int kk = 0; kk < L.gk; ++kk)
                for (int cl = 0; cl < L.CC; ++cl) {
                    const int ci = ch * L.CC + cl;
                    if (ci >= L.cin) continue;
                    float* img = &packed[(size_t)(mt * L.nchunk + ch) * wbuf];
                    for (int mm = 0; mm < L.BM; ++mm) {
                        const int m = mt * L.BM + mm;
                        if (m < L.M) img[fc::conv_pack_index(L.gk, L.CC, L.BM, kk, cl, mm)] = wg[((size_t)m * L.cin + ci) * L.gk + kk];
                    }
                }
    std::vector<float> bpad(L.Mpad, 0.f);
    for (int m = 0; m < L.M; ++m) bpad[m] = bg[m];
    if (upload(e, packed, &L.wt)) return 1;
    if (upload(e, bpad, &L.bias)) return 1;
    if (upload(e, fc::conv_koff_table(L.gk, L.gstride, L.dil, L.CC, L.BN, L.row ? 1 : 0), &L.koff)) return 1;
    return 0;
}

int pack_conv(fc_engine* e, ConvLayer& L) {
    const std::string inner = L.transposed ? ".convtr" : ".conv";
    std::vector<float> folded;
    if (L.wnorm) {
        // torch.nn.utils.weight_norm (conv.py:24-25): weight = v * (g / ||v||), the 2-norm taken over every dim but 0
        // (dim 0 = out channels of Conv1d, IN channels of ConvTranspose1d)
        const auto& V = e->host[L.prefix + inner + ".weight_v"].data;
        const auto& G = e->host[L.prefix + inner + ".weight_g"].data;
        const size_t d0 = L.transposed ? L.cin : L.cout, inner_n = V.size() / d0;
        folded.resize(V.size());
        for (size_t r = 0; r < d0; ++r) {
            double ss = 0.0;
            for (size_t j = 0; j < inner_n; ++j) ss += (double)V[r * inner_n + j] * (double)V[r * inner_n + j];
            const float nrm = (float)sqrt(ss);
            const float sc = G[r] / nrm;
            for (size_t j = 0; j < inner_n; ++j) folded[r * inner_n + j] = V[r * inner_n + j] * sc;
        }
    }
    const auto& W = L.wnorm ? folded : e->host[L.prefix + inner + ".weight"].data;
    const auto& Bv = e->host[L.prefix + inner + ".bias"].data;
    if (!L.transposed) {
        if (pack_gemm(e, L, W, Bv)) return 1;
        if (L.cout == 1 && L.stride == 1) {
            if (upload(e, W, &L.w_plain)) return 1;       // [1][cin][k]
            L.bias0 = Bv[0];
        }
    } else {
        // ConvTranspose1d(k = 2r, stride = r) as a 2-tap GEMM over phases: row m = co*r + p,
        // tap 0 multiplies x[i-1] with w[ci][co][p + r], tap 1 multiplies x[i] with w[ci][co][p].
        const int r = L.stride;
        if (L.k != 2 * r) return fail("ConvTranspose1d with kernel != 2*stride is not supported: " + L.prefix);
        std::vector<float> wg((size_t)L.M * L.cin * 2), bg(L.M);
        for (int co = 0; co < L.cout; ++co)
            for (int p = 0; p < r; ++p) {
                const int m = co * r + p;
                bg[m] = Bv[co];
                for (int ci = 0; ci < L.cin; ++ci) {
                    wg[((size_t)m * L.cin + ci) * 2 + 0] = W[((size_t)ci * L.cout + co) * L.k + p + r];
                    wg[((size_t)m * L.cin + ci) * 2 + 1] = W[((size_t)ci * L.cout + co) * L.k + p];
                }
            }
        if (pack_gemm(e, L, wg, bg)) return 1;
    }
    if (L.has_norm) {
        if (upload(e, e->host[L.prefix + ".norm.weight"].data, &L.gamma)) return 1;
        if (upload(e, e->host[L.prefix + ".norm.bias"].data, &L.beta)) return 1;
    }
    return 0;
}

// folded (weight-norm applied) Conv1d weight [cout][cin][k] of a layer, as pack_conv computes it
std::vector<float> folded_conv_weight(fc_engine* e, const ConvLayer& L) {
    const std::string inner = L.transposed ? ".convtr" : ".conv";
    if (!L.wnorm) return e->host[L.prefix + inner + ".weight"].data;
    const auto& V = e->host[L.prefix + inner + ".weight_v"].data;
    const auto& G = e->host[L.prefix + inner + ".weight_g"].data;
    const size_t d0 = L.transposed ? L.cin : L.cout, inner_n = V.size() / d0;
    std::vector<float> folded(V.size());
    for (size_t r = 0; r < d0; ++r) {
        double ss = 0.0;
        for (size_t j = 0; j < inner_n; ++j) ss += (double)V[r * inner_n + j] * (double)V[r * inner_n + j];
        const float sc = G[r] / (float)sqrt(ss);
        for (size_t j = 0; j < inner_n; ++j) folded[r * inner_n + j] = V[r * inner_n + j] * sc;
    }
    return folded;
}

// Thin residual blocks (C = 32 / 64): shortcut + block.1 run as ONE launch (kernels.hip 1c).  Weight images exactly as they sit
// in LDS: wsc[c][m] = W_sc[m][c][0];  wb1[kk*C + c][h] = W_b1[h][c][kk].
int pack_reshead(fc_engine* e, fc_engine::ResBlock& R) {
    static const int enable = fc::ab_knob("FC_RESHEAD", 1);
    const int C = R.shortcut.cin, hid = R.block1.cout, K = R.block1.k;
    R.fused_head = enable && R.shortcut.cout == C && R.block1.cin == C && fc::reshead_ok(C, hid, R.shortcut.k, K, R.block1.dil, R.block1.stride) &&
                   R.shortcut.has_norm == R.block1.has_norm;
    if (!R.fused_head) return 0;
    const std::vector<float> Wsc = folded_conv_weight(e, R.shortcut), Wb1 = folded_conv_weight(e, R.block1);
    std::vector<float> a((size_t)C * C), b((size_t)K * C * hid);
    for (int m = 0; m < C; ++m)
        for (int c = 0; c < C; ++c) a[(size_t)c * C + m] = Wsc[(size_t)m * C + c];
    for (int h = 0; h < hid; ++h)
        for (int c = 0; c < C; ++c)
            for (int kk = 0; kk < K; ++kk) b[((size_t)kk * C + c) * hid + h] = Wb1[((size_t)h * C + c) * K + kk];
    if (upload(e, a, &R.wsc) || upload(e, b, &R.wb1)) return 1;
    if (upload(e, e->host[R.shortcut.prefix + ".conv.bias"].data, &R.bsc)) return 1;
    if (upload(e, e->host[R.block1.prefix + ".conv.bias"].data, &R.bb1)) return 1;
    return 0;
}


// ---- STFT-domain codec: weight re-layout ---------------------------------------------------------------------------------------
// Conv2d weight [cout][C][kf][kt] -> GEMM weight [cout][a * C + ci][kt] (frequency-major layout: rows fo*sf + a are consecutive
// [C][T] blocks, so tap a of channel ci is GEMM channel a * C + ci)
int pack_conv2d(fc_engine* e, ConvLayer& L) {
    const std::vector<float> W = folded_weight_nd(e, L.prefix + ".conv", L.wnorm, (size_t)L.cout);
    const auto& Bv = e->host[L.prefix + ".conv.bias"].data;
    const int C = L.c2d, kf = L.kf, kt = L.k;
    const int cpg = C / L.groups, opg = L.cout / L.groups;        // grouped: weight [cout][C / groups][kf][kt], block-diagonal when dense
    std::vector<float> wg((size_t)L.cout * kf * C * kt, 0.f);
    for (int m = 0; m < L.cout; ++m)
        for (int cl = 0; cl < cpg; ++cl) {
            const int ci = (m / opg) * cpg + cl;
            for (int a = 0; a < kf; ++a)
                for (int b = 0; b < kt; ++b)
                    wg[((size_t)m * (kf * C) + (size_t)a * C + ci) * kt + b] = W[(((size_t)m * cpg + cl) * kf + a) * kt + b];
        }
    if (pack_gemm(e, L, wg, Bv)) return 1;
    // FC_GCONV=0: grouped layers stay on the block-diagonal dense GEMM (A/B aid)
    static const int gconv_env = fc::ab_knob("FC_GCONV", 1);
    if (gconv_env && L.groups > 1 && L.dil == 1 && fc::gconv2d_ok(cpg, opg, kf, kt, L.stride) && upload(e, W, &L.w_group)) return 1;
    if (L.cout <= 4 && L.stride == 1 && L.sf == 1 && (L.k == 3 || L.k == 5 || L.k == 7) && upload(e, wg, &L.w_plain)) return 1;      // [cout][kf * C][kt]: FMA kernel, no MFMA tile
    if (L.has_norm) {
        if (upload(e, e->host[L.prefix + ".norm.weight"].data, &L.gamma)) return 1;
        if (upload(e, e->host[L.prefix + ".norm.bias"].data, &L.beta)) return 1;
    }
    return 0;
}

// ConvTranspose2d weight [C][cout][2 sf][2 st].  Output frequency row fo = q * sf + p receives input rows fi = q (tap a = p) and
// fi = q - 1 (tap a = p + sf).  Per phase p: a ConvTranspose1d over 2 C channels (first C: row q - 1, then row q -- their order
// in the zero-haloed input buffer) with weight W1d[r * C + ci][co][bt] = W[ci][co][p + (1 - r) * sf][bt], packed like every other
// transposed layer (2-tap GEMM over the time phases).
int pack_convtr2d(fc_engine* e, const ConvLayer& S, std::vector<ConvLayer>& phases) {
    const std::vector<float> W = folded_weight_nd(e, S.prefix + ".convtr", S.wnorm, (size_t)S.c2d);
    const auto& Bv = e->host[S.prefix + ".convtr.bias"].data;
    const int C = S.c2d, cout = S.cout, kf = S.kf, kt = S.k, sf = S.sf, r = S.stride;
    const int cpg = C / S.groups, opg = cout / S.groups;          // grouped: weight [C][cout / groups][kf][kt]
    for (int p = 0; p < sf; ++p) {
        ConvLayer& L = phases[p];
        std::vector<float> wg((size_t)L.M * L.cin * 2, 0.f), bg(L.M);
        for (int co = 0; co < cout; ++co)
            for (int ph = 0; ph < r; ++ph) {
                const int m = co * r + ph;
                bg[m] = Bv[co];
                for (int rr = 0; rr < 2; ++rr)
                    for (int ci = (co / opg) * cpg; ci < (co / opg + 1) * cpg; ++ci) {
                        const int a = p + (1 - rr) * sf;
                        const float* w = &W[(((size_t)ci * opg + co % opg) * kf + a) * kt];
                        const size_t c1 = (size_t)rr * C + ci;
                        wg[((size_t)m * L.cin + c1) * 2 + 0] = w[ph + r];      // tap 0 multiplies x[i-1]
                        wg[((size_t)m * L.cin + c1) * 2 + 1] = w[ph];          // tap 1 multiplies x[i]
                    }
            }
        if (pack_gemm(e, L, wg, bg)) return 1;
    }
    ConvLayer& L0 = phases[0];
    static const int gconv_env = fc::ab_knob("FC_GCONV", 1);
    if (gconv_env && S.groups > 1 && fc::gconvtr2d_ok(cpg, opg, r)) {          // direct kernel: torch-layout weights + plain bias
        if (upload(e, W, &L0.w_group) || upload(e, Bv, &L0.w_plain)) return 1;
    }
    if (S.has_norm) {
        if (upload(e, e->host[S.prefix + ".norm.weight"].data, &L0.gamma)) return 1;
        if (upload(e, e->host[S.prefix + ".norm.bias"].data, &L0.beta)) return 1;
    }
    return 0;
}

// torch.stft / torch.istft (center, periodic Hann window of n_fft, onesided, not normalised) as conv weights over the hop-phase view
// xp[j][m] = xpad[m * hop + j]:  X[f][t] = sum_{a, j} w[n] e^{-2 pi i f n / N} xp[j][t + a],  n = a * hop + j  (zero weight for n >= N);
// ypoly[j][m] = sum_{a, c} Wi[j][c][a] S[c][m - a]  (overlap-add of the windowed inverse DFTs), as a correlation over S zero-padded by
// taps - 1 frames on both sides: tap a' = taps - 1 - a.
int pack_dft(fc_engine* e) {
    const int N = e->arch.n_fft, hop = e->arch.stft_hop, F = N / 2 + 1, taps = ceil_div_i(N, hop);
    std::vector<double> win(N);
    for (int n = 0; n < N; ++n) win[n] = 0.5 - 0.5 * cos(2.0 * M_PI * n / N);          // torch.hann_window(N) (periodic)
    // twiddles with EXACT zeros at the quarter periods: the DC and Nyquist rows then have an exactly zero imaginary part, like an FFT's
    auto tw_cos = [&](long long k) { k %= N; return (k % (N / 2)) == N / 4 ? 0.0 : cos(2.0 * M_PI * (double)k / N); };
    auto tw_sin = [&](long long k) { k %= N; return (k % (N / 2)) == 0 ? 0.0 : sin(2.0 * M_PI * (double)k / N); };
    {
        ConvLayer& L = e->stft;
        std::vector<float> wg((size_t)2 * F * hop * taps, 0.f), bg(2 * F, 0.f);
        for (int f = 0; f < F; ++f)
            for (int j = 0; j < hop; ++j)
                for (int a = 0; a < taps; ++a) {
                    const int n = a * hop + j;
                    if (n >= N) continue;
                    const long long k = (long long)f * n;
                    wg[((size_t)f * hop + j) * taps + a] = (float)(win[n] * tw_cos(k));
                    wg[((size_t)(F + f) * hop + j) * taps + a] = tw_sin(k) == 0.0 ? 0.f : (float)(-win[n] * tw_sin(k));
                }
        if (pack_gemm(e, L, wg, bg)) return 1;
    }
    {
        ConvLayer& L = e->istft;
        std::vector<float> wg((size_t)hop * 2 * F * taps, 0.f), bg(hop, 0.f);
        for (int j = 0; j < hop; ++j)
            for (int f = 0; f < F; ++f)
                for (int a = 0; a < taps; ++a) {
                    const int n = a * hop + j;
                    if (n >= N) continue;
                    const double cf = (f == 0 || f == N / 2) ? 1.0 : 2.0;
                    const long long k = (long long)f * n;
                    const int ap = taps - 1 - a;
                    wg[((size_t)j * 2 * F + f) * taps + ap] = (float)(win[n] * cf * tw_cos(k) / N);
                    wg[((size_t)j * 2 * F + F + f) * taps + ap] = tw_sin(k) == 0.0 ? 0.f : (float)(-win[n] * cf * tw_sin(k) / N);
                }
        if (pack_gemm(e, L, wg, bg)) return 1;
    }
    std::vector<float> w2(N);
    for (int n = 0; n < N; ++n) w2[n] = (float)((float)win[n] * (float)win[n]);
    if (upload(e, w2, &e->win2)) return 1;
    return 0;
}

int pack_lstm(fc_engine* e, LstmBlock& lb) {
    const int H = lb.H;
    if (H == 0) return 0;
    if (H % 16 != 0) return fail("LSTM width must be a multiple of 16");
    for (int l = 0; l < (int)lb.layers.size(); ++l) {
        const std::string sfx = "_l" + std::to_string(l);
        const auto& Wih = e->host[lb.prefix + ".weight_ih" + sfx].data;
        const auto& Whh = e->host[lb.prefix + ".weight_hh" + sfx].data;
        const auto& bih = e->host[lb.prefix + ".bias_ih" + sfx].data;
        const auto& bhh = e->host[lb.prefix + ".bias_hh" + sfx].data;
        // permuted row m' = blk*16 + u*4 + gate  <->  original row gate*H + blk*4 + u   (gate order i,f,g,o)
        std::vector<float> wih_p((size_t)4 * H * H), whh_p((size_t)4 * H * H), b_p(4 * H);
        for (int mp = 0; mp < 4 * H; ++mp) {
            const int blk = mp / 16, u = (mp % 16) / 4, gate = mp % 4;
            const int orig = gate * H + blk * 4 + u;
            memcpy(&wih_p[(size_t)mp * H], &Wih[(size_t)orig * H], H * sizeof(float));
            memcpy(&whh_p[(size_t)mp * H], &Whh[(size_t)orig * H], H * sizeof(float));
            b_p[mp] = bih[orig] + bhh[orig];
        }
        LstmLayer& L = lb.layers[l];
        if (pack_gemm(e, L.inproj, wih_p, b_p)) return 1;
        if (upload(e, whh_p, &L.whh)) return 1;
        if (l >= 1) {
            std::vector<float> cat((size_t)4 * H * 2 * H);
            for (int mp = 0; mp < 4 * H; ++mp) {
                memcpy(&cat[(size_t)mp * 2 * H], &wih_p[(size_t)mp * H], H * sizeof(float));
                memcpy(&cat[(size_t)mp * 2 * H + H], &whh_p[(size_t)mp * H], H * sizeof(float));
            }
            if (upload(e, cat, &L.wcat)) return 1;
            if (upload(e, b_p, &L.bperm)) return 1;
        }
    }
    return 0;
}

int pack_tf(fc_engine* e, TfBlock& tb) {
    if (tb.C == 0) return 0;
    const int C = tb.C;
    auto H = [&](const std::string& k) -> const std::vector<float>& { return e->host[k].data; };
    for (int l = 0; l < (int)tb.layers.size(); ++l) {
        const std::string p = tb.prefix + ".encoders." + std::to_string(l);
        TfLayer& L = tb.layers[l];
        std::vector<float> W((size_t)3 * C * C), Bv((size_t)3 * C);      // Linear weight [out][in] = the k = 1 GEMM's [M][cin][1]
        int part = 0;
        for (const char* n : {"linear_q", "linear_k", "linear_v"}) {
            const auto& w = H(p + ".self_attn." + n + ".weight");
            const auto& b = H(p + ".self_attn." + n + ".bias");
            std::copy(w.begin(), w.end(), W.begin() + (size_t)part * C * C);
            std::copy(b.begin(), b.end(), Bv.begin() + (size_t)part * C);
            ++part;
        }
        if (pack_gemm(e, L.qkv, W, Bv)) return 1;
        if (pack_gemm(e, L.out, H(p + ".self_attn.linear_out.weight"), H(p + ".self_attn.linear_out.bias"))) return 1;
        if (pack_gemm(e, L.ff1, H(p + ".feed_forward.w_1.weight"), H(p + ".feed_forward.w_1.bias"))) return 1;
        if (pack_gemm(e, L.ff2, H(p + ".feed_forward.w_2.weight"), H(p + ".feed_forward.w_2.bias"))) return 1;
        if (upload(e, H(p + ".norm1.weight"), &L.n1g) || upload(e, H(p + ".norm1.bias"), &L.n1b)) return 1;
        if (upload(e, H(p + ".norm2.weight"), &L.n2g) || upload(e, H(p + ".norm2.bias"), &L.n2b)) return 1;
    }
    if (upload(e, H(tb.prefix + ".after_norm.weight"), &tb.ag) || upload(e, H(tb.prefix + ".after_norm.bias"), &tb.ab)) return 1;
    return 0;
}

// ---- execution ------------------------------------------------------------------------------------
struct ConvGeom { int Tout, padL, padR, count_T; };

// SConv1d.forward padding arithmetic (conv.py:243-258, get_extra_padding_for_conv1d :57-64)
// (In a length-aware pass every ROW has its own T here; the per-layer row-length rule -- ceil at every stride -- and the
// extra-padding arithmetic, which this function uses too, are stated once in ragged_kernels.h: RagLen / ragged_cols / ragged_extra.)
ConvGeom conv_geom(const ConvLayer& L, int T) {
    ConvGeom g;
    if (L.valid) { g.padL = 0; g.padR = 0; g.Tout = T - L.k + 1; g.count_T = g.Tout; return g; }
    if (L.zpadL >= 0) { g.padL = L.zpadL; g.padR = L.zpadR; g.Tout = T + g.padL + g.padR - L.k + 1; g.count_T = g.Tout; return g; }
    if (!L.transposed) {
        const int pt = (L.k - 1) * L.dil - (L.stride - 1);      // padding_total (conv.py:247)
        const int extra = fc::ragged_extra(T, L.k, pt, L.stride);   // get_extra_padding_for_conv1d: stated once, for a batch and for a row
        if (L.causal) { g.padL = pt; g.padR = extra; }          // all fixed padding on the left (conv.py:249-251)
        else if (L.extra_left) { g.padR = pt / 2; g.padL = pt - pt / 2 + extra; }   // SConv2d, time axis (conv.py:376-377)
        else { g.padR = pt / 2 + extra; g.padL = pt - pt / 2; }
        // what nn.Conv1d then produces on the padded input (the reference's frame formula above ignores dilation; with
        // dilation 1 this equals nfr + 1)
        g.Tout = (T + g.padL + g.padR - ((L.k - 1) * L.dil + 1)) / L.stride + 1;
        g.count_T = g.Tout;
    } else {
        g.padL = 1; g.padR = 1;
        g.Tout = T * L.stride;           // trimmed length
        g.count_T = (T + 1) * L.stride;  // GroupNorm sees the untrimmed output (conv.py:287-303)
    }
    return g;
}

static bool out_override_blocks_xq(const ConvLayer& L) { return L.kf != 1 || L.valid || L.cout <= 4; }   // 2-D / STFT GEMMs / few-output FMA layers

// FreqCodec: the direct kernels and the materialisation passes write the reflected / zero halo rows of their outputs themselves (round 4;
// FC_HALO_FUSE=0: a halo_rows launch behind every producer, as before -- A / B aid)
static bool halo_fuse_on() {
    static const int v = fc::ab_knob("FC_HALO_FUSE", 1);
    return v != 0;
}

struct Act2 {              // raw [B][F + 2*halo][C][T] + pending GroupNorm affine [B][C] (null = final)
    float* buf = nullptr;
    float* aff = nullptr;
    int C = 0, F = 0, T = 0, halo = 0;
    bool normed = false;
};

// the fields of a conv launch that come from the layer's plan and its time-axis geometry (1-D convs, 2-D convs, transposed phases)
fc::ConvLaunch conv_launch_of(const ConvLayer& L, int B, int Tin, const ConvGeom& g) {
    fc::ConvLaunch c;
    c.wt = L.wt; c.bias = L.bias; c.koff = L.koff; c.w_plain = L.w_plain; c.bias_host0 = L.bias0;
    c.B = B; c.Cin = L.cin; c.Tin = Tin; c.M = L.M;
    c.k = L.gk; c.stride = L.gstride; c.dil = L.dil; c.padL = g.padL; c.padR = g.padR;
    c.BM = L.BM; c.BN = L.BN; c.CC = L.CC; c.nchunk = L.nchunk; c.row = L.row ? 1 : 0;
    return c;
}

// profiler class of a conv launch: the conv_mfma_kernel instantiation launch_conv picks, or its few-output FMA kernel
std::string conv_class(const fc::ConvLaunch& c) {
    int mode = 0, nu = 0, row = 0;
    fc::conv_variant(c, &mode, &nu, &row);
    char nm[80];
    snprintf(nm, sizeof(nm), "conv_mfma_kernel<%d, %d, %d, %d, %d, %d, %s, %s>", c.BM, c.BN, c.BM >= 128 ? 2 : 1, c.BM >= 128 ? 2 : 4, mode, nu,
             (row & 1) ? "true" : "false", (row & 2) ? "true" : "false");
    if (fc::conv_cout1_ok(c)) fc::conv_fewout_name(c, nm, sizeof(nm));
    return nm;
}

// the launches behind a conv layer's kernel: GroupNorm statistics -> affine (GroupNorm nets), then the frequency halo rows of a 2-D
// output that the kernel did not write itself (halo_of)
void conv_finish(fc_engine* e, Ctx& cx, const ConvLayer& L, const double* partials, int nblk, double count, float* aff, const Act2* halo_of = nullptr) {
    if (L.has_norm)
        cx.launch("gn_finalize", L.prefix.c_str(),
                  [&] { return fc::launch_gn_finalize(partials, nblk, count, L.gamma, L.beta, L.cout, e->arch.gn_eps, cx.B, aff, cx.st); });
    if (halo_of)
        cx.launch("halo rows", L.prefix.c_str(),
                  [&] { return fc::launch_halo_rows(halo_of->buf, cx.B, halo_of->F, halo_of->halo, halo_of->C, halo_of->T, 0, cx.st); });
}

Act run_conv(fc_engine* e, Ctx& cx, const ConvLayer& L, fc::Src s0, fc::Src s1, int elu, int Tin,
             float* out_override = nullptr, long long sB = 0, long long sM = 0, long long sT = 0) {
    const ConvGeom g = conv_geom(L, Tin);
    // Layers with several M tiles would re-apply the fused prologue (GroupNorm affine, residual add, ELU) once per
    // M tile; for those (deep, short tensors) it is cheaper to materialise the activated input once and stream it.
    const bool has_prologue = (s0.used & 2) || s1.used || elu;
    int xq_Tp = 0;
    if ((L.Mpad / L.BM >= 3 || L.force_plain) && has_prologue) {
        // the conv kernel's quad layout stages such an input by DMA when it is materialised with 4 channels interleaved and its padding in
        // place (kernels.hip combine_xq_kernel / conv_kernel.h MODE 5); else the plain [B][C][T] tensor and the register-staged PLAIN form
        const bool xq = !cx.no_xq && !s0.div && !out_override_blocks_xq(L) && fc::conv_xq_ok(L.cin, L.CC, L.gk, L.gstride, L.dil, L.BM, L.BN, L.row ? 1 : 0);
        const int padL_x = L.transposed ? 1 : g.padL, padR_x = L.transposed ? 1 : g.padR;
        const int Tp = padL_x + Tin + padR_x;
        float* tmp = xq ? cx.alloc<float>(fc::conv_xq_floats(cx.B, L.cin, Tp, L.BN, L.gstride, L.gk, L.dil))
                        : cx.alloc<float>((size_t)cx.B * L.cin * Tin);
        cx.launch("combine", L.prefix.c_str(), [&] {
            return xq ? fc::launch_combine_xq(s0, s1, elu, e->arch.elu_alpha, cx.B, L.cin, Tin, padL_x, padR_x, (L.transposed || L.zpadL >= 0) ? 1 : 0, tmp, cx.st)
                      : fc::launch_combine(s0, s1, elu, e->arch.elu_alpha, nullptr, cx.B, L.cin, Tin, Tin, tmp, (long long)L.cin * Tin, Tin, 1, cx.st);
        });
        s0 = fc::Src(); s0.ptr = tmp; s0.used = 1;
        s1 = fc::Src();
        elu = 0;
        if (xq) xq_Tp = Tp;
    }
    fc::ConvLaunch c = conv_launch_of(L, cx.B, Tin, g);
    c.s0 = s0; c.s1 = s1; c.elu = elu; c.alpha = e->arch.elu_alpha;
    c.xq_Tp = xq_Tp;
    Act out;
    out.C = L.cout; out.T = g.Tout;
    if (L.transposed) {
        c.Tout = Tin + 1; c.pad_zero = 1;
        // unpad1d: non-causal trims left = r - r/2, right = r/2; causal (trim_right_ratio 1) trims everything on the right
        c.up_r = L.stride; c.trimL = L.causal ? 0 : L.stride - L.stride / 2; c.Tfinal = g.Tout;
    } else {
        c.Tout = g.Tout;
        if (L.zpadL >= 0) c.pad_zero = 1;
    }
    if (out_override) {
        out.raw = out_override;
        c.out_sB = sB; c.out_sM = sM; c.out_sT = sT;
    } else {
        out.raw = cx.alloc<float>((size_t)cx.B * L.cout * g.Tout);
        c.out_sB = (long long)L.cout * g.Tout; c.out_sM = g.Tout; c.out_sT = 1;
    }
    c.out = out.raw;
    const int nblk = fc::conv_nblk(c);
    if (L.has_norm) {
        c.partials = cx.alloc<double>((size_t)cx.B * nblk * 2);
        out.aff = cx.alloc<float>((size_t)cx.B * L.cout * 2);
        out.normed = true;
    }
    // accounting (algorithmic: real channel counts, every operand touched once)
    const double fl = 2.0 * cx.B * (double)L.M * L.cin * L.gk * c.Tout;
    const double by = 4.0 * cx.B * ((double)L.cin * Tin * (s1.used ? 2 : 1) + (double)L.cout * g.Tout);
    cx.conv_flops += fl; cx.conv_bytes += by;
    // an invalid-value failure: tiling / LDS limits, or an utterance longer than 2^32 / (4 * channels per chunk) samples
    cx.conv_launch("conv", L.prefix.c_str(), [&] { return conv_class(c); }, fl, by, [&] { return fc::launch_conv(c, cx.st); });
    conv_finish(e, cx, L, c.partials, nblk, (double)L.cout * g.count_T, out.aff);
    return out;
}

// Src.used: bit 0 = present, bit 1 = carries an affine / divisor (planning flags, valid when pointers are null)
inline fc::Src src_of(const Act& a) { fc::Src s; s.ptr = a.raw; s.aff = a.aff; s.used = a.normed ? 3 : 1; s.ld = a.ld; return s; }

// SLSTM.forward (lstm.py:22-28) without the skip; returns plain y [B][H][T].
// Layer wavefront: one launch per "diagonal" s advances every layer l by its timestep s - l.
// `carried` (a streaming push; null offline): the per-step kernel's (h, c) buffers inside the session state, which continue the recurrence
// of the earlier pushes instead of starting from a cleared workspace buffer.  h_l(t) sits at parity t & 1 and step 0 reads parity 1, so
// after an odd number of steps the last hidden state is copied to where the next push looks for it.
// `steps` (a push of a slot session, with `carried`): row b takes ragged_cols(steps) of the T steps; the masked steps keep every row's
// hidden state at the common parity (lstm_kernels.hip lstm_wave_kernel, MASKED), so the copy after an odd T serves all rows.
Act run_lstm(fc_engine* e, Ctx& cx, const LstmBlock& lb, const Act& in, int T, float* carried = nullptr, const fc::RagLen* steps = nullptr) {
    const int H = lb.H, B = cx.B, L = (int)lb.layers.size();
    float* xproj = cx.alloc<float>((size_t)T * B * 4 * H);
    run_conv(e, cx, lb.layers[0].inproj, src_of(in), fc::Src(), 0, T, xproj, (long long)4 * H, 1, (long long)B * 4 * H);
    static const int persist_env = fc::deploy_switch("FC_LSTM_PERSIST", 1);
    bool persist = false;
    if (!carried && persist_env && e->lstm_persist_ok) {      // the persistent kernel keeps its state to itself: offline only
        const int key = B * 4096 + H;            // the occupancy query is cached per (B, H)
        if (e->persist_checked_B != key) { e->persist_checked_val = fc::lstm_persist_supported(B, H, L, e->device); e->persist_checked_B = key; }
        persist = e->persist_checked_val;
    }
    // persistent kernel: barrier words + hidden-state history; per-step launches: h [L][2][B][H], c [L][B][H]
    const size_t BH = (size_t)B * H;
    float* state = carried ? carried : cx.alloc<float>(persist ? fc::lstm_persist_state_floats(B, H, T) : 3 * L * BH);
    Act y;
    y.C = H; y.T = T;
    y.raw = cx.alloc<float>((size_t)B * H * T);
    const double fl = 2.0 * B * (double)T * 4 * H * H * (2 * L - 1);
    cx.lstm_flops += fl;
    // algorithmic bytes per SURVEY.md 8d: the recurrent weights read ONCE (they stay resident in registers) + the x-projection in + y out;
    // the per-step launches re-stream the weights, which is traffic, not algorithm
    const double by = 4.0 * (4.0 * H * H * (2 * L - 1) + (double)T * B * 4.0 * H + (double)B * H * T);
    const float* w[FC_LSTM_MAX_LAYERS] = {nullptr};
    const float* bias[FC_LSTM_MAX_LAYERS] = {nullptr};
    for (int l = 0; l < L; ++l) { w[l] = l == 0 ? lb.layers[0].whh : lb.layers[l].wcat; bias[l] = lb.layers[l].bperm; }
    const char* pre = lb.prefix.c_str();
    ProfSpan sp(e, cx.st, cx.live(), [&] { return persist ? kLstmPersistClass : kLstmWaveClass; }, fl, by);
    if (!carried)
        cx.launch("lstm state clear", pre,
                  [&] { return fc::launch_zero_fill(state, persist ? fc::lstm_persist_clear_floats(B, H) : 3 * L * BH, cx.st); });
    if (persist) {
        cx.launch("lstm", pre, [&] { return fc::launch_lstm_persist(w[0], w[1], bias[1], xproj, state, y.raw, B, H, T, e->status_dev, cx.st); });
    } else {
        for (int s = 0; s < T + L - 1; ++s)
            cx.launch("lstm step", pre, [&] {
                return steps ? fc::launch_lstm_wave(w, bias, xproj, state, state + 2 * L * BH, y.raw, B, H, T, L, s, cx.st, steps->lens, steps->div, steps->mul)
                             : fc::launch_lstm_wave(w, bias, xproj, state, state + 2 * L * BH, y.raw, B, H, T, L, s, cx.st);
            });
    }
    if (carried && (T & 1))
        for (int l = 0; l < L; ++l)
            cx.launch("lstm carry", pre, [&] {
                return hipMemcpyAsync(state + (size_t)(2 * l + 1) * BH, state + (size_t)(2 * l) * BH, BH * sizeof(float), hipMemcpyDeviceToDevice, cx.st);
            });
    return y;
}

// TransformerEncoder.forward (transformer.py:150-208) without the skip; returns plain y = after_norm(blocks(x)) [B][C][T].
// Per block (EncoderLayer.forward, transformer_encoder.py:92-150, normalize_before, dropout 0), as LauraTTS's full-sequence stacks run:
//   x += linear_out(MHA(norm1(x)));  x += w_2(relu(w_1(norm2(x))))
// Each residual add is fused into the LayerNorm that follows it (laura_kernels.hip layernorm_fm_kernel); LayerNorm eps 1e-12
// (layer_norm.py:21-23).  The input may carry a pending GroupNorm affine: it is materialised once.
// `kv` (a streaming push; null offline): the side's key / value cache inside the session state and the frames it holds.  The T frames
// of the push run through the same launches; K and V of every block are appended at [pos, pos + T) (seq_cache_append_kernel) and the
// attention reads them from there (seq_attn_cached_kernel: query i sees keys 0 .. pos + i).
// A slot push (`rows`): every row has its own frame count and position (seq_kernels.h, SeqRows); the device reads both from the push's
// table, host_n / host_pos are the same numbers on the host (null in a dry pass) and only size the attention's grid.
struct TfCache {
    float* base = nullptr;
    int pos = 0, F = 0;
    bool rows = false;
    fc::RagLen len;
    const int* pos_dev = nullptr;
    const int32_t* host_len = nullptr;
    const int32_t* host_pos = nullptr;
    bool grid_bound = false;        // a captured slot push: the attention's grid by the bound that depends on T alone (the rows' own counts and
                                    // positions are read on the device, a wave beyond a row's units returns at once: the same bits)
};
Act run_transformer(fc_engine* e, Ctx& cx, const TfBlock& tb, const Act& in, int T, const TfCache* kv = nullptr) {
    const int C = tb.C, B = cx.B, ff = tb.ff, DK = C / tb.heads;
    const long long sC = (long long)C * T;
    float* x = cx.alloc<float>((size_t)B * C * T);        // residual stream
    float* xn = cx.alloc<float>((size_t)B * C * T);       // LayerNorm output
    float* dl = cx.alloc<float>((size_t)B * C * T);       // branch output (pending residual add)
    float* qkv = cx.alloc<float>((size_t)B * 3 * C * T);
    float* ctx = cx.alloc<float>((size_t)B * C * T);
    float* hb = cx.alloc<float>((size_t)B * ff * T);
    Act y;
    y.C = C; y.T = T;
    y.raw = cx.alloc<float>((size_t)B * C * T);
    float* part = kv ? cx.alloc<float>(fc::seq_attn_cached_part_floats(B, tb.heads, DK)) : nullptr;     // of every push: no size depends on pos
    fc::SeqRows rows;                                      // a slot push: the rows' own (n_b, pos_b)
    double row_pairs = 0.0, row_keys = 0.0;                // its visible (query, key) pairs and the keys it reads, summed over the rows
    if (kv && kv->rows) {
        rows.len = kv->len; rows.pos = kv->pos_dev; rows.S = B; rows.T = T; rows.F = kv->F;
        for (int b = 0; b < B && kv->host_len; ++b) {
            const int len = kv->host_len[b], n = len > 0 ? fc::ragged_cols(len, rows.len.div, rows.len.mul, rows.len.add) : 0, pos = kv->host_pos[b];
            if (n < 1) continue;
            if (n > T || pos < 0 || pos + n > kv->F) { cx.fail("internal: a slot's frames leave the chunk or the key / value cache"); return y; }
            rows.max_waves = std::max(rows.max_waves, fc::seq_attn_rows_waves(n, pos));
            row_pairs += (double)n * pos + 0.5 * (double)n * (n + 1);
            row_keys += pos + n;
        }
        if (kv->grid_bound) rows.max_waves = (T + 15) / 16 * fc::kSeqCachedMaxUnits;
    }
    const double pairs = tb.layers.empty() ? 0.0
                         : kv && kv->rows ? row_pairs / B
                         : kv ? (double)T * kv->pos + 0.5 * (double)T * (T + 1)
                              : (e->arch.causal ? 0.5 * (double)T * (T + 1) : (double)T * T);
    const double attn_fl = 4.0 * B * pairs * C;           // q k^T and p v, every visible (query, key) pair
    cx.attn_flops += attn_fl * tb.layers.size();
    const char* pre = tb.prefix.c_str();
    auto ln = [&](const float* add, const float* g, const float* b, float* out) {
        cx.launch("transformer LayerNorm", pre, [] { return "layernorm_fm_kernel (transformer, residual add fused)"; }, 0.0, 4.0 * B * C * T * (add ? 4 : 2),
                  [&] { return fc::laura::launch_layernorm_fm(x, add, add ? x : nullptr, g, b, 1e-12f, 0, 1.f, out, B, C, T, cx.st); });
    };
    cx.launch("combine", pre, [&] { return fc::launch_combine(src_of(in), fc::Src(), 0, 1.f, nullptr, B, C, T, T, x, sC, T, 1, cx.st); });
    fc::Src sxn; sxn.ptr = xn; sxn.used = 1;
    fc::Src sctx; sctx.ptr = ctx; sctx.used = 1;
    fc::Src shb; shb.ptr = hb; shb.used = 1;
    const float* pending = nullptr;
    size_t block = 0;
    for (const TfLayer& L : tb.layers) {
        ln(pending, L.n1g, L.n1b, xn);
        run_conv(e, cx, L.qkv, sxn, fc::Src(), 0, T, qkv, 3 * sC, T, 1);
        if (kv && kv->rows) {
            const size_t plane = (size_t)B * C * kv->F;
            float* kc = kv->base ? kv->base + 2 * plane * block : nullptr;
            fc::SeqCacheAppendRows ap;
            ap.qkv = qkv; ap.kc = kc; ap.vc = kc ? kc + plane : nullptr; ap.C = C; ap.rows = rows;
            cx.launch("transformer cache append", pre, [] { return "seq_cache_append_rows_kernel (slot push: K and V of every row into its cache)"; }, 0.0,
                      4.0 * B * 4.0 * C * T, [&] { return fc::launch_seq_cache_append_rows(ap, cx.st); });
            fc::SeqAttnRows a;
            a.qkv = qkv; a.kc = ap.kc; a.vc = ap.vc; a.out = ctx; a.part = part; a.H = tb.heads; a.DK = DK; a.rows = rows;
            cx.launch("transformer cached attention", pre, [&] { return fc::seq_attn_rows_kernel_name(DK); }, attn_fl,
                      4.0 * C * (2.0 * B * T + 2.0 * row_keys), [&] { return fc::launch_seq_attn_rows(a, cx.st); });
        } else if (kv) {
            const size_t plane = (size_t)B * C * kv->F;
            float* kc = kv->base ? kv->base + 2 * plane * block : nullptr;
            fc::SeqCacheAppend ap;
            ap.qkv = qkv; ap.kc = kc; ap.vc = kc ? kc + plane : nullptr; ap.B = B; ap.C = C; ap.n = T; ap.pos = kv->pos; ap.F = kv->F;
            cx.launch("transformer cache append", pre, [] { return "seq_cache_append_kernel (streaming: K and V of a push into the cache)"; }, 0.0,
                      4.0 * B * 4.0 * C * T, [&] { return fc::launch_seq_cache_append(ap, cx.st); });
            fc::SeqAttnCached a;
            a.qkv = qkv; a.kc = ap.kc; a.vc = ap.vc; a.out = ctx; a.part = part; a.B = B; a.H = tb.heads; a.DK = DK; a.n = T; a.pos = kv->pos; a.F = kv->F;
            cx.launch("transformer cached attention", pre, [&] { return fc::seq_attn_cached_kernel_name(DK); }, attn_fl,
                      4.0 * B * C * (2.0 * T + 2.0 * (kv->pos + T)), [&] { return fc::launch_seq_attn_cached(a, cx.st); });
        } else {
            fc::SeqAttn a;
            a.qkv = qkv; a.out = ctx; a.B = B; a.H = tb.heads; a.DK = DK; a.T = T; a.causal = e->arch.causal ? 1 : 0;
            cx.launch("transformer attention", pre, [&] { return fc::seq_attn_kernel_name(DK); }, attn_fl, 4.0 * B * 4.0 * C * T,
                      [&] { return fc::launch_seq_attn(a, cx.st); });
        }
        ++block;
        run_conv(e, cx, L.out, sctx, fc::Src(), 0, T, dl, sC, T, 1);
        ln(dl, L.n2g, L.n2b, xn);
        run_conv(e, cx, L.ff1, sxn, fc::Src(), 0, T, hb, (long long)ff * T, T, 1);
        cx.launch("ReLU", pre, [] { return "act_kernel (transformer feed-forward ReLU)"; }, 0.0, 8.0 * B * ff * T,
                  [&] { return fc::laura::launch_act(hb, (size_t)B * ff * T, 1, cx.st); });
        run_conv(e, cx, L.ff2, shb, fc::Src(), 0, T, dl, sC, T, 1);
        pending = dl;
    }
    ln(pending, tb.ag, tb.ab, y.raw);                      // after_norm
    return y;
}

// the bottleneck sequence model of one side: SLSTM or TransformerEncoder, output plain [B][C][T] without the skip
bool has_seq(const LstmBlock& lb, const TfBlock& tb) { return lb.H != 0 || tb.C != 0; }
Act run_seq(fc_engine* e, Ctx& cx, const LstmBlock& lb, const TfBlock& tb, const Act& in, int T) {
    return tb.C ? run_transformer(e, cx, tb, in, T) : run_lstm(e, cx, lb, in, T);
}

// SEANetResnetBlock (seanet_encoder.py:16-61): returns the two raw branches whose GroupNorm'd sum is the output
// The block's input is one tensor (first block of a stage) or the pending sum of the previous block's two branches.
// shortcut(x) and block.1(ELU(x)) of a thin residual block from ONE staging of x (kernels.hip 1c); same outputs / statistics
// contract as two run_conv() calls
void run_reshead(fc_engine* e, Ctx& cx, const fc_engine::ResBlock& R, fc::Src a0, fc::Src a1, int T, Act* sc, Act* b1) {
    const int C = R.shortcut.cin, hid = R.block1.cout;
    const ConvGeom g = conv_geom(R.block1, T);              // stride 1: Tout == T
    sc->C = C; sc->T = T; b1->C = hid; b1->T = T;
    sc->raw = cx.alloc<float>((size_t)cx.B * C * T);
    b1->raw = cx.alloc<float>((size_t)cx.B * hid * T);
    fc::ResHeadLaunch c;
    c.s0 = a0; c.s1 = a1; c.wsc = R.wsc; c.wb1 = R.wb1; c.bsc = R.bsc; c.bb1 = R.bb1;
    c.out_sc = sc->raw; c.out_b1 = b1->raw;
    c.B = cx.B; c.C = C; c.T = T; c.k = R.block1.k; c.dil = R.block1.dil; c.padL = g.padL; c.padR = g.padR;
    c.alpha = e->arch.elu_alpha;
    const int nblk = fc::reshead_ntiles(T);
    if (R.shortcut.has_norm) {
        c.part_sc = cx.alloc<double>((size_t)cx.B * nblk * 2);
        c.part_b1 = cx.alloc<double>((size_t)cx.B * nblk * 2);
        sc->aff = cx.alloc<float>((size_t)cx.B * C * 2); sc->normed = true;
        b1->aff = cx.alloc<float>((size_t)cx.B * hid * 2); b1->normed = true;
    }
    const double fl = 2.0 * cx.B * (double)T * ((double)C * C + (double)hid * C * R.block1.k);
    const double by = 4.0 * cx.B * (double)T * ((double)C * (a1.used ? 2 : 1) + C + hid);      // x read ONCE, both outputs written
    cx.conv_flops += fl; cx.conv_bytes += by;
    auto cls = [&] {
        char nm[64];
        snprintf(nm, sizeof(nm), "reshead_kernel<%d, %d, %s>", C, R.block1.k, a1.used ? "true" : "false");
        return std::string(nm);
    };
    cx.conv_launch("fused res-block head", R.shortcut.prefix.c_str(), cls, fl, by, [&] { return fc::launch_reshead(c, cx.st); });
    conv_finish(e, cx, R.shortcut, c.part_sc, nblk, (double)C * T, sc->aff);
    conv_finish(e, cx, R.block1, c.part_b1, nblk, (double)hid * T, b1->aff);
}

// ---- the forward walk of the time-domain nets: ONE walk for an offline call, a ragged call and a push of either kind of session.  The
// four kinds of pass differ in three places and nowhere else: the conv step (walk_conv), the head of a residual block (run_resblocks) and
// the bottleneck (run_bottleneck).
struct Pass {
    enum Kind { Offline, Stream, Ragged, Slots } kind = Offline;     // Offline: one call over the whole utterance, nothing below is read
    // Stream, Slots (a push): the session, and the pushes this side (encoder / decoder) of it has taken before this one
    const Session* sess = nullptr;
    int n = 0;
    // Stream: the utterance's last encoder push (a decoder push never is)
    bool final = false;
    // Ragged, Slots: every row ends at its own length.  lengths: device [B], clamped (null in a dry pass; 0 = an idle slot); they count
    // encoder input samples, or, on the decoder side, what frame_div of them make a frame (the hop behind an encoder, 1 for token_lengths)
    const int* lengths = nullptr;
    int frame_div = 1;
    // Slots: `flags` (device [S], kSlotStart | kSlotFinal) per row; host_push = the counts and flags on the host ([2 S]; null in a dry pass)
    const int* flags = nullptr;
    const int32_t* host_push = nullptr;
    // Slots of a session with a key / value cache: the frames every row's utterance has cached on this side (device [S], behind the flags
    // in the same copy; a START row's is 0); host_push is then [3 S]
    const int* pos = nullptr;
    // Slots: the pass is being captured into a graph that later pushes replay, so nothing it enqueues may depend on the rows' host values
    bool graphed = false;
};

// the columns of every row at the input of the layer the walk of a ragged pass stands at (the rule: ragged_kernels.h)
inline fc::RagLen ragged_len(const Ctx& cx, const Pass& p) {
    fc::RagLen r;
    r.lens = p.lengths;
    if (cx.dec_side) { r.div = p.frame_div; r.mul = cx.rate; }
    else r.div = cx.rate;
    return r;
}

Act ragged_conv(fc_engine* e, Ctx& cx, const Pass& p, const ConvLayer& L, fc::Src s0, fc::Src s1, int elu, int T);
Act stream_conv(fc_engine* e, Ctx& cx, const Pass& p, const ConvLayer& L, fc::Src s0, fc::Src s1, int elu, int Tc);
Act slots_conv(fc_engine* e, Ctx& cx, const Pass& p, const ConvLayer& L, fc::Src s0, fc::Src s1, int elu, int T);
float* lstm_state(const Session& s, bool dec);
TfCache tf_cache(const Session& s, bool dec, int pos);

// the conv step.  A push stages the layers that carry a left context and runs them over [carry | chunk] (stream_conv; slots_conv with
// every row at its own place); its pointwise layers run as offline.  A ragged pass stages every conv that looks beyond its own column
// (k > 1) or normalises over the row (ragged_conv); a pointwise weight_norm conv maps column to column and runs as offline, garbage
// columns included.
Act walk_conv(fc_engine* e, Ctx& cx, const Pass& p, Role role, const ConvLayer& L, fc::Src s0, fc::Src s1, int elu, int T) {
    switch (p.kind) {
        case Pass::Stream: if (carries_context(role)) return stream_conv(e, cx, p, L, s0, s1, elu, T); break;
        case Pass::Slots: if (carries_context(role)) return slots_conv(e, cx, p, L, s0, s1, elu, T); break;
        case Pass::Ragged: if (L.k > 1 || L.has_norm) return ragged_conv(e, cx, p, L, s0, s1, elu, T); break;
        case Pass::Offline: break;
    }
    return run_conv(e, cx, L, s0, s1, elu, T);
}

// the bottleneck of one side: the sources of the conv behind it = the sequence model's output (plus its input with lstm_skip), or x itself
// in a net without one.  A push continues the per-step LSTM on the session's state, or the transformer on the session's key / value
// cache (a session opened with max_frames); a slot push does either with every row at its own place.
void run_bottleneck(fc_engine* e, Ctx& cx, const Pass& p, bool dec, const Act& x, fc::Src* a0, fc::Src* a1) {
    const LstmBlock& lb = dec ? e->dec_lstm : e->enc_lstm;
    const TfBlock& tb = dec ? e->dec_tf : e->enc_tf;
    *a0 = src_of(x); *a1 = fc::Src();
    if (!has_seq(lb, tb)) return;
    Act y;
    switch (p.kind) {
        case Pass::Stream:
            if (tb.C) {
                const TfCache kv = tf_cache(*p.sess, dec, dec ? static_cast<const fc_stream*>(p.sess)->dec_frames : static_cast<const fc_stream*>(p.sess)->enc_frames);
                if (!cx.dry && kv.pos + x.T > p.sess->max_frames) { cx.fail("internal: a push past max_frames reached the transformer"); return; }
                y = run_transformer(e, cx, tb, x, x.T, &kv);
            } else {
                y = run_lstm(e, cx, lb, x, x.T, lstm_state(*p.sess, dec));
            }
            break;
        case Pass::Slots: {                               // every row takes its own frames: of the LSTM's steps, or of the cache and the attention
            const fc::RagLen steps = ragged_len(cx, p);
            if (tb.C) {
                TfCache kv = tf_cache(*p.sess, dec, 0);
                kv.rows = true; kv.len = steps; kv.pos_dev = p.pos;
                if (p.host_push) { kv.host_len = p.host_push; kv.host_pos = p.host_push + 2 * cx.B; }
                kv.grid_bound = p.graphed;
                y = run_transformer(e, cx, tb, x, x.T, &kv);
            } else {
                y = run_lstm(e, cx, lb, x, x.T, lstm_state(*p.sess, dec), &steps);
            }
            break;
        }
        case Pass::Ragged:                                // forward in time, rows independent: as offline, garbage columns included
        case Pass::Offline: y = run_seq(e, cx, lb, tb, x, x.T); break;
    }
    *a0 = src_of(y);
    if (e->arch.lstm_skip) *a1 = src_of(x);
}

// SEANetResnetBlock (seanet_encoder.py:16-61) over the blocks of a stage: returns the two raw branches whose GroupNorm'd sum is the output
// The block's input is one tensor (first block of a stage) or the pending sum of the previous block's two branches.
void run_resblocks(fc_engine* e, Ctx& cx, const Pass& p, const fc_engine::Stage& S, fc::Src a0, fc::Src a1, int T, Act* sc, Act* b3) {
    for (const auto& R : S.res) {
        Act b1;
        if (p.kind == Pass::Offline && R.fused_head && !a0.div) {      // the fused head has no form that stages a carry or a row end
            run_reshead(e, cx, R, a0, a1, T, sc, &b1);
        } else {
            *sc = walk_conv(e, cx, p, Role::Shortcut, R.shortcut, a0, a1, 0, T);
            b1 = walk_conv(e, cx, p, Role::Block1, R.block1, a0, a1, 1, T);
        }
        *b3 = walk_conv(e, cx, p, Role::Block3, R.block3, src_of(b1), fc::Src(), 1, b1.T);
        a0 = src_of(*sc); a1 = src_of(*b3);
    }
}

// SEANetEncoder.forward: wav [B][C][T] (a chunk of it in a push; with the caller's divisor) -> last conv (raw + affine), T -> Tf
Act run_encoder(fc_engine* e, Ctx& cx, const Pass& p, fc::Src wav, int T) {
    cx.dec_side = false; cx.rate = 1; cx.no_xq = p.kind == Pass::Ragged;
    Act x = walk_conv(e, cx, p, Role::First, e->enc_first, wav, fc::Src(), 0, T);
    for (auto& S : e->enc_stages) {
        Act sc, b3;
        run_resblocks(e, cx, p, S, src_of(x), fc::Src(), x.T, &sc, &b3);
        x = walk_conv(e, cx, p, Role::Resample, S.resample, src_of(sc), src_of(b3), 1, sc.T);
        cx.rate *= S.resample.stride;
    }
    fc::Src a0, a1;
    run_bottleneck(e, cx, p, false, x, &a0, &a1);
    return walk_conv(e, cx, p, Role::Last, e->enc_last, a0, a1, 1, x.T);
}

// SEANetDecoder.forward: z [B][D][Tf] plain -> last conv (raw [B][C][Tf*hop] + affine).  A push of Tf frames gives Tf * hop samples
// without look-ahead (causal unpad1d trims on the right only).
Act run_decoder(fc_engine* e, Ctx& cx, const Pass& p, const float* z_bdt, int Tf) {
    fc::Src s; s.ptr = z_bdt; s.used = 1;
    cx.dec_side = true; cx.rate = 1; cx.no_xq = p.kind == Pass::Ragged;
    Act x = walk_conv(e, cx, p, Role::First, e->dec_first, s, fc::Src(), 0, Tf);
    fc::Src a0, a1;
    run_bottleneck(e, cx, p, true, x, &a0, &a1);
    int T = Tf;
    for (auto& S : e->dec_stages) {
        Act up = walk_conv(e, cx, p, Role::Resample, S.resample, a0, a1, 1, T);
        cx.rate *= S.resample.stride;
        Act sc, b3;
        run_resblocks(e, cx, p, S, src_of(up), fc::Src(), up.T, &sc, &b3);
        a0 = src_of(sc); a1 = src_of(b3);
        T = up.T;
    }
    return walk_conv(e, cx, p, Role::Last, e->dec_last, a0, a1, 1, T);
}


// ---- STFT-domain codec: execution over frequency-major activations --------------------------------------------------------------
// fc_engine::halo2 (set by build_plan_2d): frequency halo rows of every 2-D activation that a kf > 1 conv may read = the largest one-sided
// frequency padding of the net's convs (7x7: 3, 3x3: 1, strided 2 fr rows with stride fr: ceil(fr / 2))

// The activated input of a 2-D conv (pending affines, second source, ELU) materialised once, frequency-major with x0's halo rows, which the
// pass writes itself where it can (else a halo_rows launch).  pad > 0: an input of F <= pad rows; pad2d zero-extends it AFTER the activation
// (conv.py:100-119), so its halo rows are zeros of the activated image (or reflections through that extension), not the activation of raw
// zero rows.  Only nets with frequency ratio 1 (F = 1 at the bottleneck) get there; the recipes never do.
Act2 materialise2d(fc_engine* e, Ctx& cx, const ConvLayer& L, const Act2& x0, const Act2* x1, int elu, int pad) {
    const int B = cx.B, C = L.c2d;
    Act2 m;
    m.C = C; m.F = x0.F; m.T = x0.T; m.halo = x0.halo;
    m.buf = cx.alloc<float>((size_t)B * (m.F + 2 * m.halo) * C * m.T);
    const bool fuse_halo = !pad && halo_fuse_on() && m.F > m.halo;
    cx.launch("combine2d", L.prefix.c_str(), [&] {
        if (x0.halo < pad) return hipErrorInvalidValue;
        return fc::launch_combine2d(x0.buf, x0.aff, x0.halo, x1 ? x1->buf : nullptr, x1 ? x1->aff : nullptr, x1 ? x1->halo : 0, elu, e->arch.elu_alpha,
                                    B, m.F, C, m.T, m.buf, m.halo, cx.st, fuse_halo ? 1 : 0);
    });
    if (pad) cx.launch("halo rows", L.prefix.c_str(), [&] { return fc::launch_halo_rows_short(m.buf, B, m.F, m.halo, pad, C, m.T, cx.st); });
    else if (!fuse_halo) cx.launch("halo rows", L.prefix.c_str(), [&] { return fc::launch_halo_rows(m.buf, B, m.F, m.halo, C, m.T, 0, cx.st); });
    return m;
}

// SConv2d.forward (conv.py:342-381) as ONE launch of the 1-D implicit-GEMM kernel over B * Fo virtual utterances
Act2 run_conv2d(fc_engine* e, Ctx& cx, const ConvLayer& L, Act2 x0, const Act2* x1, int elu, int out_halo) {
    const int B = cx.B, C = L.c2d, kf = L.kf, sf = L.sf;
    const int tot_f = (kf - 1) - (sf - 1), f_after = tot_f / 2, f_before = tot_f - f_after;     // no extra padding on the frequency axis
    const int Fo = (x0.F + tot_f - kf) / sf + 1;
    const ConvGeom g = conv_geom(L, x0.T);
    const int fpad = std::max(f_before, f_after);
    if (x0.F <= fpad) { x0 = materialise2d(e, cx, L, x0, x1, elu, fpad); x1 = nullptr; elu = 0; }
    bool mat;
    if (L.w_group) {
        // the grouped direct kernel's strided 8-row layers read every input sample from 2 output rows x ~1.25 lanes with a two-source
        // prologue (11 VALU per read): activate once instead (FC_GCONV_MAT=0: in-kernel prologue)
        static const int gmat = fc::ab_knob("FC_GCONV_MAT", 1);
        mat = gmat && kf >= 4 && x1;
    } else {
        // layers with several M tiles: materialise the activated input once (as run_conv does); the few-output FMA kernel re-stages every
        // input row for each of the kf output rows that read it: activate once instead
        static const int few_mat = fc::ab_knob("FC_FEWOUT_MAT", 1);
        const bool few_out = few_mat && L.cout <= 4 && L.stride == 1 && sf == 1 && (L.k == 3 || L.k == 5 || L.k == 7) && kf > 1;   // = pack_conv2d's w_plain rule
        mat = (L.Mpad / L.BM >= 3 || few_out || L.force_plain) && (x0.normed || x1 || elu);
    }
    if (mat) { x0 = materialise2d(e, cx, L, x0, x1, elu, 0); x1 = nullptr; elu = 0; }
    Act2 o;
    o.C = L.cout; o.F = Fo; o.T = g.Tout; o.halo = out_halo;
    o.buf = cx.alloc<float>((size_t)B * (Fo + 2 * out_halo) * L.cout * g.Tout);
    if (!cx.dry && (x0.halo < f_before || x0.halo < f_after || (x1 && x1->halo != x0.halo))) {
        cx.fail("internal: frequency halo too small for " + L.prefix);
        return o;
    }
    const long long rowsz = (long long)C * x0.T, orow = (long long)L.cout * g.Tout;
    const double by = 4.0 * B * ((double)C * x0.F * x0.T * (x1 ? 2 : 1) + (double)L.cout * Fo * g.Tout);
    o.normed = L.has_norm;                  // weight_norm nets: no statistics, no affine
    if (L.w_group) {     // grouped conv with 2 / 4 channels per group: direct FMA kernel, prologue fused, no GEMM
        fc::GConvLaunch c;
        c.src0 = at(x0.buf, (x0.halo - f_before) * rowsz); c.aff0 = x0.aff;
        if (x1) { c.src1 = at(x1->buf, (x1->halo - f_before) * rowsz); c.aff1 = x1->aff; }
        c.w = L.w_group; c.bias = L.bias;
        c.out = at(o.buf, out_halo * orow);
        c.B = B; c.C = C; c.M = L.cout; c.G = L.groups; c.Tin = x0.T; c.Tout = g.Tout; c.Fo = Fo; c.kf = kf; c.kt = L.k; c.sf = sf; c.st = L.stride;
        c.padL = g.padL; c.padR = g.padR; c.elu = elu; c.alpha = e->arch.elu_alpha;
        c.guard_lo = cx.base; c.guard_hi = cx.base ? cx.base + cx.cap : nullptr;      // both sources are buffers of THIS workspace (Ctx::alloc)
        c.in_sB = (long long)(x0.F + 2 * x0.halo) * rowsz; c.in_sF = rowsz;
        c.out_sB = (long long)(Fo + 2 * out_halo) * orow; c.out_sF = orow;
        const bool fuse_halo = halo_fuse_on() && fc::gconv2d_fuses_halo(kf, L.k, L.stride, Fo, out_halo);
        c.out_halo = fuse_halo ? out_halo : 0;
        const int nblk = fc::gconv2d_nblk(g.Tout, Fo, L.groups, kf);
        c.partials = L.has_norm ? cx.alloc<double>((size_t)B * nblk * 2) : nullptr;
        o.aff = L.has_norm ? cx.alloc<float>((size_t)B * L.cout * 2) : nullptr;
        const double fl = 2.0 * B * Fo * (double)L.cout * (C / L.groups) * kf * L.k * g.Tout;
        cx.conv_flops += fl; cx.conv_bytes += by;
        auto cls = [&] {
            char nm[64];
            snprintf(nm, sizeof(nm), "gconv2d_kernel<%d, %d, %d, %d, %d, %s>", C / L.groups, L.cout / L.groups, kf, L.k, L.stride, x1 ? "true" : "false");
            return std::string(nm);
        };
        cx.conv_launch("grouped 2-D conv", L.prefix.c_str(), cls, fl, by, [&] { return fc::launch_gconv2d(c, cx.st); });
        conv_finish(e, cx, L, c.partials, nblk, (double)L.cout * Fo * g.count_T, o.aff, out_halo && !fuse_halo ? &o : nullptr);
        return o;
    }
    fc::ConvLaunch c = conv_launch_of(L, B * Fo, x0.T, g);
    c.s0.ptr = at(x0.buf, (x0.halo - f_before) * rowsz); c.s0.aff = x0.aff; c.s0.used = x0.normed ? 3 : 1;
    if (x1) { c.s1.ptr = at(x1->buf, (x1->halo - f_before) * rowsz); c.s1.aff = x1->aff; c.s1.used = x1->normed ? 3 : 1; }
    c.elu = elu; c.alpha = e->arch.elu_alpha;
    c.Tout = g.Tout; c.Fo = Fo; c.affC = C;
    c.in_sB0 = (long long)(x0.F + 2 * x0.halo) * rowsz; c.in_sB1 = (long long)sf * rowsz;
    c.out = at(o.buf, out_halo * orow);
    c.out_sB = (long long)(Fo + 2 * out_halo) * orow; c.out_sF = orow; c.out_sM = g.Tout; c.out_sT = 1;
    const int nblk = fc::conv_nblk(c);
    c.partials = L.has_norm ? cx.alloc<double>((size_t)B * Fo * nblk * 2) : nullptr;
    o.aff = L.has_norm ? cx.alloc<float>((size_t)B * L.cout * 2) : nullptr;
    const double fl = 2.0 * B * Fo * (double)L.M * L.cin * L.gk * g.Tout;
    cx.conv_flops += fl; cx.conv_bytes += by;
    cx.conv_launch("2-D conv", L.prefix.c_str(), [&] { return conv_class(c); }, fl, by, [&] { return fc::launch_conv(c, cx.st); });
    conv_finish(e, cx, L, c.partials, nblk * Fo, (double)L.cout * Fo * g.count_T, o.aff, out_halo ? &o : nullptr);
    return o;
}

// SEANetResnetBlock2d.forward (seanet_encoder.py:239-240) over the blocks of a stage: returns the two raw branches of the last block
void run_resblocks2d(fc_engine* e, Ctx& cx, const fc_engine::Stage& S, Act2 a0, const Act2* a1, Act2* sc, Act2* b3) {
    Act2 prev1;
    for (const auto& R : S.res) {
        *sc = run_conv2d(e, cx, R.shortcut, a0, a1, 0, e->halo2);
        Act2 b1 = run_conv2d(e, cx, R.block1, a0, a1, 1, 0);
        *b3 = run_conv2d(e, cx, R.block3, b1, nullptr, 1, e->halo2);
        a0 = *sc; prev1 = *b3; a1 = &prev1;
    }
}

// SConvTranspose2d.forward (conv.py:408-447): sf launches (one per output-frequency phase) of the transposed 1-D GEMM over the
// materialised, zero-haloed input; GroupNorm statistics over the UNTRIMMED (Fin + 1) sf x (Tin + 1) st output
Act2 run_convtr2d(fc_engine* e, Ctx& cx, const ConvLayer& S, const std::vector<ConvLayer>& phases, const Act2& x0, const Act2* x1, bool last,
                  int out_halo) {
    const int B = cx.B, C = S.c2d, Fin = x0.F, T = x0.T, sf = S.sf, st = S.stride, cout = S.cout;
    Act2 z;                                                   // ELU(x) with one zero row above and below
    z.C = C; z.F = Fin; z.T = T; z.halo = 1;
    z.buf = cx.alloc<float>((size_t)B * (Fin + 2) * C * T);
    const ConvGeom g = conv_geom(phases[0], T);               // time axis: Tout = T * st, count_T = (T + 1) * st
    int f_r = sf / 2;
    const int f_l = sf - f_r;
    if (last && f_r > 0) f_r -= 1;                            // last_out_padding [(0, 1), (0, 0)] (seanet_decoder.py:279,316)
    const int Fout = (Fin + 1) * sf - f_l - f_r;
    Act2 o;
    o.C = cout; o.F = Fout; o.T = g.Tout; o.halo = out_halo;
    const long long orow = (long long)cout * g.Tout;
    o.buf = cx.alloc<float>((size_t)B * (Fout + 2 * out_halo) * orow);
    fc::ConvLaunch c0;
    c0.M = phases[0].M; c0.BM = phases[0].BM; c0.BN = phases[0].BN; c0.Tout = T + 1;
    const int nblk = fc::conv_nblk(c0);
    const long long part_row = (long long)(Fin + 1) * nblk;
    const int gnblk = fc::gconvtr2d_nblk(T, st, Fin, sf);     // partial slots of the grouped direct kernel (same buffer)
    const bool has_norm = S.has_norm;
    const int t_trimL = S.causal ? 0 : st - st / 2;           // unpad2d: causal (trim_right_ratio 1) trims the time axis on the right only (conv.py:427-431)
    double* partials = has_norm ? cx.alloc<double>((size_t)B * std::max<long long>(sf * part_row, gnblk) * 2) : nullptr;
    o.aff = has_norm ? cx.alloc<float>((size_t)B * cout * 2) : nullptr;
    o.normed = has_norm;
    const double fl = 2.0 * B * (Fin + 1) * (double)phases[0].M * 2 * C * 2 * (T + 1) * sf;
    const double by = 4.0 * B * ((double)C * Fin * T * (x1 ? 2 : 1) + (double)cout * Fout * g.Tout);
    cx.conv_flops += fl; cx.conv_bytes += by;
    const char* pre = S.prefix.c_str();
    const double gn_count = (double)cout * (Fin + 1) * sf * g.count_T;
    cx.launch("combine2d", pre, [&] {
        return fc::launch_combine2d(x0.buf, x0.aff, x0.halo, x1 ? x1->buf : nullptr, x1 ? x1->aff : nullptr, x1 ? x1->halo : 0, 1, e->arch.elu_alpha,
                                    B, Fin, C, T, z.buf, 1, cx.st, halo_fuse_on() ? 2 : 0);      // 2: its zero rows too
    });
    if (!halo_fuse_on()) cx.launch("halo rows", pre, [&] { return fc::launch_halo_rows(z.buf, B, Fin, 1, C, T, 1, cx.st); });
    if (phases[0].w_group) {          // grouped (2 in / 1 out channel per group): one direct launch over the untrimmed output
        const bool fuse_halo = halo_fuse_on() && Fout > out_halo;
        cx.conv_launch("grouped 2-D transposed conv", pre, [&] { return "gconvtr2d_kernel<" + std::to_string(st) + ">"; },
                       2.0 * B * (double)cout * 8 * (Fin + 1) * sf * (T + 1) * st, by, [&] {
                           return fc::launch_gconvtr2d(z.buf, phases[0].w_group, phases[0].w_plain, o.buf + (long long)out_halo * orow, partials, B, C, cout,
                                                       Fin, T, sf, st, f_l, Fout, t_trimL, g.Tout, (long long)(Fout + 2 * out_halo) * orow, cx.st,
                                                       fuse_halo ? out_halo : 0);
                       });
        conv_finish(e, cx, phases[0], partials, gnblk, gn_count, o.aff, out_halo && !fuse_halo ? &o : nullptr);
        return o;
    }
    for (int p = 0; p < sf; ++p) {
        const ConvLayer& L = phases[p];
        fc::ConvLaunch c = conv_launch_of(L, B * (Fin + 1), T, g);
        c.s0.ptr = z.buf; c.s0.used = 1;
        c.pad_zero = 1;
        c.Tout = T + 1; c.up_r = st; c.trimL = t_trimL; c.Tfinal = g.Tout;
        c.Fo = Fin + 1; c.affC = C;
        c.in_sB0 = (long long)(Fin + 2) * C * T; c.in_sB1 = (long long)C * T;
        c.out = at(o.buf, (out_halo + p - f_l) * orow);                  // rows outside [0, Fout) are never stored (store range below)
        c.out_sB = (long long)(Fout + 2 * out_halo) * orow; c.out_sF = (long long)sf * orow; c.out_sM = g.Tout; c.out_sT = 1;
        int lo = f_l - p;                                            // q * sf + p - f_l >= 0
        lo = lo <= 0 ? 0 : (lo + sf - 1) / sf;
        int hi = (Fout - 1 + f_l - p) >= 0 ? (Fout - 1 + f_l - p) / sf + 1 : 0;   // q * sf + p - f_l <= Fout - 1
        if (hi > Fin + 1) hi = Fin + 1;
        c.store_lo = lo; c.store_hi = hi;
        c.partials = has_norm ? at(partials, p * part_row * 2) : nullptr;
        c.part_sB0 = (long long)sf * part_row;
        cx.conv_launch("2-D transposed conv", pre, [&] { return conv_class(c); }, fl / sf, by / sf, [&] { return fc::launch_conv(c, cx.st); });
    }
    conv_finish(e, cx, phases[0], partials, (int)(sf * part_row), gn_count, o.aff, out_halo ? &o : nullptr);
    return o;
}

int stft_frames(const fc_engine* e, int T) { return 1 + T / e->arch.stft_hop; }

// fc_debug_freq_features: one-shot capture (mode 1) or override (mode 2) of the STFT-domain feature tensor of the next encode
struct FeatHook { float* buf = nullptr; size_t cap = 0; int mode = 0; };
thread_local FeatHook g_feat_hook;

// FreqCodec._encode_frame (codec_freq.py:330-392, mag_phase) + SEANetEncoder2d.forward: wav -> last conv (raw + affine) at Tf frames
Act run_encoder_2d(fc_engine* e, Ctx& cx, const float* wav, int T, const float* scale) {
    const fc_arch& a = e->arch;
    const int B = cx.B, hop = a.stft_hop, F = a.n_fft / 2 + 1, Tp = stft_frames(e, T), taps = ceil_div_i(a.n_fft, hop), Mp = Tp + taps - 1;
    float* xp = cx.alloc<float>((size_t)B * hop * Mp);
    if (!cx.dry && T <= a.n_fft / 2) cx.fail("utterance shorter than n_fft/2 + 1 samples (torch.stft reflect padding needs more)");
    cx.launch("polyphase", "", [&] { return fc::launch_polyphase_in(wav, a.audio_normalize ? scale : nullptr, B, T, hop, a.n_fft, Mp, xp, cx.st); });
    fc::Src sx; sx.ptr = xp; sx.used = 1;
    Act spec = run_conv(e, cx, e->stft, sx, fc::Src(), 0, Mp);                     // [B][2F][Tp]: re rows, then im rows
    Act2 feats;
    feats.C = a.input_channels; feats.F = F; feats.T = Tp; feats.halo = e->halo2;
    feats.buf = cx.alloc<float>((size_t)B * (F + 2 * e->halo2) * feats.C * Tp);
    cx.launch("stft feature", "", [&] { return fc::launch_stft_feats(spec.raw, B, F, Tp, (long long)2 * F * Tp, e->halo2, feats.C, feats.buf, cx.st); });
    // test hooks (fc_debug_freq_features): hand the features out / take them from the caller, in the reference's [B][C][F][Tp]
    if (g_feat_hook.mode != 0) {
        if (!cx.dry && (size_t)B * feats.C * F * Tp * sizeof(float) > g_feat_hook.cap) cx.fail("fc_debug_freq_features: buffer too small");
        cx.launch("feature hook", "", [&] { return fc::launch_feats_relayout(feats.buf, g_feat_hook.buf, B, feats.C, F, Tp, e->halo2, g_feat_hook.mode == 1, cx.st); });
        if (!cx.dry) g_feat_hook.mode = 0;            // one shot
    }
    cx.launch("halo rows", "", [&] { return fc::launch_halo_rows(feats.buf, B, F, e->halo2, feats.C, Tp, 0, cx.st); });
    Act2 x = run_conv2d(e, cx, e->enc2_first, feats, nullptr, 0, e->halo2);
    for (size_t si = 0; si < e->enc_stages.size(); ++si) {
        auto& S = e->enc_stages[si];
        Act2 sc, b3;
        run_resblocks2d(e, cx, S, x, nullptr, &sc, &b3);
        x = run_conv2d(e, cx, S.resample, sc, &b3, 1, si + 1 == e->enc_stages.size() ? 0 : e->halo2);
    }
    if (!cx.dry && x.F != 1) cx.fail("the 2-D encoder must reduce the frequency axis to one bin (n_fft / ratios mismatch)");
    Act x1;                                                                        // ReshapeModule: [B][1][C][T] is [B][C][T]
    x1.raw = x.buf; x1.aff = x.aff; x1.C = x.C; x1.T = x.T; x1.normed = x.normed;
    fc::Src a0, a1;
    run_bottleneck(e, cx, Pass(), false, x1, &a0, &a1);
    return run_conv(e, cx, e->enc_last, a0, a1, 1, x1.T);
}

// FreqCodec._decode_frame behind the 2-D decoder (codec_freq.py:419-448): the decoder's last conv (raw, frequency-major, its GroupNorm
// pending as last.aff) -> spectrum rows [B][2F][Tp] -> inverse-DFT GEMM -> envelope division, centre trim, x scale[b], out_len samples.
// spec_out (fc_freq_synthesis): where the spectrum rows lie in the workspace.
void run_synthesis_2d(fc_engine* e, Ctx& cx, const Act2& last, const float* scale, int out_len, float* wav, float** spec_out = nullptr) {
    const fc_arch& a = e->arch;
    const int B = cx.B, hop = a.stft_hop, F = a.n_fft / 2 + 1, taps = ceil_div_i(a.n_fft, hop);
    const int Tp2 = last.T, Mp2 = Tp2 + taps - 1;
    float* spec = cx.alloc<float>((size_t)B * 2 * F * Tp2);
    if (spec_out) *spec_out = spec;
    if (!cx.dry && last.F != F) cx.fail("internal: decoder frequency rows != n_fft / 2 + 1");
    if (!cx.dry && out_len > hop * (Tp2 - 1)) cx.fail("out_len exceeds the inverse STFT's length stft_hop * (frames - 1)");
    cx.launch("spectrum", "", [&] { return fc::launch_spec_from_dec(last.buf, last.aff, B, F, Tp2, last.halo, a.input_channels, spec, cx.st); });
    fc::Src ss; ss.ptr = spec; ss.used = 1;
    Act yp = run_conv(e, cx, e->istft, ss, fc::Src(), 0, Tp2);                      // [B][hop][Mp2]
    if (!cx.dry && yp.T != Mp2) cx.fail("internal: inverse-STFT GEMM length");
    cx.launch("istft finish", "", [&] { return fc::launch_istft_finish(yp.raw, e->win2, B, hop, a.n_fft, Mp2, Tp2, scale, out_len, wav, cx.st); });
}

// SEANetDecoder2d.forward + FreqCodec._decode_frame (codec_freq.py:409-448, mag_phase): z [B][D][Tf] -> wav [B][out_len]
void run_decoder_2d(fc_engine* e, Ctx& cx, const float* z_bdt, int Tf, const float* scale, int out_len, float* wav) {
    const fc_arch& a = e->arch;
    fc::Src s; s.ptr = z_bdt; s.used = 1;
    Act x = run_conv(e, cx, e->dec_first, s, fc::Src(), 0, Tf);
    Act2 a0, a1;
    bool has1 = false;
    auto as2 = [](const Act& t) { Act2 r; r.buf = t.raw; r.aff = t.aff; r.C = t.C; r.F = 1; r.T = t.T; r.halo = 0; r.normed = t.normed; return r; };
    a0 = as2(x);
    if (has_seq(e->dec_lstm, e->dec_tf)) {
        Act y = run_seq(e, cx, e->dec_lstm, e->dec_tf, x, x.T);
        a0 = as2(y);
        if (a.lstm_skip) { a1 = as2(x); has1 = true; }
    }
    for (size_t si = 0; si < e->dec_stages.size(); ++si) {
        auto& S = e->dec_stages[si];
        Act2 up = run_convtr2d(e, cx, S.resample, e->dec_up_phases[si], a0, has1 ? &a1 : nullptr, si + 1 == e->dec_stages.size(), e->halo2);
        Act2 sc, b3;
        run_resblocks2d(e, cx, S, up, nullptr, &sc, &b3);
        a0 = sc; a1 = b3; has1 = true;
    }
    Act2 last = run_conv2d(e, cx, e->dec2_last, a0, &a1, 1, 0);                     // [B][F][3][Tp2] raw + GroupNorm(1, 3) affine
    run_synthesis_2d(e, cx, last, scale, out_len, wav);
}

int total_hop(const fc_engine* e) {
    int h = e->arch.model_type == 1 ? e->arch.stft_hop : 1;
    for (int i = 0; i < e->arch.n_ratios; ++i) h *= e->arch.ratios[i];
    return h;
}

int decoded_samples(const fc_engine* e, int Tf) {
    if (e->arch.model_type != 1) return Tf * total_hop(e);
    int tp = Tf;
    for (int i = 0; i < e->arch.n_ratios; ++i) tp *= e->arch.ratios[i];
    return e->arch.stft_hop * (tp - 1);                                   // torch.istft, center = True
}

int frames_for(const fc_engine* e, int T) {
    if (e->arch.model_type == 1) T = stft_frames(e, T);
    for (int i = e->arch.n_ratios - 1; i >= 0; --i) T = ceil_div_i(T, e->arch.ratios[i]);
    return T;
}

// ---- per-row stage counts (fc_engine_set_row_nq) ----------------------------------------------------
// the device table of the calls that quantise or look up codes, or null when none is set
const int* row_nq_table(const fc_engine* e) { return e->row_nq.empty() ? nullptr : e->row_nq_dev; }

// The rule of a call made while a table is set, checked BEFORE its first launch: as many rows as the table has, and n_q (the first
// dimension of the codes) no smaller than any entry.
int row_nq_check(const fc_engine* e, int rows, int n_q) {
    if (e->row_nq.empty()) return 0;
    if ((int)e->row_nq.size() != rows)
        return fail("per-row stage counts are set for " + std::to_string(e->row_nq.size()) + " rows (fc_engine_set_row_nq); this call has " +
                    std::to_string(rows) + " (clear them with a NULL table)");
    for (size_t b = 0; b < e->row_nq.size(); ++b)
        if (e->row_nq[b] > n_q)
            return fail("n_q is the cap of the per-row stage counts (fc_engine_set_row_nq): row " + std::to_string(b) + " asks for " +
                        std::to_string(e->row_nq[b]) + " stages, n_q is " + std::to_string(n_q));
    return 0;
}

// ---- what a call is refused for while counts are set, checked BEFORE its first launch ------------------
// An encode (`who`: the entry point) under the per-row table (fc_engine_set_row_nq) and the rate (fc_engine_set_rate, _frames).  An
// offline call: as many rows as the rate has, and the floor no larger than n_q or any row's cap.  A session push takes no rate.
// A noise floor (fc_engine_set_floor) is for the pushes (`floor_ok`: a session push, or the per-op hook): as many rows as the floor has, and
// min_nq no larger than n_q or any row's cap.
int counts_check_encode(const fc_engine* e, const char* who, int B, int n_q, bool session, bool floor_ok = false) {
    if (row_nq_check(e, B, n_q)) return 1;
    if (e->floor.on()) {
        const fc_engine::Floor& f = e->floor;
        if (!(session || floor_ok))
            return fail(std::string(who) + ": a noise floor is set (fc_engine_set_floor): a stage count per push by a noise floor is for session pushes only; "
                        "clear it with NULL floors");
        if (e->rate.on())
            return fail(std::string(who) + ": a noise floor (fc_engine_set_floor) and a rate (fc_engine_set_rate) are both set; clear one of them");
        if ((int)f.floor.size() != B)
            return fail("a noise floor is set for " + std::to_string(f.floor.size()) + " rows (fc_engine_set_floor); this push has " + std::to_string(B) +
                        " (clear it with NULL floors)");
        if (f.min_nq > n_q)
            return fail("fc_engine_set_floor: min_nq = " + std::to_string(f.min_nq) + " lies above n_q = " + std::to_string(n_q));
        for (size_t b = 0; b < e->row_nq.size(); ++b)
            if (f.min_nq > e->row_nq[b])
                return fail("fc_engine_set_floor: min_nq = " + std::to_string(f.min_nq) + " lies above the cap of row " + std::to_string(b) + " (" +
                            std::to_string(e->row_nq[b]) + " stages, fc_engine_set_row_nq)");
        if (floor_ok && !session && f.nq_frames_out && !f.stage_err_out)
            return fail(std::string(who) + ": the hook has no workspace: fc_engine_set_floor_form with stage_errors_out");
        if (floor_ok && !session && !f.nq_frames_out && (!f.row_err_out || !f.stage_err_out))
            return fail(std::string(who) + ": the hook has no workspace: fc_engine_set_floor_form with row_errors_out and stage_errors_out");
        return 0;
    }
    if (!e->rate.on()) return 0;
    if (session) {
        if (e->rate.frames)
            return fail(std::string(who) + ": frame mode is set (fc_engine_set_rate_frames): a stage count per frame by target SNR is for offline calls only; "
                        "clear it with NULL ratios (fc_engine_set_rate)");
        return fail(std::string(who) + ": a rate is set (fc_engine_set_rate): a stage count per row by target SNR is for offline calls only; clear it with NULL ratios");
    }
    if ((int)e->rate.ratio.size() != B)
        return fail("a rate is set for " + std::to_string(e->rate.ratio.size()) + " rows (fc_engine_set_rate); this call has " + std::to_string(B) +
                    " (clear it with NULL ratios)");
    if (e->rate.min_nq > n_q)
        return fail("fc_engine_set_rate: min_nq = " + std::to_string(e->rate.min_nq) + " lies above n_q = " + std::to_string(n_q));
    for (size_t b = 0; b < e->row_nq.size(); ++b)
        if (e->rate.min_nq > e->row_nq[b])
            return fail("fc_engine_set_rate: min_nq = " + std::to_string(e->rate.min_nq) + " lies above the cap of row " + std::to_string(b) + " (" +
                        std::to_string(e->row_nq[b]) + " stages, fc_engine_set_row_nq)");
    return 0;
}

// A decode from codes (`who`: the entry point) under the per-row table and the table per frame (fc_engine_set_frame_nq).  An offline call:
// the frame table's B and Tf, and not both tables.  A session push takes no frame table.
int counts_check_decode(const fc_engine* e, const char* who, int B, int Tf, int n_q, bool session) {
    if (row_nq_check(e, B, n_q)) return 1;
    if (e->push_nq.table) {     // fc_engine_set_push_frame_nq: the same table for the decode pushes of sessions, and for them alone
        if (!session)
            return fail(std::string(who) + ": a stage count per frame of a push is set (fc_engine_set_push_frame_nq): it is for session decode pushes only; "
                        "clear it with a NULL table");
        if (!e->row_nq.empty())
            return fail("a stage count per frame of a push (fc_engine_set_push_frame_nq) and per-row stage counts (fc_engine_set_row_nq) are both set; "
                        "clear one of them");
        if (e->push_nq.B != B || e->push_nq.Tf != Tf)
            return fail("a stage count per frame is set for [" + std::to_string(e->push_nq.B) + "][" + std::to_string(e->push_nq.Tf) +
                        "] frames (fc_engine_set_push_frame_nq); this push has [" + std::to_string(B) + "][" + std::to_string(Tf) +
                        "] (clear it with a NULL table)");
    }
    if (!e->frame_nq.table) return 0;
    if (session)
        return fail(std::string(who) + ": a stage count per frame is set (fc_engine_set_frame_nq): it is for offline decode calls only; clear it with a NULL table");
    if (!e->row_nq.empty())
        return fail("a stage count per frame (fc_engine_set_frame_nq) and per-row stage counts (fc_engine_set_row_nq) are both set; clear one of them");
    if (e->frame_nq.B != B || e->frame_nq.Tf != Tf)
        return fail("a stage count per frame is set for [" + std::to_string(e->frame_nq.B) + "][" + std::to_string(e->frame_nq.Tf) +
                    "] frames (fc_engine_set_frame_nq); this call has [" + std::to_string(B) + "][" + std::to_string(Tf) + "] (clear it with a NULL table)");
    return 0;
}

// ---- everything behind the greedy encode of a quantiser call, stated once ---------------------------------
// The search over the stages (width > 1), then -- under a rate (fc_engine_set_rate; csrc/rvq_rate_kernels.h) -- the stage errors, the
// row sums, the pick per row or per frame, the sum from the first k codes and the zeros behind them.
struct RvqTail {
    const float* x = nullptr;                   // the quantiser's input rows [B Tf][Dc]
    int64_t* codes = nullptr;                   // [n_q][B Tf]: the greedy codes, rewritten in place
    int B = 0, Tf = 0, n_q = 0, width = 1;
    float *quant = nullptr, *quant_bdt = nullptr, *subq = nullptr;      // what a sum writes; each may be null
    int64_t* paths = nullptr; float* errors = nullptr;                  // of the search, or null
    bool beam_sum = true, rate_sum = true;      // the sum behind the search, and behind the pick
    const fc::RagLen* rate_rows = nullptr;      // the rate applies: the frames of every row (null: it does not)
    const fc::RagLen* floor_rows = nullptr;     // the noise floor applies (a session push, the hook): the frames every row has in the push
    float* serr = nullptr; double* rerr = nullptr;                      // stage errors [n_q + 1][B Tf], row errors [B][n_q + 1]
};
// launch(what, flops, enqueue): how the caller makes a launch (flops: booked to the search's kernel class; 0 for every other launch)
template <typename Launch>
void rvq_after_greedy(const fc_engine* e, const RvqTail& a, hipStream_t st, Launch&& launch) {
    const int N = a.B * a.Tf, Dc = e->cdim(), K = e->arch.codebook_size;
    const int* caps = row_nq_table(e);                 // indexed by batch row (a slot push: by slot)
    auto sum = [&](const char* what, const fc::StageCounts& k) {
        launch(what, 0.0, [&] { return fc::launch_rvq_codes_sum(a.codes, N, Dc, K, a.n_q, e->cb, a.quant, a.quant_bdt, a.subq, a.Tf, k, st); });
    };
    if (a.width > 1) {      // the search rewrites the greedy codes in place; everything else from the final codes
        launch("rvq beam", 2.0 * a.B * a.Tf * (double)a.n_q * K * Dc * a.width, [&] {
            return fc::launch_rvq_beam(a.x, N, Dc, K, a.n_q, a.width, e->cb, e->cb_frag, e->enorm, a.codes, a.paths, a.errors, a.Tf, st, caps);
        });
        fc::StageCounts k; k.rows = caps;
        if (a.beam_sum && !a.floor_rows) sum("rvq beam sum", k);        // under a floor the pick's sum follows at once
    }
    if (a.floor_rows && e->floor.nq_frames_out) {       // fc_engine_set_floor_frames (the push frame rule): one fused launch of any width, or its chain
        const fc_engine::Floor& f = e->floor;
        if (!f.chain) {
            launch("rvq push floor frames", 0.0, [&] {
                return fc::launch_rvq_push_floor_frames(a.x, a.codes, a.B, a.Tf, Dc, K, a.n_q, e->cb, caps, *a.floor_rows, f.floor_dev, f.min_nq,
                                                        f.nq_frames_out, a.quant, a.quant_bdt, a.subq, f.stage_err_out, st);
            });
            return;
        }
        launch("rvq stage errors", 0.0, [&] { return fc::launch_rvq_stage_errors(a.x, a.codes, N, Dc, K, a.n_q, e->cb, a.serr, a.Tf, caps, *a.floor_rows, st); });
        launch("rvq floor frames", 0.0, [&] {
            return fc::launch_rvq_floor_frames(a.serr, a.B, a.Tf, a.n_q, caps, *a.floor_rows, f.floor_dev, f.min_nq, f.nq_frames_out, st);
        });
        fc::StageCounts k; k.frames = f.nq_frames_out;
        sum("rvq floor frame sum", k);
        launch("rvq floor frame zero codes", 0.0, [&] { return fc::launch_rvq_rate_zero_codes(a.codes, N, a.Tf, a.n_q, k, st); });
        return;
    }
    if (a.floor_rows) {     // fc_engine_set_floor (the push rule): one fused launch, or its chain for a push wider than the launch takes
        const fc_engine::Floor& f = e->floor;
        if (!f.chain && fc::rvq_push_floor_fits(a.Tf, Dc, a.n_q)) {
            launch("rvq push floor", 0.0, [&] {
                return fc::launch_rvq_push_floor(a.x, a.codes, a.B, a.Tf, Dc, K, a.n_q, e->cb, caps, *a.floor_rows, f.floor_dev, f.min_nq, f.n_q_out,
                                                 a.quant, a.quant_bdt, a.subq, f.row_err_out, f.stage_err_out, st);
            });
            return;
        }
        launch("rvq stage errors", 0.0, [&] { return fc::launch_rvq_stage_errors(a.x, a.codes, N, Dc, K, a.n_q, e->cb, a.serr, a.Tf, caps, *a.floor_rows, st); });
        launch("rvq floor rows", 0.0, [&] {
            return fc::launch_rvq_rate_rows(a.serr, a.B, a.Tf, a.n_q, caps, *a.floor_rows, nullptr, f.min_nq, nullptr, f.n_q_out, a.rerr, st, f.floor_dev);
        });
        fc::StageCounts k; k.rows = f.n_q_out;
        sum("rvq floor sum", k);
        launch("rvq floor zero codes", 0.0, [&] { return fc::launch_rvq_rate_zero_codes(a.codes, N, a.Tf, a.n_q, k, st); });
        return;
    }
    if (!a.rate_rows) return;
    const fc_engine::Rate& r = e->rate;
    launch("rvq stage errors", 0.0, [&] { return fc::launch_rvq_stage_errors(a.x, a.codes, N, Dc, K, a.n_q, e->cb, a.serr, a.Tf, caps, *a.rate_rows, st); });
    auto row_sums = [&](int min_nq, int* k_table, int32_t* n_q_out) {
        launch("rvq rate rows", 0.0, [&] {
            return fc::launch_rvq_rate_rows(a.serr, a.B, a.Tf, a.n_q, caps, *a.rate_rows, r.ratio_dev, min_nq, k_table, n_q_out, a.rerr, st);
        });
    };
    fc::StageCounts k;                                  // the chosen counts
    if (r.frames) {         // fc_engine_set_rate_frames: the row sums alone, then a count per frame
        row_sums(1, nullptr, nullptr);
        launch("rvq rate frames", 0.0, [&] {
            return fc::launch_rvq_rate_frames(a.serr, a.rerr, a.B, a.Tf, a.n_q, caps, *a.rate_rows, r.ratio_dev, r.min_nq, r.nq_frames_out, r.n_q_out,
                                              r.n_codes_out, r.achieved_out, st);
        });
        k.frames = r.nq_frames_out;
    } else {                // a count per row, into the engine's own table (NOT row_nq_dev, which holds the caps)
        row_sums(r.min_nq, r.k_dev, r.n_q_out);
        k.rows = r.k_dev;
    }
    if (a.rate_sum) sum(r.frames ? "rvq frame sum" : "rvq rate sum", k);
    launch(r.frames ? "rvq frame zero codes" : "rvq rate zero codes", 0.0, [&] { return fc::launch_rvq_rate_zero_codes(a.codes, N, a.Tf, a.n_q, k, st); });
}

// ---- composite paths (each usable in dry mode for workspace sizing / work accounting) ---------------
int do_quantize(fc_engine* e, Ctx& cx, const Act& last, int Tf, int n_q, int64_t* codes, float* quantized, float* sub_quants, float* enc_out,
                float** quant_bdt_out, const fc::RagLen* offline_rows = nullptr, const fc::RagLen* push_rows = nullptr);
int do_encode(fc_engine* e, Ctx& cx, const float* wav, int T, int n_q, int64_t* codes, float* quantized,
              float* sub_quants, float* scale, float* enc_out, float** quant_bdt_out, const Pass& p = Pass()) {
    const int B = cx.B, D = e->arch.dimension, Tf = frames_for(e, T);
    float* sc = nullptr;
    if (e->arch.audio_normalize) {
        sc = scale ? scale : cx.alloc<float>(B);
        cx.launch("volume", "", [&] {
            return fc::launch_volume(wav, B, e->audio_ch(), T, sc, cx.st, p.kind == Pass::Ragged ? p.lengths : nullptr);
        });
    }
    fc::Src s; s.ptr = wav; s.div = sc; s.used = e->arch.audio_normalize ? 3 : 1;
    Act last = e->arch.model_type == 1 ? run_encoder_2d(e, cx, wav, T, sc) : run_encoder(e, cx, p, s, T);
    // an offline call (whole batch width, or a ragged pass with the frames of every row): the one place the rate control applies
    fc::RagLen rows;
    if (p.kind == Pass::Ragged) { rows.lens = p.lengths; rows.div = total_hop(e); }
    return do_quantize(e, cx, last, Tf, n_q, codes, quantized, sub_quants, enc_out, quant_bdt_out, &rows);
}

// the quantiser behind the encoder's last conv (per frame: the offline call and a streaming push share it)
// offline_rows (an offline call; null in a session push): the frames of every row, for the rate control (fc_engine_set_rate)
// push_rows (a session push; null in an offline call): the frames every row has in the push, for the noise floor (fc_engine_set_floor)
int do_quantize(fc_engine* e, Ctx& cx, const Act& last, int Tf, int n_q, int64_t* codes, float* quantized, float* sub_quants, float* enc_out,
                float** quant_bdt_out, const fc::RagLen* offline_rows, const fc::RagLen* push_rows) {
    const int B = cx.B, D = e->arch.dimension;
    const int Dc = e->cdim();
    const bool ranged = e->arch.codec_range > 0.f;
    // encoder output rows [B][Tf][D] (seanet_encoder.py:175) with the last GroupNorm applied: the quantiser's input, or asked for
    const bool emb_rows = enc_out || !(e->q_proj || ranged);
    float* emb = enc_out ? enc_out : emb_rows ? cx.alloc<float>((size_t)B * Tf * D) : nullptr;
    // quantiser input rows [B*Tf][Dc]: the encoder output itself, or input_proj(...) / tanh(...) * range of it (costume_quantizer.py:84-87)
    Act pj;
    if (e->q_proj) pj = run_conv(e, cx, e->q_in, src_of(last), fc::Src(), 0, Tf);
    float* xq = (e->q_proj || ranged) ? cx.alloc<float>((size_t)B * Tf * Dc) : emb;
    float* quant_c = e->q_proj ? cx.alloc<float>((size_t)B * Tf * Dc) : quantized;       // quantised rows in codebook space
    float* qbdt_c = cx.alloc<float>((size_t)B * Dc * Tf);
    // quantizer_conf.q0_ds_ratio > 1 (ddp_core_vq.py:396-404): stage 0 of frame t quantises frame q0_source_frame(t, Tf) (kernels.h)
    const bool q0 = e->arch.q0_ds_ratio > 1;
    int* q0map = q0 ? cx.alloc<int>((size_t)B * Tf) : nullptr;
    const double rvq_fl = 2.0 * B * Tf * (double)n_q * e->arch.codebook_size * Dc;
    cx.rvq_flops += rvq_fl;
    if (!cx.dry && last.T != Tf) cx.fail("internal: frame count mismatch");
    const int* nq_rows = row_nq_table(e);              // indexed by batch row (a slot push: by slot)
    if (!cx.dry && nq_rows && (int)e->row_nq.size() != B) cx.fail("internal: per-row stage counts of another batch width");
    if (emb_rows)
        cx.launch("combine", "", [&] { return fc::launch_combine(src_of(last), fc::Src(), 0, 1.f, nullptr, B, D, Tf, Tf, emb, (long long)Tf * D, 1, D, cx.st); });
    if (e->q_proj)
        cx.launch("combine", "", [&] { return fc::launch_combine(src_of(pj), fc::Src(), 0, 1.f, nullptr, B, Dc, Tf, Tf, xq, (long long)Tf * Dc, 1, Dc, cx.st); });
    else if (ranged)
        cx.launch("combine", "", [&] { return fc::launch_combine(src_of(last), fc::Src(), 0, 1.f, nullptr, B, D, Tf, Tf, xq, (long long)Tf * D, 1, D, cx.st); });
    if (ranged) cx.launch("tanh", "", [&] { return fc::launch_tanh_range(xq, (size_t)B * Tf * Dc, e->arch.codec_range, cx.st); });
    if (q0) {
        if (!cx.dry && Tf < 2) cx.fail("quantizer_conf.q0_ds_ratio > 1 needs at least 2 frames (the reference's F.interpolate(size=[Tf // 2]) raises on 0)");
        cx.launch("q0 map", "", [&] { return fc::launch_q0_map(q0map, B, Tf, cx.st); });
    }
    cx.launch("rvq", "", [] { return kRvqClass; }, rvq_fl, 0.0, [&] {
        return fc::launch_rvq_encode(xq, B * Tf, Dc, e->arch.codebook_size, n_q, e->cb, e->cb_frag, e->enorm, codes, quant_c, qbdt_c, sub_quants, Tf, cx.st, q0map,
                                     nq_rows);
    });
    // fc_engine_set_rvq_beam and fc_engine_set_rate: everything behind the greedy codes.  A dry pass always counts the rate's two
    // buffers: a workspace is sized before anybody knows whether a rate will be set.
    RvqTail tail;
    tail.x = xq; tail.codes = codes; tail.B = B; tail.Tf = Tf; tail.n_q = n_q; tail.width = e->rvq_beam;
    tail.quant = quant_c; tail.quant_bdt = qbdt_c; tail.subq = sub_quants;
    if (offline_rows && (cx.dry || e->rate.on())) {
        tail.serr = cx.alloc<float>((size_t)(n_q + 1) * B * Tf);
        tail.rerr = cx.alloc<double>((size_t)B * (n_q + 1));
        if (e->rate.on()) {
            if (!cx.dry && (int)e->rate.ratio.size() != B) cx.fail("internal: a rate of another batch width");
            if (e->rate.stage_err_out) tail.serr = e->rate.stage_err_out;
            if (e->rate.row_err_out) tail.rerr = e->rate.row_err_out;
            tail.rate_rows = offline_rows;
        }
    }
    // fc_engine_set_floor: a push needs the two buffers in the chain form alone (a push wider than the fused launch takes, or the form
    // forced); a dry pass counts them for the session's widest push
    if (push_rows && (cx.dry || e->floor.on())) {
        if (!cx.dry && (int)e->floor.floor.size() != B) cx.fail("internal: a noise floor of another batch width");
        if (cx.dry || e->floor.chain || (!e->floor.nq_frames_out && !fc::rvq_push_floor_fits(Tf, Dc, n_q))) {
            tail.serr = cx.alloc<float>((size_t)(n_q + 1) * B * Tf);
            tail.rerr = cx.alloc<double>((size_t)B * (n_q + 1));
        }
        if (e->floor.on()) tail.floor_rows = push_rows;
    }
    rvq_after_greedy(e, tail, cx.st, [&](const char* what, double flops, auto&& enqueue) {
        if (flops > 0.0) cx.launch(what, "", [] { return kRvqBeamClass; }, flops, 0.0, enqueue);
        else cx.launch(what, "", enqueue);
    });
    float* qbdt = qbdt_c;
    if (e->q_proj) {       // output_proj (costume_quantizer.py:92-94): decoder input [B][D][Tf] and the returned embeddings [B][Tf][D]
        fc::Src qs; qs.ptr = qbdt_c; qs.used = 1;
        Act qo = run_conv(e, cx, e->q_out, qs, fc::Src(), 0, Tf);
        qbdt = qo.raw;
        if (quantized)
            cx.launch("combine", "", [&] { return fc::launch_combine(src_of(qo), fc::Src(), 0, 1.f, nullptr, B, D, Tf, Tf, quantized, (long long)Tf * D, 1, D, cx.st); });
    }
    if (quant_bdt_out) *quant_bdt_out = qbdt;
    return cx.err;
}

// The tail of every decode pass, into the caller's wav [B][C][out_len]: the final GroupNorm apply (decoder.model.N.conv.norm has C = audio
// channels), x scale (codec_basic.py:406-407), trim (:711); `valid` (rows that end at their own length): zeros behind every row's samples
int finish_decode(fc_engine* e, Ctx& cx, const Act& last, const float* scale, int out_len, float* wav, const fc::RagLen* valid) {
    const int C = e->audio_ch();
    cx.launch("combine", "", [&] {
        return fc::launch_combine(src_of(last), fc::Src(), 0, 1.f, scale, cx.B, C, last.T, out_len, wav, (long long)C * out_len, out_len, 1, cx.st);
    });
    if (valid) cx.launch("ragged mask", "wav", [&] { return fc::launch_ragged_mask_f32(wav, 1, cx.B, C, out_len, 1, *valid, cx.st); });
    return cx.err;
}

int do_decode(fc_engine* e, Ctx& cx, const float* z_bdt, int Tf, const float* scale, int out_len, float* wav, const Pass& p = Pass(),
              const fc::RagLen* valid = nullptr) {
    if (e->arch.model_type == 1) {
        run_decoder_2d(e, cx, z_bdt, Tf, scale, out_len, wav);
        return cx.err;
    }
    Act last = run_decoder(e, cx, p, z_bdt, Tf);
    if (!cx.dry && out_len > last.T) cx.fail("out_len exceeds Tf*hop");
    return finish_decode(e, cx, last, scale, out_len, wav, valid);
}

// Embeddings to decoder input (the decode_emb calls): emb [B][Tf][D] into z [B][D][Tf].  What lies behind a row's frames in a ragged
// call or a slot push is never read (dec_first is staged).
float* decoder_input_emb(fc_engine* e, Ctx& cx, const float* emb, int Tf) {
    const int D = e->arch.dimension;
    float* z = cx.alloc<float>((size_t)cx.B * D * Tf);
    cx.launch("transpose", "emb", [&] { return fc::launch_transpose_btd(emb, cx.B, Tf, D, z, cx.st); });
    return z;
}

// Codes to decoder input (the decode_codes calls): the summed code vectors of `codes` [B][Tf][n_q] into [B][Dc][Tf], then
// CostumeQuantizer.decode's output_proj on them (costume_quantizer.py:114-119).  Returns the decoder's input [B][D][Tf]; emb_out
// (optional) gets the embeddings [B][Tf][D].  `rows` (null, or the frames of every row of a ragged call / slot push): the tokens behind a
// row's frames are the caller's garbage, so a masked copy is looked up (none of them is read, or reported as out of range) and emb_out is
// masked too.  `either` (workspace sizing): the first buffer as wide as the wider of the two decode calls needs it.
// `frame_nq` (an offline call under fc_engine_set_frame_nq, else null): a stage count per frame [B][Tf], by csrc/rvq_rate_kernels.h.
float* decoder_input_codes(fc_engine* e, Ctx& cx, const int64_t* codes, int Tf, int n_q, float* emb_out, const fc::RagLen* rows, bool either = false,
                           const int32_t* frame_nq = nullptr) {
    const int B = cx.B, D = e->arch.dimension, Dc = e->cdim();
    if (rows) {
        int64_t* masked = cx.alloc<int64_t>((size_t)B * Tf * n_q);
        cx.launch("copy", "tokens", [&] { return hipMemcpyAsync(masked, codes, (size_t)B * Tf * n_q * sizeof(int64_t), hipMemcpyDeviceToDevice, cx.st); });
        cx.launch("ragged mask", "tokens", [&] { return fc::launch_ragged_mask_i64(masked, 1, B, 1, Tf, n_q, *rows, cx.st); });
        codes = masked;
    }
    float* z = cx.alloc<float>((size_t)B * (either ? std::max(D, Dc) : Dc) * Tf);
    fc::StageCounts k;                                  // a frame's codes behind its count are not read
    k.rows = row_nq_table(e); k.frames = frame_nq;
    if (!cx.dry && k.rows && (int)e->row_nq.size() != B) cx.fail("internal: per-row stage counts of another batch width");
    cx.launch("rvq decode", "", [&] {       // a count per frame also counts 0 behind a row's frames, whatever the caller's table holds there
        return fc::launch_rvq_decode(codes, B, Tf, n_q, Dc, e->arch.codebook_size, e->cb, e->q_proj ? nullptr : emb_out, z, e->status_dev, k,
                                     frame_nq && rows ? *rows : fc::RagLen(), cx.st);
    });
    if (e->q_proj) {
        fc::Src qs; qs.ptr = z; qs.used = 1;
        Act qo = run_conv(e, cx, e->q_out, qs, fc::Src(), 0, Tf);
        if (emb_out)
            cx.launch("combine", "", [&] { return fc::launch_combine(src_of(qo), fc::Src(), 0, 1.f, nullptr, B, D, Tf, Tf, emb_out, (long long)Tf * D, 1, D, cx.st); });
        z = qo.raw;
    }
    if (rows && emb_out) cx.launch("ragged mask", "emb_out", [&] { return fc::launch_ragged_mask_f32(emb_out, 1, B, 1, Tf, D, *rows, cx.st); });
    return z;
}

// Deferred device-side failures of EARLIER calls (kernels cannot return a status): reported once, then cleared.
int consume_status(fc_engine* e) {
    if (!e->status_host) return 0;
    if (e->status_host[FC_STATUS_LSTM_TIMEOUT]) {
        e->status_host[FC_STATUS_LSTM_TIMEOUT] = 0;
        e->lstm_persist_ok = false;
        return fail("a previous call's persistent LSTM kernel timed out at its grid barrier (its workgroups were not all co-resident: "
                    "GPU shared with another process / stream, or CUs masked); that call's outputs were NaN-poisoned and are invalid. "
                    "This engine now uses the per-step LSTM launches (same results); set FC_LSTM_PERSIST=0 for shared-GPU deployments");
    }
    if (e->status_host[FC_STATUS_BAD_CODE]) {
        e->status_host[FC_STATUS_BAD_CODE] = 0;
        return fail("a previous decode call was given code indices outside [0, codebook_size) (the reference's F.embedding raises, "
                    "ddp_core_vq.py:191); they were clamped, the decoded audio of that call is not meaningful");
    }
    if (e->status_host[FC_STATUS_BAD_LENGTH]) {
        e->status_host[FC_STATUS_BAD_LENGTH] = 0;
        return fail("a previous length-aware call was given a row length outside [1, Tmax] (speech_lengths / token_lengths); it was clamped, "
                    "that row's outputs of that call are not meaningful");
    }
    return 0;
}

int check_ready(fc_engine* e) {
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    return consume_status(e);
}


// ---- streaming session ---------------------------------------------------------------------------------------------------------
// The reference has no streaming code; what a session must reproduce is the OFFLINE callable on the concatenation of its pushes:
// Encodec.inference_encoding (codec_basic.py:720-764) for fc_stream_encode, Encodec.inference_decoding / inference_decoding_emb
// (:766-836) for the two decode calls.  A causal SConv1d (conv.py:243-261) looks at padding_total columns to its left and at nothing to
// its right except the last call's extra_padding, so a chunk is a plain conv without padding over [carry | chunk] where the carry is the
// last padding_total columns of the layer's input so far.  The one place the offline call is NOT causal is the very start: pad1d reflects
// (pad_mode "reflect", the only mode the configs use), i.e. the left padding of EVERY layer is columns 1..padding_total of its own input.
// A session therefore takes a first push long enough to hold that reflection at every layer (fc_stream_min_first; the Python session
// gathers short pushes until it has that much) and stages the reflection instead of a carry there.
inline int stream_pt(const ConvLayer& L) { return L.transposed ? 1 : (L.k - 1) * L.dil - (L.stride - 1); }

// why this engine cannot stream, or null.  Each reason names the configuration key.
const char* stream_refusal(const fc_engine* e, int max_frames = 0) {
    const fc_arch& a = e->arch;
    if (a.model_type != 0) return "streaming is not available for model: freq_codec (the STFT frames overlap; time-domain codec only)";
    if (!a.causal) return "streaming needs encoder_conf.causal / decoder_conf.causal: true (a non-causal net looks ahead at every layer)";
    if (a.lstm_layers > 0 && a.seq_model == 1 && max_frames <= 0)
        return "streaming is not available for seq_model: transformer (it needs a key / value cache across pushes: fc_seqstream_create takes its bound, max_frames)";
    if (a.q0_ds_ratio > 1) return "streaming is not available for quantizer_conf.q0_ds_ratio > 1 (the half-rate first stage looks across frame pairs)";
    if (max_frames > 0 && !(a.lstm_layers > 0 && a.seq_model == 1))
        return "max_frames bounds the key / value cache of seq_model: transformer; this net has no transformer bottleneck (fc_stream_create opens its session)";
    return nullptr;
}

void stream_layout(fc_engine* e, int B, Session* S) {
    size_t off = ((size_t)B + 63) & ~(size_t)63;      // scale [B]
    const int hop = total_hop(e);
    int enc_min = hop, dec_min = 1;
    for_each_conv(e, [&](const ConvVisit& v) {
        const ConvLayer& L = v.L;
        const int pt = stream_pt(L);
        if (!carries_context(v.role) || pt <= 0) return;
        S->carry[&L] = off;
        off += ((size_t)2 * B * L.cin * pt + 63) & ~(size_t)63;
        if (L.transposed) return;                      // zero left context at the start: no reflection to hold
        if (!v.dec) enc_min = std::max(enc_min, (pt + 1) * v.rate);
        else dec_min = std::max(dec_min, ceil_div_i(pt + 1, v.rate));
    });
    const size_t L = (size_t)e->arch.lstm_layers;
    S->enc_lstm_off = off; off += 3 * L * B * e->enc_lstm.H;
    S->dec_lstm_off = off; off += 3 * L * B * e->dec_lstm.H;
    S->carried_floats = off;
    if (S->max_frames > 0) {                          // the key / value caches: per block K then V, [B][C][F] each
        const size_t F = (size_t)fc::seq_cache_pitch(S->max_frames);
        off = (off + 63) & ~(size_t)63;
        S->enc_kv_off = off; off += e->enc_tf.layers.size() * 2 * B * e->enc_tf.C * F;
        S->dec_kv_off = off; off += e->dec_tf.layers.size() * 2 * B * e->dec_tf.C * F;
    }
    S->state_floats = off;
    S->enc_min_first = ceil_div_i(enc_min, hop) * hop;
    S->dec_min_first = dec_min;
}

// the carry of layer L inside the session state: a push reads the one at the parity of the n pushes its side has taken and writes the other
struct CarryPair { const float* in = nullptr; float* out = nullptr; };
CarryPair carry_pair(const Session& s, const ConvLayer& L, int n) {
    CarryPair c;
    const int pt = stream_pt(L);
    if (pt <= 0) return c;
    float* pair = s.state + s.carry.at(&L);
    const size_t half = (size_t)s.B * L.cin * pt;
    c.in = pair + (size_t)(n & 1) * half;
    c.out = pair + (size_t)(~n & 1) * half;
    return c;
}

// the session's LSTM state of one side (run_lstm's `carried`)
float* lstm_state(const Session& s, bool dec) { return s.state + (dec ? s.dec_lstm_off : s.enc_lstm_off); }

// the session's key / value cache of one side and the frames it holds (run_transformer's `kv`; a slot session's rows have their own
// positions, which the caller adds).  The sizing pass (no state yet) runs at pos 0: no size of a push depends on pos.
TfCache tf_cache(const Session& s, bool dec, int pos) {
    TfCache c;
    c.base = s.state ? s.state + (dec ? s.dec_kv_off : s.enc_kv_off) : nullptr;
    c.pos = pos;
    c.F = fc::seq_cache_pitch(s.max_frames);
    return c;
}

// The segment list of the session's slot record, in the order slots_kernels.h states: what stream_layout gave one row, walked again.
// Called once, at create, behind stream_layout; the table goes to device memory with room for one call's named slots behind it.
int record_layout(fc_engine* e, Session* S) {
    Session::Record& R = S->rec;
    const int B = S->B;
    uint32_t fp = fc::kSlotRecordLayoutSeed;
    auto plain = [&](int kind, int side, size_t st_off, size_t half, int len) {
        fc::SlotSeg g{};
        g.st_off = (long long)st_off; g.half = (long long)half; g.rec_fixed = (long long)R.fixed;
        g.slot_stride = len; g.rows = 1; g.len = len; g.st_pitch = len; g.side = side; g.enc_cols = R.enc_cols; g.dec_cols = R.dec_cols;
        R.segs.push_back(g);
        R.fixed += (size_t)len;
        R.max_len = std::max(R.max_len, len);
        fp = fc::slot_record_layout_step(fp, kind, side, len);
    };
    plain(fc::kSegScale, -1, 0, 0, 1);
    const int F = fc::seq_cache_pitch(S->max_frames);
    for (int side = 0; side < 2; ++side) {
        const bool dec = side == 1;
        for_each_conv(e, [&](const ConvVisit& v) {
            const int pt = stream_pt(v.L);
            if (v.dec != dec || !carries_context(v.role) || pt <= 0) return;
            plain(fc::kSegCarry, side, S->carry.at(&v.L), (size_t)B * v.L.cin * pt, v.L.cin * pt);
        });
        const LstmBlock& lb = dec ? e->dec_lstm : e->enc_lstm;
        const size_t lstm = dec ? S->dec_lstm_off : S->enc_lstm_off, BH = (size_t)B * lb.H, L = (size_t)e->arch.lstm_layers;
        for (size_t l = 0; lb.H > 0 && l < L; ++l) {        // h [L][2][B][H], the half at parity 1; then c [L][B][H]
            plain(fc::kSegH, side, lstm + (2 * l + 1) * BH, 0, lb.H);
            plain(fc::kSegC, side, lstm + (2 * L + l) * BH, 0, lb.H);
        }
        if (S->max_frames <= 0) continue;
        const TfBlock& tb = dec ? e->dec_tf : e->enc_tf;
        const size_t kv = dec ? S->dec_kv_off : S->enc_kv_off, plane = (size_t)B * tb.C * F;
        for (size_t p = 0; p < 2 * tb.layers.size(); ++p) {  // per block K then V, [B][C][F] each
            fc::SlotSeg g{};
            g.st_off = (long long)(kv + p * plane); g.rec_fixed = (long long)R.fixed;
            g.slot_stride = tb.C * F; g.rows = tb.C; g.len = 0; g.st_pitch = F; g.side = side; g.enc_cols = R.enc_cols; g.dec_cols = R.dec_cols;
            R.segs.push_back(g);
            (dec ? R.dec_cols : R.enc_cols) += tb.C;
            R.max_rows = std::max(R.max_rows, tb.C);
            fp = fc::slot_record_layout_step(fp, (p & 1) ? fc::kSegV : fc::kSegK, side, tb.C);
        }
    }
    R.layout = (fp & ~1u) | (S->max_frames > 0 ? 1u : 0u);
    R.refs.resize(B);
    const size_t seg_bytes = (R.segs.size() * sizeof(fc::SlotSeg) + 15) & ~(size_t)15;
    char* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, seg_bytes + (size_t)B * sizeof(fc::SlotRef)));
    R.segs_dev = (fc::SlotSeg*)dev;
    R.refs_dev = (fc::SlotRef*)(dev + seg_bytes);
    HIP_TRY(hipMemcpy(R.segs_dev, R.segs.data(), R.segs.size() * sizeof(fc::SlotSeg), hipMemcpyHostToDevice));
    return 0;
}

// The GEMM behind every staging pass (stream_conv, slots_conv, ragged_conv): the layer's own kernel as a conv without padding over the
// staged buf [B][cin][Tp], which holds T new columns per row behind the left context.  A transposed layer computes `groups` tap pairs
// (group j = taps (x[j-1], x[j]) = staged columns (j, j + 1)) and drops trimL columns on the left.  With a GroupNorm behind it, which sees
// the UNTRIMMED output (conv.py:287-303), all groups * stride columns are `stored` at pitch `pitch` and `out` is the trimmed window into them.
struct Staged { Act out; float* stored = nullptr; int pitch = 0; };
Staged staged_conv(fc_engine* e, Ctx& cx, const ConvLayer& L, const float* buf, int Tp, int T, int groups, int trimL) {
    const int B = cx.B;
    ConvGeom geo;
    geo.padL = 0; geo.padR = 0;
    geo.Tout = L.transposed ? T * L.stride : (Tp - ((L.k - 1) * L.dil + 1)) / L.stride + 1;
    geo.count_T = geo.Tout;
    fc::ConvLaunch c = conv_launch_of(L, B, Tp, geo);
    c.s0.ptr = buf; c.s0.used = 1;
    c.alpha = e->arch.elu_alpha;
    c.pad_zero = 1;                                   // nothing is padded; columns past the row end of the last tile read as zero
    Staged r;
    r.out.C = L.cout; r.out.T = geo.Tout;
    r.pitch = geo.Tout;
    const bool untrimmed = L.transposed && L.has_norm;
    if (L.transposed) {
        c.Tout = groups; c.up_r = L.stride;
        if (untrimmed) {
            r.pitch = groups * L.stride;
            c.trimL = 0; c.Tfinal = r.pitch;
            r.out.ld = r.pitch;
        } else {
            c.trimL = trimL; c.Tfinal = geo.Tout;
        }
    } else {
        c.Tout = geo.Tout;
    }
    r.stored = cx.alloc<float>((size_t)B * L.cout * r.pitch);
    r.out.raw = untrimmed ? at(r.stored, trimL) : r.stored;
    c.out = r.stored; c.out_sB = (long long)L.cout * r.pitch; c.out_sM = r.pitch; c.out_sT = 1;
    const double fl = 2.0 * B * (double)L.M * L.cin * L.gk * c.Tout;
    const double by = 4.0 * B * ((double)L.cin * Tp + (double)L.cout * r.pitch);
    cx.conv_flops += fl; cx.conv_bytes += by;
    cx.conv_launch("conv", L.prefix.c_str(), [&] { return conv_class(c); }, fl, by, [&] { return fc::launch_conv(c, cx.st); });
    return r;
}

// One causal SConv1d / SConvTranspose1d of a push: the staging pass (prologue + left context + new carry), then the layer's own GEMM
// kernel as a conv without padding over what was staged.
Act stream_conv(fc_engine* e, Ctx& cx, const Pass& p, const ConvLayer& L, fc::Src s0, fc::Src s1, int elu, int Tc) {
    const int B = cx.B, pt = stream_pt(L);
    // the last push takes the reference's extra_padding (conv.py:57-64): earlier pushes are multiples of the stride, so the figure for the
    // whole utterance is the one conv_geom gives the last chunk
    const int extra = (!L.transposed && p.final) ? conv_geom(L, Tc).padR : 0;
    const int Tp = pt + Tc + extra;
    float* buf = cx.alloc<float>((size_t)B * L.cin * Tp);
    if (!cx.dry && !L.transposed && !p.final && Tc % L.stride != 0) cx.fail("internal: a chunk that is not a multiple of the stride (" + L.prefix + ")");
    if (!cx.dry && extra > pt + Tc - 1) cx.fail("internal: extra padding longer than the staged columns (" + L.prefix + ")");
    const CarryPair carry = carry_pair(*p.sess, L, p.n);
    fc::StreamStage g;
    g.s0 = s0; g.s1 = s1; g.elu = elu; g.alpha = e->arch.elu_alpha;
    g.B = B; g.C = L.cin; g.Tc = Tc; g.pt = pt; g.padR = extra; g.buf = buf;
    g.left = p.n > 0 ? 0 : (L.transposed ? 2 : 1);
    g.carry_in = carry.in; g.carry_out = carry.out;
    cx.launch("stream stage", L.prefix.c_str(), [] { return "stream_stage_kernel (streaming: prologue, left context and carry of a conv)"; }, 0.0,
              4.0 * B * L.cin * ((double)Tc * (s1.used ? 2 : 1) + Tp + 2.0 * pt), [&] { return fc::launch_stream_stage(g, cx.st); });
    return staged_conv(e, cx, L, buf, Tp, Tc, Tc, 0).out;
}

// One causal SConv1d / SConvTranspose1d of a push of a slot session: stream_conv with every row at its own place in its own utterance.
// The common staged width holds the widest row with the extra_padding of a last push, whether a row of this push ends or not.
Act slots_conv(fc_engine* e, Ctx& cx, const Pass& p, const ConvLayer& L, fc::Src s0, fc::Src s1, int elu, int T) {
    const int B = cx.B, pt = stream_pt(L);
    const int Tp = L.transposed ? 1 + T : pt + T + fc::ragged_extra(T, L.k, pt, L.stride);
    float* buf = cx.alloc<float>((size_t)B * L.cin * Tp);
    const CarryPair carry = carry_pair(*p.sess, L, p.n);
    fc::SlotsStage g;
    g.s0 = s0; g.s1 = s1; g.elu = elu; g.alpha = e->arch.elu_alpha;
    g.S = B; g.C = L.cin; g.T = T; g.Tp = Tp; g.k = L.k; g.pt = pt; g.stride = L.stride; g.transposed = L.transposed ? 1 : 0;
    g.len = ragged_len(cx, p); g.flags = p.flags; g.buf = buf;
    g.carry_in = carry.in; g.carry_out = carry.out;
    if (!cx.dry && p.host_push)
        for (int b = 0; b < B; ++b) {                 // what the kernel relies on, per row
            const int len = p.host_push[b];
            if (len <= 0) continue;
            const int n = fc::ragged_cols(len, g.len.div, g.len.mul, 0);
            const int extra = (!L.transposed && (p.host_push[B + b] & fc::kSlotFinal)) ? fc::ragged_extra(n, L.k, pt, L.stride) : 0;
            if (n > T || extra > pt + n - 1 || pt + n + extra > Tp) cx.fail("internal: a row of a slot push does not fit its staging (" + L.prefix + ")");
        }
    cx.launch("slots stage", L.prefix.c_str(), [] { return "slots_stage_kernel (slot session: prologue, per-row context, end and carry of a conv)"; }, 0.0,
              4.0 * B * L.cin * ((double)T * (s1.used ? 2 : 1) + Tp + 2.0 * pt), [&] { return fc::launch_slots_stage(g, cx.st); });
    return staged_conv(e, cx, L, buf, Tp, T, T, 0).out;
}

// a push of a streaming session; n: pushes this side has taken before this one (0 = the first push of an utterance)
Pass stream_pass(const fc_stream* S, int n, bool final) {
    Pass p;
    p.kind = Pass::Stream; p.sess = S; p.n = n; p.final = final;
    return p;
}

int stream_encode_pass(const fc_stream* S, Ctx& cx, int n, const float* wav, int Tc, bool final, int64_t* codes, float* quantized, float* enc_out) {
    fc_engine* e = S->e;
    fc::Src s; s.ptr = wav; s.div = S->state; s.used = 3;       // the session's scale [B] (ones when reset gave none)
    Act last = run_encoder(e, cx, stream_pass(S, n, final), s, Tc);
    const int Tfc = final ? frames_for(e, Tc) : Tc / total_hop(e);
    if (!cx.dry && last.T != Tfc) cx.fail("internal: frame count of a streaming push");
    const fc::RagLen rows;                                      // lock-step: every row has the push's frames
    return do_quantize(e, cx, last, Tfc, S->n_q, codes, quantized, nullptr, enc_out, nullptr, nullptr, &rows);
}

int stream_decode_pass(const fc_stream* S, Ctx& cx, int n, const float* z_bdt, int Tfc, int use_scale, float* wav) {
    Act last = run_decoder(S->e, cx, stream_pass(S, n, false), z_bdt, Tfc);
    return finish_decode(S->e, cx, last, use_scale ? S->state : nullptr, last.T, wav, nullptr);
}

// ---- length-aware (ragged) pass -------------------------------------------------------------------------------------------------
// What a ragged call must reproduce is the OFFLINE callable on every row alone, cut at the row's own length.  The pass differs from the
// offline one in three places: the volume scale (the row's own samples), the conv step (ragged_conv: a staging pass that pads every row at
// its own end, then the layer's GEMM kernel without padding over the common width) and the GroupNorm statistics (the row's valid columns
// only).  Columns behind a row's end hold finite garbage from then on (the staging pass writes zeros there and never reads there), which
// the LSTM (forward in time, rows independent) and the quantiser (per frame) compute and the final masking stores zero.

// why this engine has no length-aware calls, or null.  Each reason names the configuration key.
const char* ragged_refusal(const fc_engine* e) {
    const fc_arch& a = e->arch;
    if (a.model_type != 0) return "length-aware batches are not available for model: freq_codec (time-domain codec only)";
    if (a.lstm_layers > 0 && a.seq_model == 1) return "length-aware batches are not available for seq_model: transformer (it needs a key mask per row)";
    if (a.q0_ds_ratio > 1) return "length-aware batches are not available for quantizer_conf.q0_ds_ratio > 1 (the half-rate first stage is laid out per batch width)";
    return nullptr;
}

// One SConv1d / SConvTranspose1d (+ GroupNorm) of a ragged pass
Act ragged_conv(fc_engine* e, Ctx& cx, const Pass& p, const ConvLayer& L, fc::Src s0, fc::Src s1, int elu, int T) {
    const int B = cx.B, pt = stream_pt(L);
    const fc::RagLen in = ragged_len(cx, p);
    const int Tp = L.transposed ? T + 2 : pt + T + fc::ragged_extra(T, L.k, pt, L.stride);
    float* buf = cx.alloc<float>((size_t)B * L.cin * Tp);
    fc::RaggedStage g;
    g.s0 = s0; g.s1 = s1; g.elu = elu; g.alpha = e->arch.elu_alpha;
    g.B = B; g.C = L.cin; g.Tin = T; g.Tp = Tp; g.k = L.k; g.pt = pt; g.stride = L.stride;
    g.causal = L.causal ? 1 : 0; g.transposed = L.transposed ? 1 : 0; g.len = in; g.buf = buf;
    cx.launch("ragged stage", L.prefix.c_str(), [] { return "ragged_stage_kernel (length-aware: prologue and per-row padding of a conv)"; }, 0.0,
              4.0 * B * L.cin * ((double)T * (s1.used ? 2 : 1) + Tp), [&] { return fc::launch_ragged_stage(g, cx.st); });
    // a transposed layer computes T + 1 tap pairs; unpad1d trims left = r - r/2 of them when the net is not causal
    const Staged r = staged_conv(e, cx, L, buf, Tp, T, T + 1, L.causal ? 0 : L.stride - L.stride / 2);
    Act out = r.out;
    if (!cx.dry && out.T != conv_geom(L, T).Tout) cx.fail("internal: staged width of a ragged conv (" + L.prefix + ")");
    if (L.has_norm) {
        fc::RagLen valid = in;                        // the row's columns of what GroupNorm sees
        if (L.transposed) { valid.mul *= L.stride; valid.add = L.stride; }
        else valid.div *= L.stride;                   // strided convs sit on the encoder side only (mul == 1 there)
        double* partials = cx.alloc<double>((size_t)B * L.cout * fc::ragged_gn_segments(r.pitch) * 2);
        out.aff = cx.alloc<float>((size_t)B * L.cout * 2);
        out.normed = true;
        cx.launch("ragged GroupNorm statistics", L.prefix.c_str(),
                  [] { return "ragged_gn_partials_kernel (length-aware: GroupNorm sums over a row's valid columns)"; }, 0.0, 4.0 * B * L.cout * (double)r.pitch,
                  [&] { return fc::launch_ragged_gn_partials(r.stored, B, L.cout, r.pitch, valid, partials, cx.st); });
        cx.launch("ragged gn_finalize", L.prefix.c_str(),
                  [&] { return fc::launch_ragged_gn_finalize(partials, B, L.cout, r.pitch, valid, L.gamma, L.beta, e->arch.gn_eps, out.aff, cx.st); });
    }
    return out;
}

// a ragged call: the clamped device lengths in the workspace; frame_div of them make a frame
Pass ragged_pass(fc_engine* e, Ctx& cx, const int32_t* lengths, int Tmax, int frame_div) {
    int* lens = cx.alloc<int>(cx.B);
    cx.launch("ragged lengths", "", [&] { return fc::launch_ragged_lengths(lengths, cx.B, Tmax, lens, e->status_dev, cx.st); });
    Pass p;
    p.kind = Pass::Ragged; p.lengths = lens; p.frame_div = frame_div;
    return p;
}

// zero behind every row's frames in the encoder-side outputs
void ragged_mask_encoded(fc_engine* e, Ctx& cx, const Pass& p, int Tf, int n_q, int64_t* codes, float* quantized, float* sub_quants, float* enc_out) {
    const int B = cx.B, D = e->arch.dimension;
    fc::RagLen f; f.lens = p.lengths; f.div = total_hop(e);
    cx.launch("ragged mask", "codes", [&] { return fc::launch_ragged_mask_i64(codes, n_q, B, 1, Tf, 1, f, cx.st); });
    if (quantized) cx.launch("ragged mask", "quantized", [&] { return fc::launch_ragged_mask_f32(quantized, 1, B, 1, Tf, D, f, cx.st); });
    if (sub_quants) cx.launch("ragged mask", "sub_quants", [&] { return fc::launch_ragged_mask_f32(sub_quants, n_q, B, e->cdim(), Tf, 1, f, cx.st); });
    if (enc_out) cx.launch("ragged mask", "enc_out", [&] { return fc::launch_ragged_mask_f32(enc_out, 1, B, 1, Tf, D, f, cx.st); });
}

int ragged_ready(fc_engine* e) {
    if (check_ready(e)) return 1;
    if (const char* why = ragged_refusal(e)) return fail(why);
    return 0;
}

// the encoder side of the four calls over one context (dry: workspace sizing)
int ragged_encode(fc_engine* e, Ctx& cx, const float* wav, const int32_t* lengths, int T, int n_q, int64_t* codes, float* quantized,
                  float* sub_quants, float* scale, float* enc_out, float** qbdt, Pass* pass) {
    const Pass p = ragged_pass(e, cx, lengths, T, total_hop(e));
    if (do_encode(e, cx, wav, T, n_q, codes, quantized, sub_quants, scale, enc_out, qbdt, p)) return 1;
    ragged_mask_encoded(e, cx, p, frames_for(e, T), n_q, codes, quantized, sub_quants, enc_out);
    if (pass) *pass = p;
    return cx.err;
}

int stream_ready(fc_stream* S) {
    if (!S) return fail("null stream");
    if (S->broken)
        return fail("a push of this session failed after it had begun to write carries: the utterance's state is invalid until fc_stream_reset");
    return check_ready(S->e);
}

// the bound of a session with a key / value cache: a push that would take a side past max_frames is refused before its first launch
int frames_fit(const fc_stream* S, bool dec, int frames) {
    const int have = dec ? S->dec_frames : S->enc_frames;
    if (S->max_frames > 0 && have + frames > S->max_frames)
        return fail(std::string(dec ? "streaming decode" : "streaming encode") + ": this push of " + std::to_string(frames) + " frames would take the utterance to " +
                    std::to_string(have + frames) + " frames, past the session's max_frames = " + std::to_string(S->max_frames) +
                    " (the size of its key / value cache); nothing was changed, fc_stream_reset starts the next utterance");
    return 0;
}

int stream_decode_check(fc_stream* S, int Tfc) {
    if (S->dec_pushes < 0) return fail("streaming decode: fc_stream_reset first");
    if (Tfc <= 0 || Tfc > ceil_div_i(S->max_chunk, total_hop(S->e))) return fail("streaming decode: a push holds 1 .. max_chunk_samples / hop frames");
    if (S->dec_pushes == 0 && Tfc < S->dec_min_first)
        return fail("streaming decode: the first push of an utterance must hold at least " + std::to_string(S->dec_min_first) +
                    " frames (the offline call's reflected left padding spans them); shorter utterances go through the offline call");
    return frames_fit(S, true, Tfc);
}

// ---- graph replay of a push (include/funcodec_amd.h) ----------------------------------------------------------
// FC_SESSION_GRAPH=0: the process switch that keeps every session eager, whatever fc_graph*_set is asked
bool session_graph_allowed() {
    static const int on = fc::deploy_switch("FC_SESSION_GRAPH", 1);
    return on != 0;
}

enum GraphForm { kFormEncode = 0, kFormDecodeCodes = 1, kFormDecodeEmb = 2 };

Session::GraphKey graph_key(const Session& s, int form, int width, int parity, int use_scale, std::array<const void*, 5> ptr, void* ws, size_t ws_bytes,
                            void* stream) {
    Session::GraphKey k;
    k.form = form; k.width = width; k.parity = parity & 1; k.n_q = s.n_q; k.use_scale = use_scale ? 1 : 0;
    k.ptr = ptr; k.ws = ws; k.ws_bytes = ws_bytes; k.stream = stream;
    k.nq_table = row_nq_table(s.e); k.nq_rows = (int)s.e->row_nq.size();
    k.rvq_beam = s.e->rvq_beam;
    if (form == kFormEncode && s.e->floor.on()) {
        const fc_engine::Floor& f = s.e->floor;
        k.floor_table = f.floor_dev; k.floor_out = f.n_q_out; k.floor_min = f.min_nq; k.floor_chain = f.chain ? 1 : 0;
        k.floor_frames = f.nq_frames_out;
    }
    if (form == kFormDecodeCodes) k.push_nq = s.e->push_nq.table;
    return k;
}

// One push of a session, after every check of it has passed.  body(cx, captured) walks the whole pass over a fresh context and returns
// its error; `eager(st)` enqueues what must not sit inside a graph (the slot push's copy from host memory) and is called in front of a
// graph launch only: an eager pass enqueues that copy itself.  key: null for a push that is not to be cached (a one-off).
// Returns 0, 1 (the pass failed: its message is set) or 2 (the graph's launch failed: what it has written is unknown).
//   hit:  eager part, hipGraphLaunch.
//   miss: the pass is captured on the caller's stream (thread-local mode: one stream, a linear chain, nothing executes), instantiated,
//         launched and stored; the least recently used of kMaxGraphs graphs goes.  A launch that fails while capturing fails the push.
//   If the stream cannot be captured or the graph not instantiated, the sticky error is cleared and the push runs eagerly (fallbacks).
template <typename Eager, typename Body>
int session_push(Session* s, const Session::GraphKey* key, void* ws, size_t ws_bytes, void* stream, Eager&& eager, Body&& body) {
    auto run = [&](bool captured) {
        Ctx cx = make_ctx(s->e, s->B, ws, ws_bytes, stream);
        return body(cx, captured) ? 1 : 0;
    };
    if (!key || !s->graph_on || s->e->profiling) return run(false);
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](hipGraphExec_t exec) {
        hipError_t er = eager(st);
        if (er == hipSuccess) er = hipGraphLaunch(exec, st);
        if (er != hipSuccess) { fail(std::string("the graph launch of a push failed: ") + hipGetErrorString(er)); return 2; }
        return 0;
    };
    const unsigned long long tick = ++s->graph_tick;
    for (Session::Graph& g : s->graphs)
        if (g.key == *key) {
            g.used = tick;
            if (const int rc = launch(g.exec)) return rc;
            ++s->graph_counts[0];
            return 0;
        }
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        ++s->graph_counts[3];
        return run(false);
    }
    const int err = run(true);
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(st, &graph);
    hipGraphExec_t exec = nullptr;
    if (!err && ec == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) exec = nullptr;
    if (graph) (void)hipGraphDestroy(graph);
    if (err) return 1;                                  // a launch failed while capturing: a failed push, nothing is stored
    if (!exec) {
        (void)hipGetLastError();
        ++s->graph_counts[3];
        return run(false);
    }
    if (const int rc = launch(exec)) { (void)hipGraphExecDestroy(exec); return rc; }
    if (s->graphs.size() >= Session::kMaxGraphs) {
        auto lru = std::min_element(s->graphs.begin(), s->graphs.end(), [](const Session::Graph& a, const Session::Graph& b) { return a.used < b.used; });
        (void)hipGraphExecDestroy(lru->exec);
        s->graphs.erase(lru);
        ++s->graph_counts[2];
    }
    Session::Graph g;
    g.key = *key; g.exec = exec; g.used = tick;
    s->graphs.push_back(g);
    ++s->graph_counts[1];
    return 0;
}
const auto no_eager_part = [](hipStream_t) { return hipSuccess; };

int session_set_graph(Session* s, int on) {
    s->graph_on = on && session_graph_allowed();
    if (!s->graph_on) s->drop_graphs();
    return 0;
}
int session_graph_counts(const Session* s, int64_t* out) {
    if (!s || !out) return fail("null argument");
    std::copy(s->graph_counts, s->graph_counts + 4, out);
    return 0;
}

// A decode push of either form (`in`: codes or embeddings): enqueued whole, or the session is broken.  The first push of an utterance
// stages reflections and is a one-off; every later one is a steady push that a session with graph replay captures and replays.
int stream_decode_push(fc_stream* S, int form, const void* in, int Tfc, int use_scale, float* wav, float* emb_out, void* ws, size_t ws_bytes, void* stream) {
    const Session::GraphKey key = graph_key(*S, form, Tfc, S->dec_pushes, use_scale, {in, wav, emb_out}, ws, ws_bytes, stream);
    const int rc = session_push(S, S->dec_pushes > 0 ? &key : nullptr, ws, ws_bytes, stream, no_eager_part, [&](Ctx& cx, bool) {
        const float* z = form == kFormDecodeCodes ? decoder_input_codes(S->e, cx, (const int64_t*)in, Tfc, S->n_q, emb_out, nullptr, false, S->e->push_nq.table)      // the lookup is per frame: nothing to carry
                                                  : decoder_input_emb(S->e, cx, (const float*)in, Tfc);
        if (cx.err) return 1;                           // nothing of the state has been written yet
        S->broken = true;
        if (stream_decode_pass(S, cx, S->dec_pushes, z, Tfc, use_scale, wav)) return 1;
        S->broken = false;
        return 0;
    });
    if (rc == 2) S->broken = true;
    if (rc) return 1;
    S->dec_pushes++;
    S->dec_frames += Tfc;
    return 0;
}


// ---- slot session ---------------------------------------------------------------------------------------------------------------
// What a slot must reproduce is what a streaming session reproduces: the OFFLINE callable on the concatenation of the slot's pushes of
// one utterance, whatever the other slots of the push do.  A push is a pass of the fourth kind (Pass::Slots): the staging pass of every conv
// with a context treats each row by its own count and flags (slots_conv), the LSTM masks the steps a row does not take, the quantiser runs
// per frame over the common width, and what lies behind a row's valid part of every output is zeroed last (the ragged pass's masking).

int slots_ready(fc_slots* Q) {
    if (!Q) return fail("null slot session");
    return check_ready(Q->e);
}

// The rules of a push (include/funcodec_amd.h), checked for every slot BEFORE anything is enqueued or changed.  `unit`: what a count
// counts; whole: non-final counts are multiples of it (the hop on the encoder side, 1 frame on the decoder side).
int slots_check(const fc_slots* Q, bool decode, const int32_t* counts, const int32_t* flags, int width, int max_width) {
    const int S = Q->B, hop = total_hop(Q->e);
    const char* side = decode ? "slot decode" : "slot encode";
    const char* unit = decode ? "frames" : "samples";
    const std::vector<char>& phase = decode ? Q->dec_phase : Q->enc_phase;
    const int min_first = decode ? Q->dec_min_first : Q->enc_min_first, whole = decode ? 1 : hop;
    auto bad = [&](int b, const std::string& what) { return fail(std::string(side) + ": slot " + std::to_string(b) + ": " + what); };
    if (width < 1 || width > max_width)
        return fail(std::string(side) + ": a push is 1 .. " + std::to_string(max_width) + " " + unit + " wide (max_chunk_samples), got " + std::to_string(width));
    int active = 0;
    for (int b = 0; b < S; ++b) {
        const int n = counts[b], f = flags[b];
        if (n < 0 || n > width) return bad(b, "a count lies in [0, the push's width " + std::to_string(width) + "], got " + std::to_string(n));
        if (f & ~(FC_SLOT_START | FC_SLOT_FINAL)) return bad(b, "unknown flag bits");
        if (n == 0) {
            if (f) return bad(b, "an idle slot (count 0) takes no START or FINAL: a push that starts or ends an utterance holds at least one of its " + std::string(unit));
            continue;
        }
        ++active;
        if (!(f & FC_SLOT_START) && phase[b] != fc_slots::Running)
            return bad(b, phase[b] == fc_slots::Poisoned
                              ? "a push of this session failed after it had begun to write carries: the slot's state is invalid until it is restarted with START"
                              : phase[b] == fc_slots::Ended ? "the utterance took its FINAL push; the next push of this slot needs START"
                                                            : "no utterance is running: a push without START continues one");
        if (!(f & FC_SLOT_FINAL) && n % whole != 0)
            return bad(b, "every push but the FINAL one must be a positive multiple of the hop (" + std::to_string(hop) + " samples), got " + std::to_string(n) +
                              "; it is not padded silently");
        if ((f & FC_SLOT_START) && n < min_first)
            return bad(b, "the START push of an utterance must hold at least " + std::to_string(min_first) + " " + unit +
                              " (fc_slots_min_first: the offline call's reflected left padding spans them), got " + std::to_string(n));
        if (Q->max_frames > 0) {                          // the bound of the slot's key / value cache
            const int have = (f & FC_SLOT_START) ? 0 : (decode ? Q->dec_frames : Q->enc_frames)[b], add = ceil_div_i(n, whole);
            if (have + add > Q->max_frames)
                return bad(b, "this push of " + std::to_string(add) + " frames would take the utterance to " + std::to_string(have + add) +
                                  " frames, past the session's max_frames = " + std::to_string(Q->max_frames) +
                                  " (the size of its key / value cache); nothing was changed, a push with START begins the slot's next utterance");
        }
    }
    if (!active) return fail(std::string(side) + ": no slot is active in this push (every count is 0)");
    return 0;
}

// The counts and flags of a push on the device: ONE copy out of the session's own host buffer to the HEAD of the workspace.  The table
// is the place a fresh context's first allocation gets (slots_table), so its address depends on the workspace pointer alone: a captured
// push reads it where the copy in front of every replay writes it (slots_upload), and slots_pass refuses any other order of allocation.
// Q->push is pageable memory that the next push overwrites.  That is correct because the runtime stages a pageable host-to-device copy
// before hipMemcpyAsync returns (the call is synchronous with respect to the host buffer, as for fc_stream_reset's ones); the price is
// that the host waits there instead of queueing the next push behind this one.  A push is synchronised by its caller anyway (the wrapper
// slices its outputs per slot).  The copy is never part of a captured graph: a capture takes no copy from pageable host memory.
size_t slots_table_words(const fc_slots* Q) { return (size_t)(Q->max_frames > 0 ? 3 : 2) * Q->B; }      // with a cache the rows' positions travel behind the flags
int32_t* slots_table(void* workspace) { return (int32_t*)((char*)workspace + Ctx().off); }

// the host side of the copy: counts, flags and, with a cache, the positions of the push (a START row's is 0) in Q->push
void slots_fill(fc_slots* Q, bool decode, const int32_t* counts, const int32_t* flags) {
    const int S = Q->B;
    std::copy(counts, counts + S, Q->push.begin());
    std::copy(flags, flags + S, Q->push.begin() + S);
    const std::vector<int32_t>& frames = decode ? Q->dec_frames : Q->enc_frames;
    for (int b = 0; Q->max_frames > 0 && b < S; ++b) Q->push[2 * S + b] = (flags[b] & FC_SLOT_START) ? 0 : frames[b];
}

// the copy in front of a captured or replayed push.  A workspace too small for the table takes no copy: the pass fails at its first allocation.
hipError_t slots_upload(fc_slots* Q, bool decode, const int32_t* counts, const int32_t* flags, void* workspace, size_t workspace_bytes, hipStream_t st) {
    const size_t bytes = slots_table_words(Q) * sizeof(int32_t);
    if (!workspace || Ctx().off + bytes + Ctx::kTailSlack > workspace_bytes) return hipSuccess;
    slots_fill(Q, decode, counts, flags);
    return hipMemcpyAsync(slots_table(workspace), Q->push.data(), bytes, hipMemcpyHostToDevice, st);
}

// upload: the pass enqueues the copy itself (an eager push); a captured pass leaves it to slots_upload
Pass slots_pass(fc_slots* Q, Ctx& cx, bool decode, const int32_t* counts, const int32_t* flags, bool upload = true) {
    const int S = cx.B;
    Pass p;
    p.kind = Pass::Slots; p.sess = Q; p.n = decode ? Q->dec_pushes : Q->enc_pushes; p.frame_div = 1; p.graphed = !upload;
    const bool cached = Q->max_frames > 0;
    const size_t words = slots_table_words(Q);
    int32_t* dev = cx.alloc<int32_t>(words);
    if (!cx.dry && dev && dev != slots_table(cx.base)) cx.fail("internal: the table of a slot push is not the first allocation of its pass");
    p.lengths = dev; p.flags = at(dev, S);
    if (cached) p.pos = at(dev, 2 * S);
    if (!cx.dry) {
        slots_fill(Q, decode, counts, flags);
        p.host_push = Q->push.data();
    }
    if (upload) cx.launch("copy", "slot counts", [&] { return hipMemcpyAsync(dev, Q->push.data(), words * sizeof(int32_t), hipMemcpyHostToDevice, cx.st); });
    return p;
}

// the rows that START: LSTM state of the side cleared, and on the encoder side the slot's scale set
void slots_start(fc_slots* Q, Ctx& cx, const Pass& p, bool decode, const float* scale) {
    const LstmBlock& lb = decode ? Q->e->dec_lstm : Q->e->enc_lstm;
    float* lstm = lb.H ? lstm_state(*Q, decode) : nullptr;
    if (!lstm && decode) return;
    cx.launch("slots start", "", [&] {
        return fc::launch_slots_start(p.flags, cx.B, lstm, (int)lb.layers.size(), lb.H, scale, decode ? nullptr : Q->state, cx.st);
    });
}

int slots_encode_pass(fc_slots* Q, Ctx& cx, const float* wav, int Tc, const int32_t* counts, const int32_t* flags, const float* scale, int64_t* codes,
                      float* quantized, float* enc_out, bool captured = false) {
    fc_engine* e = Q->e;
    const Pass p = slots_pass(Q, cx, false, counts, flags, !captured);
    slots_start(Q, cx, p, false, scale);
    fc::Src s; s.ptr = wav; s.div = Q->state; s.used = 3;       // the slots' scale [S]
    Act last = run_encoder(e, cx, p, s, Tc);
    const int Tf = frames_for(e, Tc);
    if (!cx.dry && last.T != Tf) cx.fail("internal: frame count of a slot push");
    fc::RagLen rows; rows.lens = p.lengths; rows.div = total_hop(e);      // a slot's frames in this push: ceil(samples / hop), 0 for an idle one
    if (do_quantize(e, cx, last, Tf, Q->n_q, codes, quantized, nullptr, enc_out, nullptr, nullptr, &rows)) return 1;
    Pass m = p; m.frame_div = total_hop(e);                          // ragged_mask_encoded counts samples
    ragged_mask_encoded(e, cx, m, Tf, Q->n_q, codes, quantized, nullptr, enc_out);
    return cx.err;
}

// z: the decoder input [S][D][Tf] of either decode call; what lies behind a row's frames in it is never read (dec_first is staged)
int slots_decode_pass(fc_slots* Q, Ctx& cx, const Pass& p, const float* z_bdt, int Tf, int use_scale, float* wav) {
    slots_start(Q, cx, p, true, nullptr);
    Act last = run_decoder(Q->e, cx, p, z_bdt, Tf);
    fc::RagLen v; v.lens = p.lengths; v.mul = total_hop(Q->e);
    return finish_decode(Q->e, cx, last, use_scale ? Q->state : nullptr, last.T, wav, &v);
}

// the frames the rows of an enqueued push have added to their key / value caches (a START row begins at 0); `whole`: counts per frame
void slots_advance(fc_slots* Q, bool decode, const int32_t* counts, const int32_t* flags, int whole) {
    if (Q->max_frames <= 0) return;
    std::vector<int32_t>& frames = decode ? Q->dec_frames : Q->enc_frames;
    for (int b = 0; b < Q->B; ++b)
        if (counts[b] > 0) frames[b] = ((flags[b] & FC_SLOT_START) ? 0 : frames[b]) + ceil_div_i(counts[b], whole);
}

// a push has been enqueued (ok) or failed after its first launch: the slots' phases and the side's parity
void slots_commit(fc_slots* Q, bool decode, const int32_t* counts, const int32_t* flags, bool ok) {
    std::vector<char>& phase = decode ? Q->dec_phase : Q->enc_phase;
    if (!ok) {      // carries and LSTM state are a mix of old and new, on both parities: every slot restarts, on either side
        std::fill(Q->enc_phase.begin(), Q->enc_phase.end(), (char)fc_slots::Poisoned);
        std::fill(Q->dec_phase.begin(), Q->dec_phase.end(), (char)fc_slots::Poisoned);
        return;
    }
    for (int b = 0; b < Q->B; ++b)
        if (counts[b] > 0) phase[b] = (flags[b] & FC_SLOT_FINAL) ? fc_slots::Ended : fc_slots::Running;
    slots_advance(Q, decode, counts, flags, decode ? 1 : total_hop(Q->e));
    ++(decode ? Q->dec_pushes : Q->enc_pushes);
}

}  // namespace

// ====================================================================================================
extern "C" {

int fc_abi_version(void) { return FC_ABI_VERSION; }
const char* fc_last_error(void) { return g_err.c_str(); }
// the other translation units of the library (laura.hip) report through the same thread-local message
void fc_set_last_error_(const char* msg) { g_err = msg ? msg : ""; }

int fc_engine_create(const fc_arch* arch, int device, fc_engine** out) {
    if (!arch || !out) return fail("null argument");
    if (arch->abi_version != FC_ABI_VERSION) return fail("fc_arch.abi_version mismatch");
    if (arch->n_residual_layers < 1 || arch->n_residual_layers > 8 || arch->dilation_base < 1)
        return fail("fc_arch.n_residual_layers must be in 1..8 and dilation_base >= 1");
    if (arch->norm_type < 0 || arch->norm_type > 2) return fail("fc_arch.norm_type must be 0 (GroupNorm), 1 (weight_norm) or 2 (none)");
    if (arch->norm_type == 0 && arch->causal) return fail("GroupNorm convs cannot be causal (the reference refuses it too, conv.py:46-47)");
    if (arch->n_ratios < 1 || arch->n_ratios > FC_MAX_RATIOS) return fail("n_ratios out of range");
    if (arch->compress < 1 || arch->n_filters < 2 || (arch->n_filters % arch->compress) != 0) return fail("bad n_filters/compress");
    if (arch->n_filters % 2) return fail("n_filters must be even");
    const int D = arch->dimension;
    if (!(D == 16 || D == 32 || D == 64 || D == 128 || D == 256 || D == 512)) return fail("dimension must be one of 16/32/64/128/256/512");
    if (arch->codec_dim < 0 || arch->codec_range < 0.f) return fail("fc_arch.codec_dim / codec_range must be >= 0");
    if (arch->codec_dim > 0) {
        const int Dc = arch->codec_dim;
        if (!(Dc == 16 || Dc == 32 || Dc == 64 || Dc == 128 || Dc == 256 || Dc == 512)) return fail("codec_dim must be one of 16/32/64/128/256/512");
    }
    if (arch->codebook_size % 64 || (arch->codebook_size > 128 && arch->codebook_size % 128))
        return fail("codebook_size must be a multiple of 64, and of 128 above 128 (8 waves x 16-code tiles)");
    if (arch->seq_model != 0 && arch->seq_model != 1) return fail("fc_arch.seq_model must be 0 (SLSTM) or 1 (TransformerEncoder)");
    if (arch->seq_model == 0 && arch->lstm_layers > 0 && ((arch->n_filters << arch->n_ratios) % 16)) return fail("LSTM width must be a multiple of 16");
    if (arch->seq_model == 0 && arch->lstm_layers > FC_LSTM_MAX_LAYERS) return fail("too many LSTM layers");
    if (arch->seq_model == 1 && arch->lstm_layers > 0) {
        const int C = arch->n_filters << arch->n_ratios;
        if (arch->seq_heads < 1 || C % arch->seq_heads || !fc::seq_attn_supported(C / arch->seq_heads))
            return fail("transformer bottleneck: head size C / seq_heads must be 16, 32, 64, 128 or 256 (C = " + std::to_string(C) + ")");
        if (C % 16 || C > 1024) return fail("transformer bottleneck: width must be a multiple of 16 and at most 1024 (LayerNorm kernel)");
        if (arch->seq_ff < 1) return fail("transformer bottleneck: seq_ff must be >= 1");
        if (arch->lstm_layers > 64) return fail("transformer bottleneck: at most 64 blocks");
    }
    for (int i = 0; i < arch->n_ratios; ++i)
        if (arch->ratios[i] < 1) return fail("ratios must be >= 1");
    if (arch->model_type != 0 && arch->model_type != 1) return fail("fc_arch.model_type must be 0 (encodec) or 1 (freq_codec, mag_phase)");
    if (arch->model_type == 0 && (arch->input_channels < 0 || arch->input_channels > 2))
        return fail("encodec: input_channels must be 1 (0 reads as 1) or 2 (stereo; the reference asserts channels <= 2, codec_basic.py:344)");
    if (arch->model_type == 1) {
        if (arch->norm_type != 0 && arch->norm_type != 1) return fail("freq_codec: norm must be time_group_norm or weight_norm");
        if (arch->input_channels != 3 && arch->input_channels != 2)
            return fail("freq_codec: input_channels must be 3 (codec_domain mag_phase: log-magnitude, phase re, phase im) or 2 (mag_angle: log-magnitude, angle)");
        if (arch->n_fft < 64 || (arch->n_fft & (arch->n_fft - 1)) || arch->stft_hop < 1 || arch->stft_hop > arch->n_fft)
            return fail("freq_codec: n_fft must be a power of two >= 64 and 1 <= stft_hop <= n_fft");
        if (arch->stft_hop % 2) return fail("freq_codec: stft_hop must be even");
        if (arch->dilation_base != 1 && arch->n_residual_layers > 1) return fail("freq_codec: dilated residual stacks are not built for the 2-D nets");
        int f = arch->n_fft / 2 + 1;
        for (int i = arch->n_ratios - 1; i >= 0; --i) {
            const int fr = arch->ratios_f[i];
            if (fr < 1) return fail("freq_codec: ratios_f must be >= 1");
            const int tot = (2 * fr - 1) - (fr - 1);
            f = (f + tot - 2 * fr) / fr + 1;
        }
        if (f != 1) return fail("freq_codec: the frequency ratios must reduce n_fft / 2 + 1 bins to exactly one");
    }
    fc_engine* e = new fc_engine();
    e->arch = *arch;
    e->device = device;
    build_plan(e);
    for (const auto& kv : e->by_prefix)
        if (kv.second->unsupported) {
            const std::string msg = "stride " + std::to_string(kv.second->gstride) + " / kernel " + std::to_string(kv.second->gk) + " of " + kv.first +
                                    " exceeds the conv kernel's slab (ratios above 16 are not built)";
            delete e;
            return fail(msg);
        }
    if (arch->model_type == 1) {          // torch.nn.Conv2d / ConvTranspose2d constraints on `groups` (conv_group_ratio > 0)
        std::vector<const ConvLayer*> ls;
        for (auto* st : {&e->enc_stages, &e->dec_stages})
            for (auto& S : *st) {
                for (auto& R : S.res) { ls.push_back(&R.shortcut); ls.push_back(&R.block1); ls.push_back(&R.block3); }
                ls.push_back(&S.resample);
            }
        for (const ConvLayer* L : ls)
            if (L->groups < 1 || L->c2d % L->groups || L->cout % L->groups) {
                const std::string msg = "freq_codec: conv_group_ratio gives " + std::to_string(L->groups) + " groups for " + L->prefix + " (" +
                                        std::to_string(L->c2d) + " -> " + std::to_string(L->cout) + " channels)";
                delete e;
                return fail(msg);
            }
    }
    *out = e;
    return 0;
}

int fc_engine_profile(fc_engine* e, int enable) {
    if (!e) return fail("null engine");
    e->profiling = enable != 0;
    return 0;
}

int fc_engine_profile_read(fc_engine* e, fc_prof* out) {
    if (!e || !out) return fail("null argument");
    for (int i = 0; i < FC_PROF_CLASSES; ++i) {
        memset(&out[i], 0, sizeof(fc_prof));
        if (i < (int)e->prof_names.size()) strncpy(out[i].kernel, e->prof_names[i].c_str(), sizeof(out[i].kernel) - 1);
    }
    if (!e->spans.empty()) HIP_TRY(hipEventSynchronize(e->spans.back().b));
    for (auto& s : e->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) != hipSuccess) continue;
        out[s.cls].total_ms += ms; out[s.cls].flops += s.flops; out[s.cls].bytes += s.bytes; out[s.cls].launches += 1;
    }
    e->spans.clear();
    e->events_used = 0;
    return 0;
}

void fc_engine_destroy(fc_engine* e) {
    if (!e) return;
    for (hipEvent_t ev : e->event_pool) (void)hipEventDestroy(ev);
    for (void* p : e->dev_allocs) (void)hipFree(p);
    if (e->status_host) (void)hipHostFree((void*)e->status_host);
    delete e;
}

int fc_engine_num_weights(const fc_engine* e) { return e ? (int)e->expected.size() : 0; }

int fc_engine_weight_info(const fc_engine* e, int i, const char** name, int64_t* dims) {
    if (!e || i < 0 || i >= (int)e->expected.size()) return -1;
    if (name) *name = e->expected[i].first.c_str();
    const auto& d = e->expected[i].second;
    if (dims) for (size_t j = 0; j < d.size(); ++j) dims[j] = d[j];
    return (int)d.size();
}

int fc_engine_set_weight(fc_engine* e, const char* name, const float* host, const int64_t* dims, int ndim) {
    if (!e || !name || !host || !dims) return fail("null argument");
    if (e->finalized) return fail("engine already finalized");
    for (auto& ex : e->expected) {
        if (ex.first != name) continue;
        if ((int)ex.second.size() != ndim) return fail(std::string("rank mismatch for ") + name);
        size_t n = 1;
        for (int j = 0; j < ndim; ++j) {
            if (ex.second[j] != dims[j]) return fail(std::string("shape mismatch for ") + name);
            n *= (size_t)dims[j];
        }
        HostTensor& t = e->host[name];
        t.dims.assign(dims, dims + ndim);
        t.data.assign(host, host + n);
        t.set = true;
        return 0;
    }
    g_err = std::string("tensor not part of the hot path: ") + name;
    return 2;
}

int fc_engine_finalize(fc_engine* e) {
    if (!e) return fail("null engine");
    if (e->finalized) return 0;
    for (auto& ex : e->expected)
        if (!e->host.count(ex.first) || !e->host[ex.first].set) return fail("checkpoint is missing tensor " + ex.first);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail("no HIP device visible: the FunCodec MI355X engine has no CPU fallback");
    HIP_TRY(hipSetDevice(e->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, e->device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return fail(std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    if (e->arch.model_type == 1) {
        if (pack_conv2d(e, e->enc2_first) || pack_conv2d(e, e->dec2_last)) return 1;
        for (auto& S : e->enc_stages) {
            for (auto& R : S.res)
                if (pack_conv2d(e, R.shortcut) || pack_conv2d(e, R.block1) || pack_conv2d(e, R.block3)) return 1;
            if (pack_conv2d(e, S.resample)) return 1;
        }
        for (size_t si = 0; si < e->dec_stages.size(); ++si) {
            auto& S = e->dec_stages[si];
            for (auto& R : S.res)
                if (pack_conv2d(e, R.shortcut) || pack_conv2d(e, R.block1) || pack_conv2d(e, R.block3)) return 1;
            if (pack_convtr2d(e, S.resample, e->dec_up_phases[si])) return 1;
        }
        if (pack_conv(e, e->enc_last) || pack_conv(e, e->dec_first)) return 1;
        if (pack_dft(e)) return 1;
    } else {
        // all fused res-block heads, then all convs: the heads read the host copies of their two convs' weights (the host map is still
        // alive here)
        int err = 0;
        for_each_conv(e, [&](const ConvVisit& v) { if (!err && v.role == Role::Shortcut) err = pack_reshead(e, *v.block); });
        for_each_conv(e, [&](const ConvVisit& v) { if (!err) err = pack_conv(e, v.L); });
        if (err) return 1;
    }
    if (pack_lstm(e, e->enc_lstm)) return 1;
    if (pack_lstm(e, e->dec_lstm)) return 1;
    if (pack_tf(e, e->enc_tf) || pack_tf(e, e->dec_tf)) return 1;
    // codebooks + |e|^2 (EuclideanCodebook.quantize ddp_core_vq.py:185: embed.pow(2).sum(0)); sequential d, squares rounded
    const auto& E = e->host["quantizer.rq.model.embed"].data;
    const int nq = e->arch.num_quantizers, K = e->arch.codebook_size, D = e->cdim();
    if (e->q_proj) {       // Linear weights [out][in] are the k = 1 GEMM's [M][cin][1]
        if (pack_gemm(e, e->q_in, e->host["quantizer.input_proj.weight"].data, e->host["quantizer.input_proj.bias"].data)) return 1;
        if (pack_gemm(e, e->q_out, e->host["quantizer.output_proj.weight"].data, e->host["quantizer.output_proj.bias"].data)) return 1;
    }
    std::vector<float> en((size_t)nq * K);
    for (size_t r = 0; r < (size_t)nq * K; ++r) {
        volatile float s = 0.f;
        for (int d = 0; d < D; ++d) {
            volatile float sq = E[r * D + d] * E[r * D + d];
            s = s + sq;
        }
        en[r] = s;
    }
    if (upload(e, E, &e->cb)) return 1;
    if (K % 16 == 0 && D % 16 == 0) {
        // fragment order: [stage][16-code tile][q = d/16][g = (d%16)/4][code in tile][d%4]: lane (g, code) of a wave reads
        // 16 contiguous bytes and a whole wave instruction reads 1 KiB contiguous (row-major rows give 64-byte pieces)
        std::vector<float> F((size_t)nq * K * D);
        for (int i = 0; i < nq; ++i)
            for (int c = 0; c < K; ++c)
                for (int d = 0; d < D; ++d) {
                    const size_t tile = (size_t)i * (K / 16) + c / 16;
                    F[((tile * (D / 16) + d / 16) * 4 + (d % 16) / 4) * 64 + (size_t)(c % 16) * 4 + d % 4] = E[((size_t)i * K + c) * D + d];
                }
        if (upload(e, F, &e->cb_frag)) return 1;
    }
    if (upload(e, en, &e->enorm)) return 1;
    {   // status words: pinned host memory the kernels write to directly (error paths only)
        void* hp = nullptr;
        HIP_TRY(hipHostMalloc(&hp, FC_STATUS_WORDS * sizeof(unsigned), hipHostMallocMapped));
        memset(hp, 0, FC_STATUS_WORDS * sizeof(unsigned));
        void* dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
        e->status_host = (volatile unsigned*)hp;
        e->status_dev = (unsigned*)dp;
    }
    e->host.clear();                                  // host copies of the checkpoint are dropped
    HIP_TRY(hipDeviceSynchronize());
    e->finalized = true;
    return 0;
}

int fc_engine_hop_length(const fc_engine* e) { return e ? total_hop(e) : 0; }
int fc_engine_frames(const fc_engine* e, int n_samples) { return e ? frames_for(e, n_samples) : 0; }
int fc_engine_decoded_samples(const fc_engine* e, int n_frames) { return e ? decoded_samples(e, n_frames) : 0; }

size_t fc_engine_workspace_bytes(const fc_engine* ce, int B, int T) {
    fc_engine* e = const_cast<fc_engine*>(ce);
    if (!e || B <= 0 || T <= 0) return 0;
    // tiling is only known after finalize(); plan with the same rule here
    const int Tf = frames_for(e, T), D = e->arch.dimension;
    Ctx cx = dry_ctx(e, B);
    float* q = nullptr;
    do_encode(e, cx, nullptr, T, e->arch.num_quantizers, nullptr, nullptr, nullptr, nullptr, nullptr, &q);
    cx.alloc<float>((size_t)B * Tf * D);           // quantized when the caller does not want it
    cx.alloc<float>((size_t)B * Tf * D);           // emb for decode_codes
    decoder_input_emb(e, cx, nullptr, Tf);
    do_decode(e, cx, nullptr, Tf, nullptr, decoded_samples(e, Tf), nullptr);
    return cx.off + 4096;
}

int fc_engine_work(const fc_engine* ce, int B, int T, int n_q, fc_work* out) {
    fc_engine* e = const_cast<fc_engine*>(ce);
    if (!e || !out) return fail("null argument");
    Ctx cx = dry_ctx(e, B);
    float* q = nullptr;
    // the call counted is fc_encode_decode as the Python wrapper makes it: with the quantised embeddings (the pointer only marks presence)
    float quantized_mark;
    do_encode(e, cx, nullptr, T, n_q, nullptr, &quantized_mark, nullptr, nullptr, nullptr, &q);
    do_decode(e, cx, nullptr, frames_for(e, T), nullptr, T, nullptr);
    out->conv_flops = cx.conv_flops; out->conv_bytes = cx.conv_bytes;
    out->lstm_flops = cx.lstm_flops; out->rvq_flops = cx.rvq_flops;
    out->total_flops = cx.conv_flops + cx.lstm_flops + cx.rvq_flops + cx.attn_flops;     // transformer Linears are in conv_flops
    out->total_bytes = cx.conv_bytes;
    out->conv_launches = cx.conv_launches; out->total_launches = cx.launches;
    return 0;
}

namespace {
// fc_debug_freq_features is ONE SHOT: whatever the next fc_encode / fc_encode_decode call of this thread does -- a time-domain model, an early
// error, success -- the hook (a raw device pointer the caller may free afterwards) is disarmed when that call returns
struct FeatHookDisarm { ~FeatHookDisarm() { g_feat_hook = FeatHook(); } };
}  // namespace

int fc_encode(fc_engine* e, const float* wav, int B, int T, int n_q, int64_t* codes, float* quantized, float* sub_quants,
              float* scale, float* enc_out, void* workspace, size_t workspace_bytes, void* stream) {
    FeatHookDisarm disarm_feature_hook;
    if (check_ready(e)) return 1;
    if (!wav || !codes || B <= 0 || T <= 0) return fail("bad argument");
    if (n_q < 1 || n_q > e->arch.num_quantizers) return fail("n_q out of range");
    if (counts_check_encode(e, "fc_encode", B, n_q, false)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    return do_encode(e, cx, wav, T, n_q, codes, quantized, sub_quants, scale, enc_out, nullptr);
}

int fc_decode_emb(fc_engine* e, const float* emb, const float* scale, int B, int Tf, int out_len, float* wav,
                  void* workspace, size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!emb || !wav || B <= 0 || Tf <= 0 || out_len <= 0) return fail("bad argument");
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    return do_decode(e, cx, decoder_input_emb(e, cx, emb, Tf), Tf, scale, out_len, wav);
}

int fc_decode_codes(fc_engine* e, const int64_t* codes, int B, int Tf, int n_q, int out_len, float* wav, float* emb_out,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!codes || !wav || B <= 0 || Tf <= 0 || out_len <= 0) return fail("bad argument");
    if (n_q < 1 || n_q > e->arch.num_quantizers) return fail("n_q out of range");
    if (counts_check_decode(e, "fc_decode_codes", B, Tf, n_q, false)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    return do_decode(e, cx, decoder_input_codes(e, cx, codes, Tf, n_q, emb_out, nullptr, false, e->frame_nq.table), Tf, nullptr, out_len, wav);
}

int fc_encode_decode(fc_engine* e, const float* wav, int B, int T, int n_q, int use_scale, int64_t* codes, float* quantized,
                     float* sub_quants, float* scale, float* recon, void* workspace, size_t workspace_bytes, void* stream) {
    FeatHookDisarm disarm_feature_hook;
    if (check_ready(e)) return 1;
    if (!wav || !codes || !recon || B <= 0 || T <= 0) return fail("bad argument");
    if (n_q < 1 || n_q > e->arch.num_quantizers) return fail("n_q out of range");
    if (counts_check_encode(e, "fc_encode_decode", B, n_q, false)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    float* sc = scale;
    if (e->arch.audio_normalize && !sc) sc = cx.alloc<float>(B);
    float* qbdt = nullptr;
    if (do_encode(e, cx, wav, T, n_q, codes, quantized, sub_quants, sc, nullptr, &qbdt)) return 1;
    const int Tf = frames_for(e, T);
    const int dec_len = decoded_samples(e, Tf);                     // recon is [B, min(T, decoded samples)] (the reference's recon[:, :, :T])
    return do_decode(e, cx, qbdt, Tf, (use_scale && e->arch.audio_normalize) ? sc : nullptr, T < dec_len ? T : dec_len, recon);
}

// ---- length-aware (ragged) calls: the offline siblings' signatures plus `lengths`
size_t fc_ragged_workspace_bytes(const fc_engine* ce, int B, int Tmax) {
    fc_engine* e = const_cast<fc_engine*>(ce);
    if (!e || B <= 0 || Tmax <= 0 || ragged_refusal(e)) return 0;
    const int Tf = frames_for(e, Tmax);
    Ctx cx = dry_ctx(e, B);
    float* q = nullptr;
    Pass p;
    float mark;                                    // optional outputs: the pointer only marks presence in a dry pass
    ragged_encode(e, cx, nullptr, nullptr, Tmax, e->arch.num_quantizers, nullptr, &mark, &mark, nullptr, &mark, &q, &p);
    decoder_input_emb(e, cx, nullptr, Tf);         // as wide as the code vectors of decode_codes
    cx.alloc<int64_t>((size_t)B * Tf * e->arch.num_quantizers);     // masked copy of the tokens
    fc::RagLen v;
    do_decode(e, cx, nullptr, Tf, nullptr, decoded_samples(e, Tf), nullptr, p, &v);
    return cx.off + 4096;
}

int fc_encode_ragged(fc_engine* e, const float* wav, const int32_t* lengths, int B, int T, int n_q, int64_t* codes, float* quantized,
                     float* sub_quants, float* scale, float* enc_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (ragged_ready(e)) return 1;
    if (!wav || !lengths || !codes || B <= 0 || T <= 0) return fail("bad argument");
    if (n_q < 1 || n_q > e->arch.num_quantizers) return fail("n_q out of range");
    if (counts_check_encode(e, "fc_encode_ragged", B, n_q, false)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    return ragged_encode(e, cx, wav, lengths, T, n_q, codes, quantized, sub_quants, scale, enc_out, nullptr, nullptr);
}

int fc_decode_emb_ragged(fc_engine* e, const float* emb, const float* scale, const int32_t* lengths, int B, int Tf, int out_len, float* wav,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (ragged_ready(e)) return 1;
    if (!emb || !lengths || !wav || B <= 0 || Tf <= 0 || out_len <= 0) return fail("bad argument");
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    const Pass p = ragged_pass(e, cx, lengths, Tf, 1);
    fc::RagLen v; v.lens = p.lengths; v.mul = total_hop(e);
    return do_decode(e, cx, decoder_input_emb(e, cx, emb, Tf), Tf, scale, out_len, wav, p, &v);
}

int fc_decode_codes_ragged(fc_engine* e, const int64_t* codes, const int32_t* lengths, int B, int Tf, int n_q, int out_len, float* wav,
                           float* emb_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (ragged_ready(e)) return 1;
    if (!codes || !lengths || !wav || B <= 0 || Tf <= 0 || out_len <= 0) return fail("bad argument");
    if (n_q < 1 || n_q > e->arch.num_quantizers) return fail("n_q out of range");
    if (counts_check_decode(e, "fc_decode_codes_ragged", B, Tf, n_q, false)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    const Pass p = ragged_pass(e, cx, lengths, Tf, 1);
    fc::RagLen f; f.lens = p.lengths;
    fc::RagLen v; v.lens = p.lengths; v.mul = total_hop(e);
    return do_decode(e, cx, decoder_input_codes(e, cx, codes, Tf, n_q, emb_out, &f, false, e->frame_nq.table), Tf, nullptr, out_len, wav, p, &v);
}

int fc_encode_decode_ragged(fc_engine* e, const float* wav, const int32_t* lengths, int B, int T, int n_q, int use_scale, int64_t* codes,
                            float* quantized, float* sub_quants, float* scale, float* recon, void* workspace, size_t workspace_bytes, void* stream) {
    if (ragged_ready(e)) return 1;
    if (!wav || !lengths || !codes || !recon || B <= 0 || T <= 0) return fail("bad argument");
    if (n_q < 1 || n_q > e->arch.num_quantizers) return fail("n_q out of range");
    if (counts_check_encode(e, "fc_encode_decode_ragged", B, n_q, false)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    float* sc = scale;
    if (e->arch.audio_normalize && !sc) sc = cx.alloc<float>(B);
    float* qbdt = nullptr;
    Pass p;
    if (ragged_encode(e, cx, wav, lengths, T, n_q, codes, quantized, sub_quants, sc, nullptr, &qbdt, &p)) return 1;
    fc::RagLen v; v.lens = p.lengths;              // a row's reconstruction is cut at its own samples (the reference's recon[:, :, :T])
    return do_decode(e, cx, qbdt, frames_for(e, T), (use_scale && e->arch.audio_normalize) ? sc : nullptr, T, recon, p, &v);
}

int fc_engine_set_row_nq(fc_engine* e, const int32_t* n_q_rows, int B, void* stream) {
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    if (!n_q_rows) { e->row_nq.clear(); return 0; }
    if (B <= 0) return fail("fc_engine_set_row_nq: a table holds at least one row");
    for (int b = 0; b < B; ++b)
        if (n_q_rows[b] < 1 || n_q_rows[b] > e->arch.num_quantizers)
            return fail("fc_engine_set_row_nq: row " + std::to_string(b) + ": a stage count lies in [1, num_quantizers = " +
                        std::to_string(e->arch.num_quantizers) + "], got " + std::to_string(n_q_rows[b]));
    if ((size_t)B > e->row_nq_cap) {    // a larger table; the old one stays allocated for the launches that may still read it
        const size_t cap = std::max<size_t>(64, 2 * (size_t)B);
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, cap * sizeof(int32_t)));
        e->dev_allocs.push_back(p);
        e->row_nq_dev = (int*)p; e->row_nq_cap = cap;
    }
    // the source of the copy is the engine's own host copy, which lives as long as the engine: the caller's table may go at once
    e->row_nq.assign(n_q_rows, n_q_rows + B);
    if (hipError_t er = hipMemcpyAsync(e->row_nq_dev, e->row_nq.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, (hipStream_t)stream);
        er != hipSuccess) {
        e->row_nq.clear();
        return fail(std::string("fc_engine_set_row_nq: copy of the table: ") + hipGetErrorString(er));
    }
    return 0;
}

namespace {
// why the quantiser's beam search is refused for this engine and width (before any launch), or 0
int rvq_beam_check(const fc_engine* e, int width, const char* who) {
    if (!fc::rvq_beam_width_ok(width) && width != 1)
        return fail(std::string(who) + ": rvq_beam: a width is one of 1, 2, 4, 8, got " + std::to_string(width));
    if (width > 1 && e->arch.q0_ds_ratio > 1)
        return fail(std::string(who) + ": rvq_beam: quantizer_conf.q0_ds_ratio > 1 shares stage 0 between frame pairs, so the frames are not independent; "
                    "the search over the stages is per frame");
    return 0;
}

// The prologue of the three fc_rvq_encode* hooks (`who`), before any launch: the arguments; then the N rows as B utterances of Tf = N / B
// frames each, B from the rate (`rate`: the hook runs under fc_engine_set_rate) or from the per-row table (none set: one utterance).
int rvq_hook_rows(fc_engine* e, const char* who, const float* x, const int64_t* codes, int N, int n_q, int width, bool search_outputs, bool rate,
                  int* B, int* Tf) {
    if (check_ready(e)) return 1;
    if (!x || !codes || N <= 0) return fail("bad argument");
    if (n_q < 1 || n_q > e->arch.num_quantizers) return fail("n_q out of range");
    const bool floor = rate && e->floor.on();          // the rate hook under a noise floor (fc_engine_set_floor): the push rule on B rows
    if (!rate && e->floor.on())
        return fail(std::string(who) + ": a noise floor is set (fc_engine_set_floor): it is for session pushes only; clear it with NULL floors");
    if (rate && !floor && !e->rate.on()) return fail(std::string(who) + ": no rate is set (fc_engine_set_rate)");
    if (rate && !floor && (!e->rate.row_err_out || !e->rate.stage_err_out))
        return fail(std::string(who) + ": the hook has no workspace: fc_engine_set_rate with row_errors_out and stage_errors_out");
    if (rvq_beam_check(e, width, who)) return 1;
    if (width == 1 && search_outputs) return fail(std::string(who) + ": paths and errors are those of a search: rvq_beam above 1");
    *B = floor ? (int)e->floor.floor.size() : rate ? (int)e->rate.ratio.size() : e->row_nq.empty() ? 1 : (int)e->row_nq.size();
    *Tf = N / *B;
    if (N % *B != 0)
        return fail(std::string(who) + ": with " + (rate ? "a rate for " : "per-row stage counts for ") + std::to_string(*B) +
                    " rows, N must be a multiple of that");
    return rate ? counts_check_encode(e, who, *B, n_q, false, true) : row_nq_check(e, *B, n_q);
}

// The greedy encode of the search and rate hooks (`quantized`: what it sums, or null) and everything behind it; the first launch that
// fails ends the sequence and is reported by name.
int rvq_hook_launch(fc_engine* e, const char* who, const RvqTail& a, float* quantized, hipStream_t st) {
    hipError_t er = hipSuccess;
    const char* failed = "";
    auto launch = [&](const char* what, double, auto&& enqueue) {
        if (er == hipSuccess && (er = enqueue()) != hipSuccess) failed = what;
    };
    launch("rvq", 0.0, [&] {
        return fc::launch_rvq_encode(a.x, a.B * a.Tf, e->cdim(), e->arch.codebook_size, a.n_q, e->cb, e->cb_frag, e->enorm, a.codes, quantized, nullptr,
                                     nullptr, a.Tf, st, nullptr, row_nq_table(e));
    });
    rvq_after_greedy(e, a, st, launch);
    return er == hipSuccess ? 0 : fail(std::string(who) + ": " + failed + ": " + hipGetErrorString(er));
}
}  // namespace

int fc_engine_set_rvq_beam(fc_engine* e, int width, void* stream) {
    (void)stream;
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    if (rvq_beam_check(e, width, "fc_engine_set_rvq_beam")) return 1;
    // outside any capture: a graph-replay session captures the launches only
    if (width > 1) HIP_TRY(fc::rvq_beam_prepare(e->cdim(), width));
    e->rvq_beam = width;
    return 0;
}

int fc_rvq_encode_beam(fc_engine* e, const float* x, int N, int n_q, int width, int64_t* codes, float* quantized, int64_t* paths, float* errors,
                       void* stream) {
    RvqTail a;
    if (rvq_hook_rows(e, "fc_rvq_encode_beam", x, codes, N, n_q, width, paths || errors, false, &a.B, &a.Tf)) return 1;
    a.x = x; a.codes = codes; a.n_q = n_q; a.width = width;
    a.quant = quantized; a.beam_sum = quantized != nullptr;
    a.paths = paths; a.errors = errors;
    return rvq_hook_launch(e, "fc_rvq_encode_beam", a, quantized, (hipStream_t)stream);
}

int fc_engine_set_rate(fc_engine* e, const double* ratio_rows, int B, int min_nq, int32_t* n_q_rows_out, double* row_errors_out,
                       float* stage_errors_out, void* stream) {
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    if (ratio_rows && e->floor.on())
        return fail("fc_engine_set_rate: a noise floor is set (fc_engine_set_floor): a call takes a rate or a floor, not both; clear one of them");
    e->rate.clear_frames();             // frame mode is given after the rate, every time (fc_engine_set_rate_frames)
    if (!ratio_rows) { e->rate.ratio.clear(); e->rate.n_q_out = nullptr; e->rate.row_err_out = nullptr; e->rate.stage_err_out = nullptr; return 0; }
    if (B <= 0) return fail("fc_engine_set_rate: a rate holds at least one row");
    if (!n_q_rows_out) return fail("fc_engine_set_rate: n_q_rows_out (device int32 [B]) takes the chosen stage counts");
    if (e->arch.q0_ds_ratio > 1)
        return fail("fc_engine_set_rate: quantizer_conf.q0_ds_ratio > 1: stage 0 quantises another frame's row, so a frame's residual is not its input "
                    "minus its codes");
    if (min_nq < 1 || min_nq > e->arch.num_quantizers)
        return fail("fc_engine_set_rate: min_nq lies in [1, num_quantizers = " + std::to_string(e->arch.num_quantizers) + "], got " + std::to_string(min_nq));
    for (int b = 0; b < B; ++b)
        if (!(ratio_rows[b] >= 0.0))
            return fail("fc_engine_set_rate: row " + std::to_string(b) + ": a ratio 10^(-target_snr_db / 10) is neither negative nor NaN");
    if ((size_t)B > e->rate.cap) {      // larger tables; the old ones stay allocated for the launches that may still read them
        const size_t cap = std::max<size_t>(64, 2 * (size_t)B);
        void *pr = nullptr, *pk = nullptr;
        HIP_TRY(hipMalloc(&pr, cap * sizeof(double)));
        e->dev_allocs.push_back(pr);
        HIP_TRY(hipMalloc(&pk, cap * sizeof(int)));
        e->dev_allocs.push_back(pk);
        e->rate.ratio_dev = (double*)pr; e->rate.k_dev = (int*)pk; e->rate.cap = cap;
    }
    // the source of the copy is the engine's own host copy, which lives as long as the engine: the caller's array may go at once
    e->rate.ratio.assign(ratio_rows, ratio_rows + B);
    if (hipError_t er = hipMemcpyAsync(e->rate.ratio_dev, e->rate.ratio.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream);
        er != hipSuccess) {
        e->rate.ratio.clear();
        return fail(std::string("fc_engine_set_rate: copy of the ratios: ") + hipGetErrorString(er));
    }
    e->rate.min_nq = min_nq;
    e->rate.n_q_out = n_q_rows_out; e->rate.row_err_out = row_errors_out; e->rate.stage_err_out = stage_errors_out;
    return 0;
}

int fc_engine_set_rate_frames(fc_engine* e, int min_nq, int32_t* n_q_frames_out, int32_t* n_codes_rows_out, double* achieved_out, void* stream) {
    (void)stream;
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    if (!e->rate.on()) return fail("fc_engine_set_rate_frames: no rate is set: it is given after fc_engine_set_rate");
    if (!n_q_frames_out) return fail("fc_engine_set_rate_frames: n_q_frames_out (device int32 [B][Tf]) takes the chosen stage counts");
    if (min_nq < 0 || min_nq > e->arch.num_quantizers)
        return fail("fc_engine_set_rate_frames: min_nq lies in [0, num_quantizers = " + std::to_string(e->arch.num_quantizers) + "], got " +
                    std::to_string(min_nq));
    e->rate.frames = true;
    e->rate.min_nq = min_nq;
    e->rate.nq_frames_out = n_q_frames_out; e->rate.n_codes_out = n_codes_rows_out; e->rate.achieved_out = achieved_out;
    return 0;
}

int fc_engine_set_floor(fc_engine* e, const double* floor_rows, int B, int min_nq, int32_t* n_q_rows_out, void* stream) {
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    e->floor.nq_frames_out = nullptr;       // frame mode is given after the floor, every time (fc_engine_set_floor_frames)
    if (!floor_rows) { e->floor.floor.clear(); e->floor.n_q_out = nullptr; e->floor.clear_form(); return 0; }
    if (e->rate.on())
        return fail("fc_engine_set_floor: a rate is set (fc_engine_set_rate): a call takes a rate or a floor, not both; clear one of them");
    if (B <= 0) return fail("fc_engine_set_floor: a floor holds at least one row");
    if (!n_q_rows_out) return fail("fc_engine_set_floor: n_q_rows_out (device int32 [B]) takes the chosen stage counts");
    if (e->arch.q0_ds_ratio > 1)
        return fail("fc_engine_set_floor: quantizer_conf.q0_ds_ratio > 1: stage 0 quantises another frame's row, so a frame's residual is not its input "
                    "minus its codes");
    if (min_nq < 1 || min_nq > e->arch.num_quantizers)
        return fail("fc_engine_set_floor: min_nq lies in [1, num_quantizers = " + std::to_string(e->arch.num_quantizers) + "], got " + std::to_string(min_nq));
    for (size_t b = 0; b < e->row_nq.size(); ++b)
        if (min_nq > e->row_nq[b])
            return fail("fc_engine_set_floor: min_nq = " + std::to_string(min_nq) + " lies above the cap of row " + std::to_string(b) + " (" +
                        std::to_string(e->row_nq[b]) + " stages, fc_engine_set_row_nq)");
    for (int b = 0; b < B; ++b)
        if (!(floor_rows[b] >= 0.0))
            return fail("fc_engine_set_floor: row " + std::to_string(b) + ": a floor D * 10^(noise_floor_db / 10) is neither negative nor NaN");
    if ((size_t)B > e->floor.cap) {     // a larger table; the old one stays allocated for the launches that may still read it
        const size_t cap = std::max<size_t>(64, 2 * (size_t)B);
        void* pf = nullptr;
        HIP_TRY(hipMalloc(&pf, cap * sizeof(double)));
        e->dev_allocs.push_back(pf);
        e->floor.floor_dev = (double*)pf; e->floor.cap = cap;
    }
    // the source of the copy is the engine's own host copy, which lives as long as the engine: the caller's array may go at once
    const std::vector<double> keep = e->floor.floor;
    e->floor.floor.assign(floor_rows, floor_rows + B);
    if (hipError_t er = hipMemcpyAsync(e->floor.floor_dev, e->floor.floor.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream);
        er != hipSuccess) {
        e->floor.floor = keep;
        return fail(std::string("fc_engine_set_floor: copy of the floors: ") + hipGetErrorString(er));
    }
    e->floor.clear_form();              // the form is given after the floor, every time (fc_engine_set_floor_form)
    e->floor.min_nq = min_nq;
    e->floor.n_q_out = n_q_rows_out;
    return 0;
}

int fc_engine_set_floor_form(fc_engine* e, int chain, double* row_errors_out, float* stage_errors_out, float* sub_quants_out, const int32_t* off_rows,
                             void* stream) {
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    if (!e->floor.on()) return fail("fc_engine_set_floor_form: no noise floor is set: it is given after fc_engine_set_floor");
    if (off_rows) {         // a row switched off keeps its cap: on the device its floor reads -1 (the push rule, csrc/rvq_rate_kernels.h)
        bool any = false;
        for (size_t b = 0; b < e->floor.floor.size(); ++b)
            if (off_rows[b]) { e->floor.floor[b] = -1.0; any = true; }
        if (any)
            if (hipError_t er = hipMemcpyAsync(e->floor.floor_dev, e->floor.floor.data(), e->floor.floor.size() * sizeof(double), hipMemcpyHostToDevice,
                                               (hipStream_t)stream);
                er != hipSuccess)
                return fail(std::string("fc_engine_set_floor_form: copy of the floors: ") + hipGetErrorString(er));
    }
    e->floor.chain = chain != 0; e->floor.row_err_out = row_errors_out; e->floor.stage_err_out = stage_errors_out; e->floor.subq_out = sub_quants_out;
    return 0;
}

int fc_engine_set_floor_frames(fc_engine* e, int min_nq, int32_t* n_q_frames_out, void* stream) {
    (void)stream;
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    if (!e->floor.on()) return fail("fc_engine_set_floor_frames: no noise floor is set: it is given after fc_engine_set_floor");
    if (!n_q_frames_out) return fail("fc_engine_set_floor_frames: n_q_frames_out (device int32 [B][Tf of the push]) takes the chosen stage counts");
    if (min_nq < 0 || min_nq > e->arch.num_quantizers)
        return fail("fc_engine_set_floor_frames: min_nq lies in [0, num_quantizers = " + std::to_string(e->arch.num_quantizers) + "], got " +
                    std::to_string(min_nq));
    for (size_t b = 0; b < e->row_nq.size(); ++b)
        if (min_nq > e->row_nq[b])
            return fail("fc_engine_set_floor_frames: min_nq = " + std::to_string(min_nq) + " lies above the cap of row " + std::to_string(b) + " (" +
                        std::to_string(e->row_nq[b]) + " stages, fc_engine_set_row_nq)");
    e->floor.min_nq = min_nq;
    e->floor.nq_frames_out = n_q_frames_out;
    return 0;
}

int fc_engine_set_push_frame_nq(fc_engine* e, const int32_t* n_q_frames, int B, int Tfc, void* stream) {
    (void)stream;
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    if (!n_q_frames) { e->push_nq = fc_engine::FrameNq(); return 0; }
    if (B <= 0 || Tfc <= 0) return fail("fc_engine_set_push_frame_nq: a table holds at least one row of at least one frame");
    if (!e->row_nq.empty())
        return fail("fc_engine_set_push_frame_nq: per-row stage counts are set (fc_engine_set_row_nq): a push takes a count per row or per frame, not both");
    e->push_nq.table = n_q_frames; e->push_nq.B = B; e->push_nq.Tf = Tfc;
    return 0;
}

int fc_engine_set_frame_nq(fc_engine* e, const int32_t* n_q_frames, int B, int Tf, void* stream) {
    (void)stream;
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    if (!n_q_frames) { e->frame_nq = fc_engine::FrameNq(); return 0; }
    if (B <= 0 || Tf <= 0) return fail("fc_engine_set_frame_nq: a table holds at least one row of at least one frame");
    if (!e->row_nq.empty())
        return fail("fc_engine_set_frame_nq: per-row stage counts are set (fc_engine_set_row_nq): a call takes a count per row or per frame, not both");
    e->frame_nq.table = n_q_frames; e->frame_nq.B = B; e->frame_nq.Tf = Tf;
    return 0;
}

int fc_rvq_encode_rate(fc_engine* e, const float* x, int N, int n_q, int width, int64_t* codes, float* quantized, void* stream) {
    RvqTail a;
    if (rvq_hook_rows(e, "fc_rvq_encode_rate", x, codes, N, n_q, width, false, true, &a.B, &a.Tf)) return 1;
    a.x = x; a.codes = codes; a.n_q = n_q; a.width = width;
    a.quant = quantized; a.beam_sum = false; a.rate_sum = quantized != nullptr;      // one sum, from the chosen counts
    const fc::RagLen rows;                              // every row has Tf frames
    if (e->floor.on()) { a.floor_rows = &rows; a.serr = e->floor.stage_err_out; a.rerr = e->floor.row_err_out; a.subq = e->floor.subq_out; }
    else { a.rate_rows = &rows; a.serr = e->rate.stage_err_out; a.rerr = e->rate.row_err_out; }
    return rvq_hook_launch(e, "fc_rvq_encode_rate", a, nullptr, (hipStream_t)stream);
}

int fc_rvq_encode(fc_engine* e, const float* x, int N, int n_q, int64_t* codes, float* quantized, void* workspace,
                  size_t workspace_bytes, void* stream) {
    // with per-row stage counts for B rows (fc_engine_set_row_nq) the N rows are B utterances of N / B frames each
    int B = 0, Tf = 0;
    if (rvq_hook_rows(e, "fc_rvq_encode", x, codes, N, n_q, 1, false, false, &B, &Tf)) return 1;
    int* q0map = nullptr;
    if (e->arch.q0_ds_ratio > 1) {      // the rows are ONE utterance of N frames; the stage-0 source-row table lives in the caller's workspace
        if (Tf < 2) return fail("quantizer_conf.q0_ds_ratio > 1 needs at least 2 frames");
        if (!workspace || workspace_bytes < (size_t)N * sizeof(int)) return fail("fc_rvq_encode with q0_ds_ratio > 1 needs a workspace of N * 4 bytes");
        q0map = (int*)workspace;
        HIP_TRY(fc::launch_q0_map(q0map, B, Tf, (hipStream_t)stream));
    }
    HIP_TRY(fc::launch_rvq_encode(x, N, e->cdim(), e->arch.codebook_size, n_q, e->cb, e->cb_frag, e->enorm, codes, quantized,
                                  nullptr, nullptr, Tf, (hipStream_t)stream, q0map, row_nq_table(e)));
    return 0;
}

int fc_q0_source_frames(int Tf, int32_t* frames) {
    if (Tf < 2 || !frames) return fail("fc_q0_source_frames: Tf >= 2 and a host buffer of Tf entries");
    for (int t = 0; t < Tf; ++t) frames[t] = fc::q0_source_frame(t, Tf);
    return 0;
}

int fc_layer_out_len(const fc_engine* e, const char* prefix, int T) {
    if (!e || !prefix) return -1;
    auto it = e->by_prefix.find(prefix);
    if (it == e->by_prefix.end() || it->second->c2d > 0) return -1;
    return conv_geom(*it->second, T).Tout;
}

namespace {
// fc_layer2d_forward / fc_layer2d_out_shape: one 2-D layer through the drivers' own run_conv2d / run_convtr2d (dry: shape and workspace only)
struct Layer2dRef { const ConvLayer* L = nullptr; int stage = -1; };      // stage >= 0: decoder convtr of that stage
int find_layer2d(const fc_engine* e, const char* prefix, Layer2dRef* r) {
    if (!e || !prefix) return fail("null argument");
    if (e->arch.model_type != 1) return fail("fc_layer2d_forward: the engine is not an STFT-domain codec (model_type 1)");
    for (size_t s = 0; s < e->dec_stages.size(); ++s)
        if (e->dec_stages[s].resample.prefix == prefix) { r->L = &e->dec_stages[s].resample; r->stage = (int)s; return 0; }
    auto it = e->by_prefix.find(prefix);
    if (it == e->by_prefix.end()) return fail(std::string("unknown layer ") + prefix);
    if (it->second->c2d == 0) return fail(std::string("layer ") + prefix + " is a 1-D layer: use fc_layer_forward");
    r->L = it->second;
    return 0;
}

int layer2d(fc_engine* e, Ctx& cx, const Layer2dRef& r, const float* x0, const float* aff0, const float* x1, const float* aff1, int F, int T,
            int apply_elu, int out_halo, float* y, int64_t* shape) {
    const ConvLayer& L = *r.L;
    const int B = cx.B, C = L.c2d, h = e->halo2;
    if (F <= 0 || T <= 0 || B <= 0) return fail("bad argument");
    if (out_halo != 0 && out_halo != h) return fail("fc_layer2d_forward: out_halo must be 0 or the engine's halo (" + std::to_string(h) + ")");
    if (r.stage >= 0 && !apply_elu) return fail("fc_layer2d_forward: a decoder convtr always follows its ELU (apply_elu = 1)");
    if (r.stage < 0 && F + (L.kf - L.sf) < L.kf) return fail("fc_layer2d_forward: fewer frequency rows than the kernel");
    if (r.stage < 0 && x1 && !L.dual) return fail("fc_layer2d_forward: " + L.prefix + " is planned for one source (its staging has no room for two)");
    // the inputs, frequency-major with reflected halo rows, in buffers of this workspace (as the drivers hand them over)
    Act2 a[2];
    const float* xs[2] = {x0, x1};
    const float* affs[2] = {aff0, aff1};
    for (int i = 0; i < 2; ++i) {
        if (i == 1 && !x1) break;
        a[i].C = C; a[i].F = F; a[i].T = T; a[i].halo = h;
        a[i].buf = cx.alloc<float>((size_t)B * (F + 2 * h) * C * T);
        a[i].aff = const_cast<float*>(affs[i]);
        a[i].normed = affs[i] != nullptr;
        cx.launch("input relayout", L.prefix.c_str(), [&] { return fc::launch_feats_relayout(a[i].buf, const_cast<float*>(xs[i]), B, C, F, T, h, 0, cx.st); });
        cx.launch("halo rows", L.prefix.c_str(), [&] { return fc::launch_halo_rows(a[i].buf, B, F, h, C, T, 0, cx.st); });
    }
    const Act2* p1 = x1 ? &a[1] : nullptr;
    Act2 o = r.stage >= 0 ? run_convtr2d(e, cx, L, e->dec_up_phases[r.stage], a[0], p1, r.stage + 1 == (int)e->dec_stages.size(), out_halo)
                          : run_conv2d(e, cx, L, a[0], p1, apply_elu, out_halo);
    const int Fh = o.F + 2 * o.halo;
    shape[0] = o.C; shape[1] = Fh; shape[2] = o.T;
    // the pending GroupNorm affine over every row (halo rows included), then the reference's [B][C][F][T]
    float* fin = cx.alloc<float>((size_t)B * Fh * o.C * o.T);
    cx.launch("output affine", L.prefix.c_str(), [&] { return fc::launch_combine2d(o.buf, o.aff, 0, nullptr, nullptr, 0, 0, 1.f, B, Fh, o.C, o.T, fin, 0, cx.st, 0); });
    cx.launch("output relayout", L.prefix.c_str(), [&] { return fc::launch_feats_relayout(fin, y, B, o.C, Fh, o.T, 0, 1, cx.st); });
    return cx.err;
}
}  // namespace

int fc_layer2d_out_shape(const fc_engine* ce, const char* prefix, int B, int F, int T, int out_halo, int64_t* dims) {
    fc_engine* e = const_cast<fc_engine*>(ce);
    Layer2dRef r;
    if (find_layer2d(e, prefix, &r)) return 1;
    if (!dims) return fail("null argument");
    if (out_halo == -1) { dims[0] = e->halo2; return 0; }
    // the workspace of the largest call form: one or two sources, with or without affines, with or without ELU (a dry run of each; the
    // pointers only mark presence, nothing is dereferenced)
    const float* mark = reinterpret_cast<const float*>(&dims[0]);
    size_t need = 0;
    int ok = 0;
    for (int form = 0; form < 8; ++form) {
        const bool two = form & 1, aff = form & 2, elu = form & 4;
        Ctx cx = dry_ctx(e, B);
        int64_t shape[3];
        const std::string keep = g_err;
        if (layer2d(e, cx, r, mark, aff ? mark : nullptr, two ? mark : nullptr, (two && aff) ? mark : nullptr, F, T, elu, out_halo, nullptr, shape)) {
            g_err = keep;
            continue;
        }
        if (!ok++) { dims[0] = shape[0]; dims[1] = shape[1]; dims[2] = shape[2]; }
        need = std::max(need, cx.off);
    }
    if (!ok) {                                        // no form is valid: report why the single-source ELU form is not
        Ctx cx = dry_ctx(e, B);
        int64_t shape[3];
        layer2d(e, cx, r, mark, nullptr, nullptr, nullptr, F, T, 1, out_halo, nullptr, shape);
        return 1;
    }
    dims[3] = (int64_t)(need + 4096);
    dims[4] = r.L->c2d;
    return 0;
}

int fc_layer2d_forward(fc_engine* e, const char* prefix, const float* x0, const float* aff0, const float* x1, const float* aff1, int B, int F,
                       int T, int apply_elu, int out_halo, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!x0 || !y || (aff1 && !x1)) return fail("bad argument");
    Layer2dRef r;
    if (find_layer2d(e, prefix, &r)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    int64_t shape[3];
    return layer2d(e, cx, r, x0, aff0, x1, aff1, F, T, apply_elu, out_halo, y, shape);
}

namespace {
// fc_freq_synthesis / fc_freq_synthesis_size: the host-side refusals (they need the architecture only)
int freq_synthesis_check(const fc_engine* e, int B, int C, int F, int Tp, int out_len) {
    if (!e) return fail("null argument");
    const fc_arch& a = e->arch;
    if (a.model_type != 1) return fail("fc_freq_synthesis: the engine is not an STFT-domain codec (model_type 1)");
    if (B <= 0) return fail("bad argument");
    if (C != a.input_channels)
        return fail("fc_freq_synthesis: dec has " + std::to_string(C) + " channels, the decoder's output has " + std::to_string(a.input_channels));
    if (F != a.n_fft / 2 + 1)
        return fail("fc_freq_synthesis: dec has " + std::to_string(F) + " frequency rows, n_fft / 2 + 1 is " + std::to_string(a.n_fft / 2 + 1));
    if (Tp < 2) return fail("fc_freq_synthesis: the inverse STFT needs at least 2 frames, got " + std::to_string(Tp));
    const long long full = (long long)a.stft_hop * (Tp - 1);
    if (out_len < 1 || out_len > full)
        return fail("fc_freq_synthesis: out_len " + std::to_string(out_len) + " is outside [1, stft_hop * (frames - 1)] = [1, " + std::to_string(full) + "]");
    return 0;
}

// dec [B][C][F][Tp] -> the engine's frequency-major rows (halo 0, as run_decoder_2d's last conv leaves them) -> run_synthesis_2d
int freq_synthesis(fc_engine* e, Ctx& cx, const float* dec, const float* aff, const float* scale, int Tp, int out_len, float* wav, float* spec_out) {
    const fc_arch& a = e->arch;
    const int B = cx.B, C = a.input_channels, F = a.n_fft / 2 + 1;
    Act2 last;
    last.C = C; last.F = F; last.T = Tp; last.halo = 0;
    last.buf = cx.alloc<float>((size_t)B * F * C * Tp);
    last.aff = const_cast<float*>(aff);
    last.normed = aff != nullptr;
    cx.launch("input relayout", "", [&] { return fc::launch_feats_relayout(last.buf, const_cast<float*>(dec), B, C, F, Tp, 0, 0, cx.st); });
    float* spec = nullptr;
    run_synthesis_2d(e, cx, last, scale, out_len, wav, &spec);
    if (spec_out)
        cx.launch("copy", "spectrum", [&] { return hipMemcpyAsync(spec_out, spec, (size_t)B * 2 * F * Tp * sizeof(float), hipMemcpyDeviceToDevice, cx.st); });
    return cx.err;
}
}  // namespace

int fc_freq_synthesis_size(const fc_engine* ce, int B, int C, int F, int Tp, int out_len, size_t* workspace_bytes) {
    fc_engine* e = const_cast<fc_engine*>(ce);
    if (freq_synthesis_check(e, B, C, F, Tp, out_len)) return 1;
    if (!workspace_bytes) return fail("null argument");
    Ctx cx = dry_ctx(e, B);
    if (freq_synthesis(e, cx, nullptr, nullptr, nullptr, Tp, out_len, nullptr, nullptr)) return 1;
    *workspace_bytes = cx.off + 4096;
    return 0;
}

int fc_freq_synthesis(fc_engine* e, const float* dec, const float* aff, const float* scale, int B, int C, int F, int Tp, int out_len, float* wav,
                      float* spec, void* workspace, size_t workspace_bytes, void* stream) {
    if (freq_synthesis_check(e, B, C, F, Tp, out_len)) return 1;
    if (!dec || !wav) return fail("bad argument");
    if (check_ready(e)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    return freq_synthesis(e, cx, dec, aff, scale, Tp, out_len, wav, spec);
}

namespace {
fc::Src hook_src(const float* x, const float* aff, const float* div) {
    fc::Src s;
    s.ptr = x; s.aff = aff; s.div = div;
    s.used = x ? ((aff || div) ? 3 : 1) : 0;
    return s;
}
}  // namespace

// the host-side refusals of fc_layer_forward_src (they need the plan only, no weights)
static int layer_src_check(const fc_engine* e, const char* prefix, const float* x0, const float* aff0, const float* div0, const float* x1,
                           const float* aff1, int B, int T, const ConvLayer** out) {
    if (!e || !prefix || !x0 || B <= 0 || T <= 0 || (aff1 && !x1) || (aff0 && div0)) return fail("bad argument");
    auto it = e->by_prefix.find(prefix);
    if (it == e->by_prefix.end()) return fail(std::string("unknown layer ") + prefix);
    const ConvLayer& L = *it->second;
    if (L.c2d > 0)      // a Conv2d planned over kf * C channels of frequency-major rows: the 1-D path would read kf times the input
        return fail(std::string("layer ") + prefix + " is a 2-D layer of the STFT-domain codec: use fc_layer2d_forward");
    if (x1 && !L.dual) return fail("fc_layer_forward_src: " + L.prefix + " is planned for one source (its staging has no room for two)");
    if (div0 && &L != &e->enc_first) return fail("fc_layer_forward_src: div0 is the encoder's first conv's volume scale (" + e->enc_first.prefix + ")");
    *out = &L;
    return 0;
}

int fc_layer_forward_src(fc_engine* e, const char* prefix, const float* x0, const float* aff0, const float* div0, const float* x1,
                         const float* aff1, int B, int T, int apply_elu, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    const ConvLayer* L = nullptr;
    if (layer_src_check(e, prefix, x0, aff0, div0, x1, aff1, B, T, &L)) return 1;
    if (!y) return fail("bad argument");
    if (check_ready(e)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    Act o = run_conv(e, cx, *L, hook_src(x0, aff0, div0), hook_src(x1, aff1, nullptr), apply_elu, T);
    if (cx.err) return 1;
    HIP_TRY(fc::launch_combine(src_of(o), fc::Src(), 0, 1.f, nullptr, B, o.C, o.T, o.T, y, (long long)o.C * o.T, o.T, 1, cx.st));
    return 0;
}

int fc_layer_forward(fc_engine* e, const char* prefix, const float* x, int B, int T, int apply_elu, float* y,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return fc_layer_forward_src(e, prefix, x, nullptr, nullptr, nullptr, nullptr, B, T, apply_elu, y, workspace, workspace_bytes, stream);
}

int fc_resblock_forward_src(fc_engine* e, const char* prefix, const float* x0, const float* aff0, const float* x1, const float* aff1, int B,
                            int T, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !prefix || !x0 || !y || B <= 0 || T <= 0 || (aff1 && !x1)) return fail("bad argument");
    auto it = e->res_by_prefix.find(prefix);
    if (it == e->res_by_prefix.end()) return fail(std::string("unknown residual block ") + prefix);
    const fc_engine::ResBlock& R = *it->second;
    if (x1 && !R.shortcut.dual)
        return fail(std::string("fc_resblock_forward_src: block ") + prefix + " is planned for one source (its staging has no room for two)");
    if (check_ready(e)) return 1;
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    fc_engine::Stage one;
    one.res.push_back(R);
    Act sc, b3;
    run_resblocks(e, cx, Pass(), one, hook_src(x0, aff0, nullptr), hook_src(x1, aff1, nullptr), T, &sc, &b3);
    if (cx.err) return 1;
    HIP_TRY(fc::launch_combine(src_of(sc), src_of(b3), 0, 1.f, nullptr, B, sc.C, T, T, y, (long long)sc.C * T, T, 1, cx.st));
    return 0;
}

int fc_resblock_forward(fc_engine* e, const char* prefix, const float* x, int B, int T, float* y, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return fc_resblock_forward_src(e, prefix, x, nullptr, nullptr, nullptr, B, T, y, workspace, workspace_bytes, stream);
}

int fc_lstm_forward(fc_engine* e, const char* prefix, const float* x, int B, int T, float* y, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!prefix || !x || !y || B <= 0 || T <= 0) return fail("bad argument");
    auto it = e->lstm_by_prefix.find(prefix);
    if (it == e->lstm_by_prefix.end()) return fail(std::string("unknown lstm ") + prefix);
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    Act in; in.raw = const_cast<float*>(x); in.C = it->second->H; in.T = T;
    Act o = run_lstm(e, cx, *it->second, in, T);
    if (cx.err) return 1;
    fc::Src s1;
    if (e->arch.lstm_skip) s1 = src_of(in);
    HIP_TRY(fc::launch_combine(src_of(o), s1, 0, 1.f, nullptr, B, o.C, T, T, y, (long long)o.C * T, T, 1, cx.st));
    return 0;
}

int fc_seq_forward(fc_engine* e, const char* prefix, const float* x, int B, int T, float* y, void* workspace,
                   size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!prefix || !x || !y || B <= 0 || T <= 0) return fail("bad argument");
    auto it = e->tf_by_prefix.find(prefix);
    if (it == e->tf_by_prefix.end()) return fail(std::string("unknown transformer ") + prefix);
    Ctx cx = make_ctx(e, B, workspace, workspace_bytes, stream);
    Act in; in.raw = const_cast<float*>(x); in.C = it->second->C; in.T = T;
    Act o = run_transformer(e, cx, *it->second, in, T);
    if (cx.err) return 1;
    fc::Src s1;
    if (e->arch.lstm_skip) s1 = src_of(in);           // TransformerEncoder(skip=res_seq): after_norm(x) + input
    HIP_TRY(fc::launch_combine(src_of(o), s1, 0, 1.f, nullptr, B, o.C, T, T, y, (long long)o.C * T, T, 1, cx.st));
    return 0;
}

int fc_engine_status(fc_engine* e, unsigned* flags) {
    if (!e) return fail("null engine");
    unsigned f = 0;
    if (e->status_host) {
        if (e->status_host[FC_STATUS_LSTM_TIMEOUT]) f |= FC_STATUS_FLAG_LSTM_TIMEOUT;
        if (e->status_host[FC_STATUS_BAD_CODE]) f |= FC_STATUS_FLAG_BAD_CODE;
        if (e->status_host[FC_STATUS_BAD_LENGTH]) f |= FC_STATUS_FLAG_BAD_LENGTH;
    }
    if (flags) *flags = f;
    if (!e->finalized) return 0;
    return consume_status(e);
}

int fc_overlap_add(const float* const* frames, const int* lens, int n_frames, int B, int frame0_len, int stride, int out_len,
                   float* out, void* stream) {
    if (!frames || !lens || !out || n_frames <= 0 || B <= 0 || frame0_len <= 0 || stride <= 0 || out_len <= 0) return fail("bad argument");
    HIP_TRY(fc::launch_overlap_add(frames, lens, n_frames, B, frame0_len, stride, out_len, out, (hipStream_t)stream));
    return 0;
}

size_t fc_codec_json_bound(int n_q, int len) { return (size_t)(n_q > 0 ? n_q : 0) * ((size_t)(len > 0 ? len : 0) * 22 + 4) + 8; }

int fc_format_codec_json(const int64_t* codes, int n_q, int B, int T, int b, int len, char* out, size_t cap, size_t* written) {
    if (!codes || !out || !written || n_q <= 0 || B <= 0 || T <= 0 || b < 0 || b >= B || len < 0 || len > T) return fail("bad argument");
    if (cap < fc_codec_json_bound(n_q, len)) return fail("output buffer too small (fc_codec_json_bound)");
    char* p = out;
    *p++ = '['; *p++ = '[';
    for (int q = 0; q < n_q; ++q) {
        if (q) { *p++ = ','; *p++ = ' '; }
        *p++ = '[';
        const int64_t* row = codes + ((size_t)q * B + b) * T;
        for (int t = 0; t < len; ++t) {
            if (t) { *p++ = ','; *p++ = ' '; }
            long long v = row[t];
            if (v < 0) { *p++ = '-'; v = -v; }
            char tmp[24];
            int n = 0;
            do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
            while (n) *p++ = tmp[--n];
        }
        *p++ = ']';
    }
    *p++ = ']'; *p++ = ']';
    *written = (size_t)(p - out);
    return 0;
}

int fc_write_wav_pcm16(const char* path, const float* wav, int n, int sample_rate, int rescale) {
    if (!path || !wav || n < 0 || sample_rate <= 0) return fail("bad argument");
    const float limit = 0.99f;
    float mx = 0.f;
    for (int i = 0; i < n; ++i) { const float a = fabsf(wav[i]); if (a > mx) mx = a; }
    // torch: wav * min(limit / mx, 1), else clamp(-limit, limit).  `limit / mx` with a 0-dim tensor mx is Tensor.__rtruediv__ =
    // mx.reciprocal() * limit, two fp32 roundings (1 ulp off limit / mx for about a quarter of all peaks)
    float mul = 1.f;
    if (rescale && mx > 0.f) { const float r = (1.0f / mx) * limit; mul = r < 1.f ? r : 1.f; }
    std::vector<int16_t> pcm((size_t)n);
    for (int i = 0; i < n; ++i) {
        float v = wav[i];
        if (rescale) v = v * mul;
        else v = v < -limit ? -limit : (v > limit ? limit : v);
        float s = nearbyintf(v * 32768.0f);            // torch.round: half to even
        s = s < -32768.f ? -32768.f : (s > 32767.f ? 32767.f : s);
        pcm[i] = (int16_t)s;
    }
    FILE* f = fopen(path, "wb");
    if (!f) return fail(std::string("cannot open ") + path);
    const uint32_t data_bytes = (uint32_t)n * 2u, riff = 36u + data_bytes, fmt_len = 16u, sr = (uint32_t)sample_rate, byte_rate = sr * 2u;
    const uint16_t pcm_tag = 1, ch = 1, align = 2, bits = 16;
    bool ok = fwrite("RIFF", 1, 4, f) == 4 && fwrite(&riff, 4, 1, f) == 1 && fwrite("WAVEfmt ", 1, 8, f) == 8 && fwrite(&fmt_len, 4, 1, f) == 1 &&
              fwrite(&pcm_tag, 2, 1, f) == 1 && fwrite(&ch, 2, 1, f) == 1 && fwrite(&sr, 4, 1, f) == 1 && fwrite(&byte_rate, 4, 1, f) == 1 &&
              fwrite(&align, 2, 1, f) == 1 && fwrite(&bits, 2, 1, f) == 1 && fwrite("data", 1, 4, f) == 4 && fwrite(&data_bytes, 4, 1, f) == 1 &&
              (n == 0 || fwrite(pcm.data(), 2, (size_t)n, f) == (size_t)n);
    ok = (fclose(f) == 0) && ok;
    return ok ? 0 : fail(std::string("short write to ") + path);
}

int fc_debug_freq_features(void* dev_buf, size_t cap_bytes, int mode) {
    if (mode < 0 || mode > 2 || (mode != 0 && !dev_buf)) return fail("fc_debug_freq_features: mode 0 (off), 1 (capture) or 2 (override) with a device buffer");
    g_feat_hook.buf = (float*)dev_buf; g_feat_hook.cap = cap_bytes; g_feat_hook.mode = mode;
    return 0;
}

// Host-side description of the conv kernel's operand layout for one chunk shape (kernels.hip: conv_pack_index / conv_koff_table); no GPU work.
int fc_debug_conv_layout(int k, int stride, int dil, int CC, int BM, int BN, int row, int* info /* [6] */, int* pack_index, size_t pack_cap,
                         int* koff, size_t koff_cap) {
    if (k < 1 || stride < 1 || dil < 1 || CC < 1 || BM < 1 || BN < 1 || !info) return fail("fc_debug_conv_layout: bad shape");
    const std::vector<int> t = fc::conv_koff_table(k, stride, dil, CC, BN, row ? 1 : 0);
    const int slabW = (BN - 1) * stride + (k - 1) * dil + 1;
    int PL = (slabW + stride - 1) / stride, rowStride = PL * stride;
    if (row) { rowStride = (slabW + 3) & ~3; PL = rowStride; }
    info[0] = fc::conv_quad(CC) ? 1 : 0; info[1] = fc::conv_wbuf_floats(k, CC, BM); info[2] = (int)t.size();
    info[3] = rowStride; info[4] = PL; info[5] = slabW;
    if (pack_index) {
        if (pack_cap < (size_t)k * CC * BM) return fail("fc_debug_conv_layout: pack_index buffer too small");
        for (int kk = 0; kk < k; ++kk)
            for (int cl = 0; cl < CC; ++cl)
                for (int mm = 0; mm < BM; ++mm) pack_index[((size_t)kk * CC + cl) * BM + mm] = (int)fc::conv_pack_index(k, CC, BM, kk, cl, mm);
    }
    if (koff) {
        if (koff_cap < t.size()) return fail("fc_debug_conv_layout: koff buffer too small");
        for (size_t i = 0; i < t.size(); ++i) koff[i] = t[i];
    }
    return 0;
}

int fc_debug_timeline(unsigned long long* dst) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(fc::debug_timeline(dst));
    return 0;
}

// ---- streaming session (include/funcodec_amd.h) ---------------------------------------------------------------------------------
size_t fc_stream_state_bytes(const fc_engine* ce, int B) {
    fc_engine* e = const_cast<fc_engine*>(ce);
    if (!e || B <= 0 || stream_refusal(e)) return 0;
    Session tmp;
    stream_layout(e, B, &tmp);
    return tmp.state_floats * sizeof(float);
}

size_t fc_seqstream_state_bytes(const fc_engine* ce, int B, int max_frames) {
    fc_engine* e = const_cast<fc_engine*>(ce);
    if (!e || B <= 0 || max_frames <= 0 || stream_refusal(e, max_frames)) return 0;
    Session tmp;
    tmp.max_frames = max_frames;
    stream_layout(e, B, &tmp);
    return tmp.state_floats * sizeof(float);
}

}  // extern "C"

namespace {

// What fc_stream_create and fc_slots_create share: the argument checks and the layout of the caller's state.  rows_error: why the row
// count is refused, or null; `first`: what the kind calls the first push of an utterance; state_rule: its wording of the state rule.
int session_create(Session* s, fc_engine* e, const void* out, int rows, const char* rows_error, int max_chunk_samples, int n_q, void* state,
                   size_t state_bytes, const char* first, const char* state_rule, int max_frames = 0) {
    if (!e || !out) return fail("null argument");
    if (!e->finalized) return fail("engine not finalized");
    if (const char* why = stream_refusal(e, max_frames)) return fail(why);
    if (rows_error) return fail(rows_error);
    if (n_q < 1 || n_q > e->arch.num_quantizers) return fail("n_q out of range");
    s->e = e; s->B = rows; s->n_q = n_q; s->max_chunk = max_chunk_samples; s->max_frames = max_frames;
    stream_layout(e, rows, s);
    if (max_frames > 0 && max_frames < std::max(s->enc_min_first / total_hop(e), s->dec_min_first))
        return fail("max_frames must hold the first push of an utterance: at least " + std::to_string(std::max(s->enc_min_first / total_hop(e), s->dec_min_first)) +
                    " frames for this net");
    const int need = std::max(s->enc_min_first, s->dec_min_first * total_hop(e));
    if (max_chunk_samples < need)
        return fail(std::string("max_chunk_samples must hold the ") + first + " push of an utterance: at least " + std::to_string(need) + " samples for this net");
    if (!state || ((uintptr_t)state & 15) || state_bytes < s->state_floats * sizeof(float)) return fail(state_rule);
    s->state = (float*)state;
    s->ones.assign(rows, 1.f);
    return record_layout(e, s);
}

// The two fc_*_lstm_forward hooks: the SLSTM stage of a push alone (lstm.py:22-28 without the skip) on the session's LSTM state of one
// side, exactly as a push runs it (run_lstm on the carried state; `steps`: a slot push).  x, y dev f32 [B][H][T].
const LstmBlock* lstm_hook_block(const Session& s, int decoder, bool args_ok) {
    const LstmBlock& lb = decoder ? s.e->dec_lstm : s.e->enc_lstm;
    if (!args_ok) { fail("bad argument"); return nullptr; }
    if (!lb.H) { fail("this net has no LSTM"); return nullptr; }
    return &lb;
}
int lstm_hook_run(const Session& s, Ctx& cx, const LstmBlock& lb, int decoder, const float* x, int T, const fc::RagLen* steps, float* y) {
    Act in; in.raw = const_cast<float*>(x); in.C = lb.H; in.T = T;
    Act out = run_lstm(s.e, cx, lb, in, T, lstm_state(s, decoder != 0), steps);
    cx.launch("copy", "y", [&] { return hipMemcpyAsync(y, out.raw, (size_t)s.B * lb.H * T * sizeof(float), hipMemcpyDeviceToDevice, cx.st); });
    return cx.err;
}

}  // namespace

extern "C" {

int fc_stream_create(fc_engine* e, int B, int max_chunk_samples, int n_q, void* state, size_t state_bytes, fc_stream** out) {
    std::unique_ptr<fc_stream> S(new fc_stream);
    if (session_create(S.get(), e, out, B, B <= 0 ? "bad batch size" : nullptr, max_chunk_samples, n_q, state, state_bytes, "first",
                       "stream state: a 16-byte aligned device buffer of fc_stream_state_bytes() bytes"))
        return 1;
    S->enc_done = true; S->enc_pushes = -1; S->dec_pushes = -1;     // unusable until the first fc_stream_reset
    *out = S.release();
    return 0;
}

int fc_seqstream_create(fc_engine* e, int B, int max_chunk_samples, int n_q, int max_frames, void* state, size_t state_bytes, fc_stream** out) {
    if (max_frames <= 0) return fail("max_frames must be positive: the most frames an utterance of this session may hold per side");
    std::unique_ptr<fc_stream> S(new fc_stream);
    if (session_create(S.get(), e, out, B, B <= 0 ? "bad batch size" : nullptr, max_chunk_samples, n_q, state, state_bytes, "first",
                       "stream state: a 16-byte aligned device buffer of fc_seqstream_state_bytes() bytes", max_frames))
        return 1;
    S->enc_done = true; S->enc_pushes = -1; S->dec_pushes = -1;     // unusable until the first fc_stream_reset
    *out = S.release();
    return 0;
}

void fc_stream_destroy(fc_stream* s) { delete s; }

int fc_stream_min_first(const fc_stream* s, int decode) { return s ? (decode ? s->dec_min_first : s->enc_min_first) : 0; }

int fc_graphstream_set(fc_stream* S, int on) {
    if (!S) return fail("null stream");
    if (on && S->max_frames > 0)
        return fail("graph replay is not available for a lock-step session opened with max_frames: its key / value cache position is a launch argument that "
                    "changes with every push; a slot session opened with max_frames reads every row's position from device memory and replays");
    return session_set_graph(S, on);
}
int fc_graphstream_enabled(const fc_stream* S) { return S && S->graph_on ? 1 : 0; }
int fc_graphstream_counts(const fc_stream* S, int64_t counts[4]) { return session_graph_counts(S, counts); }

size_t fc_stream_workspace_bytes(const fc_stream* S) {
    if (!S) return 0;
    const int Tf = ceil_div_i(S->max_chunk, total_hop(S->e));
    // the largest encode push.  A first push and a later one stage the same columns: sized as push 0, a final one (the extra padding)
    Ctx ce = dry_ctx(S->e, S->B);
    stream_encode_pass(S, ce, 0, nullptr, S->max_chunk, true, nullptr, nullptr, nullptr);
    // the largest decode push: decode_codes, with the first buffer as wide as decode_emb's
    Ctx cd = dry_ctx(S->e, S->B);
    stream_decode_pass(S, cd, 0, decoder_input_codes(S->e, cd, nullptr, Tf, S->n_q, nullptr, nullptr, true), Tf, 1, nullptr);
    return std::max(ce.off, cd.off) + 4096;
}

int fc_stream_reset(fc_stream* S, const float* scale, void* stream) {
    if (!S) return fail("null stream");
    if (check_ready(S->e)) return 1;                  // a session broken by a failed push is what reset repairs
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(fc::launch_zero_fill(S->state, S->carried_floats, st));      // not the key / value caches: they are written before they are read
    if (scale) HIP_TRY(hipMemcpyAsync(S->state, scale, (size_t)S->B * sizeof(float), hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemcpyAsync(S->state, S->ones.data(), (size_t)S->B * sizeof(float), hipMemcpyHostToDevice, st));
    S->enc_pushes = 0; S->dec_pushes = 0; S->enc_frames = 0; S->dec_frames = 0; S->enc_done = false; S->broken = false;
    return 0;
}

int fc_stream_encode(fc_stream* S, const float* wav, int Tc, int final, int64_t* codes, float* quantized, float* enc_out, int* n_frames,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (stream_ready(S)) return 1;
    fc_engine* e = S->e;
    const int hop = total_hop(e);
    if (!wav || !codes || !n_frames) return fail("bad argument");
    if (S->enc_pushes < 0) return fail("streaming encode: fc_stream_reset first");
    if (S->enc_done) return fail("streaming encode: the utterance took its final push; fc_stream_reset starts the next one");
    if (Tc < 1 || Tc > S->max_chunk) return fail("streaming encode: a push holds 1 .. max_chunk_samples samples, got " + std::to_string(Tc));
    if (!final && Tc % hop != 0)
        return fail("streaming encode: every push but the final one must be a multiple of the hop (" + std::to_string(hop) + " samples), got " +
                    std::to_string(Tc) + "; it is not padded silently");
    if (S->enc_pushes == 0 && Tc < S->enc_min_first)
        return fail("streaming encode: the first push of an utterance must hold at least " + std::to_string(S->enc_min_first) +
                    " samples (the offline call's reflected left padding spans them); shorter utterances go through the offline call");
    const int Tfc = final ? frames_for(e, Tc) : Tc / hop;
    if (frames_fit(S, false, Tfc)) return 1;
    if (counts_check_encode(e, "fc_stream_encode", S->B, S->n_q, true)) return 1;
    // the first push of an utterance (reflection staging) and the final one (extra padding) are one-offs: never cached
    const Session::GraphKey key = graph_key(*S, kFormEncode, Tc, S->enc_pushes, 0, {wav, codes, quantized, enc_out}, workspace, workspace_bytes, stream);
    S->broken = true;                                   // until the whole push is enqueued: a failure in between leaves mixed carries
    if (session_push(S, S->enc_pushes > 0 && !final ? &key : nullptr, workspace, workspace_bytes, stream, no_eager_part,
                     [&](Ctx& cx, bool) { return stream_encode_pass(S, cx, S->enc_pushes, wav, Tc, final != 0, codes, quantized, enc_out); }))
        return 1;
    S->broken = false;
    *n_frames = Tfc;
    S->enc_pushes++;
    S->enc_frames += Tfc;
    if (final) S->enc_done = true;
    return 0;
}

int fc_stream_decode_emb(fc_stream* S, const float* emb, int Tfc, int use_scale, float* wav, void* workspace, size_t workspace_bytes, void* stream) {
    if (stream_ready(S)) return 1;
    if (!emb || !wav) return fail("bad argument");
    if (stream_decode_check(S, Tfc)) return 1;
    return stream_decode_push(S, kFormDecodeEmb, emb, Tfc, use_scale, wav, nullptr, workspace, workspace_bytes, stream);
}

int fc_stream_decode_codes(fc_stream* S, const int64_t* codes, int Tfc, int use_scale, float* wav, float* emb_out, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (stream_ready(S)) return 1;
    if (!codes || !wav) return fail("bad argument");
    if (stream_decode_check(S, Tfc)) return 1;
    if (counts_check_decode(S->e, "fc_stream_decode_codes", S->B, Tfc, S->n_q, true)) return 1;
    return stream_decode_push(S, kFormDecodeCodes, codes, Tfc, use_scale, wav, emb_out, workspace, workspace_bytes, stream);
}

// Test hook: the SLSTM stage of a push alone, continuing the recurrence the session's encoder (decoder = 0) or decoder (decoder = 1)
// LSTM state holds.
int fc_stream_lstm_forward(fc_stream* S, int decoder, const float* x, int T, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (stream_ready(S)) return 1;
    const LstmBlock* lb = lstm_hook_block(*S, decoder, x && y && T > 0);
    if (!lb) return 1;
    if (S->enc_pushes < 0) return fail("streaming: fc_stream_reset first");
    Ctx cx = make_ctx(S->e, S->B, workspace, workspace_bytes, stream);
    S->broken = true;
    if (lstm_hook_run(*S, cx, *lb, decoder, x, T, nullptr, y)) return 1;
    S->broken = false;
    return 0;
}

// Test hook: the transformer stage of a push alone (TransformerEncoder.forward without the res_seq skip) on the session's key / value
// cache of one side; it advances that side's frame count as a push does.  x, y dev f32 [B][C][T].
int fc_seqstream_forward(fc_stream* S, int decoder, const float* x, int T, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (stream_ready(S)) return 1;
    if (!x || !y || T <= 0) return fail("bad argument");
    const TfBlock& tb = decoder ? S->e->dec_tf : S->e->enc_tf;
    if (!tb.C || S->max_frames <= 0) return fail("this session has no transformer bottleneck (fc_seqstream_create opens one)");
    if (S->enc_pushes < 0) return fail("streaming: fc_stream_reset first");
    if (frames_fit(S, decoder != 0, T)) return 1;
    Ctx cx = make_ctx(S->e, S->B, workspace, workspace_bytes, stream);
    const TfCache kv = tf_cache(*S, decoder != 0, decoder ? S->dec_frames : S->enc_frames);
    Act in; in.raw = const_cast<float*>(x); in.C = tb.C; in.T = T;
    S->broken = true;
    Act out = run_transformer(S->e, cx, tb, in, T, &kv);
    cx.launch("copy", "y", [&] { return hipMemcpyAsync(y, out.raw, (size_t)S->B * tb.C * T * sizeof(float), hipMemcpyDeviceToDevice, cx.st); });
    if (cx.err) return 1;
    S->broken = false;
    (decoder ? S->dec_frames : S->enc_frames) += T;
    return 0;
}

// ---- slot session (include/funcodec_amd.h) --------------------------------------------------------------------------------------
size_t fc_slots_state_bytes(const fc_engine* e, int S) { return fc_stream_state_bytes(e, S); }
size_t fc_seqslots_state_bytes(const fc_engine* e, int S, int max_frames) { return fc_seqstream_state_bytes(e, S, max_frames); }

}  // extern "C"

namespace {
// fc_slots_create (max_frames = 0) and fc_seqslots_create: one slot session, with or without a key / value cache
int slots_create(fc_engine* e, int S, int max_chunk_samples, int n_q, int max_frames, void* state, size_t state_bytes, const char* state_rule,
                 fc_slots** out) {
    std::unique_ptr<fc_slots> Q(new fc_slots);
    if (session_create(Q.get(), e, out, S, (S <= 0 || S > 65535) ? "bad slot count (1 .. 65535)" : nullptr, max_chunk_samples, n_q, state, state_bytes,
                       "START", state_rule, max_frames))
        return 1;
    // the scale of a slot whose encoder has not started an utterance is 1: decode multiplies by it from the first push on
    HIP_TRY(hipMemcpy(state, Q->ones.data(), (size_t)S * sizeof(float), hipMemcpyHostToDevice));
    Q->enc_phase.assign(S, (char)fc_slots::Idle); Q->dec_phase.assign(S, (char)fc_slots::Idle);
    Q->push.assign((size_t)(max_frames > 0 ? 3 : 2) * S, 0);
    if (max_frames > 0) { Q->enc_frames.assign(S, 0); Q->dec_frames.assign(S, 0); }
    *out = Q.release();
    return 0;
}

// ---- the slot record (slots_kernels.h states it; include/funcodec_amd.h the calls) ----------------------------------------------
// what the host knows of one row of a session of either kind, as the record sees it
struct RowView { int enc_phase, dec_phase, enc_frames, dec_frames; };

// the argument rules export and import share, checked before anything else; `who` begins every message
int record_args(const Session& s, const std::string& who, int n, const int32_t* slots, const void* records, const void* meta) {
    if (!slots || !records || !meta) return fail(who + ": null argument");
    if (n < 1 || n > s.B) return fail(who + ": a call names 1 .. " + std::to_string(s.B) + " slots (the session's rows), got n = " + std::to_string(n));
    std::vector<char> seen(s.B, 0);
    for (int i = 0; i < n; ++i) {
        const int b = slots[i];
        if (b < 0 || b >= s.B) return fail(who + ": slot " + std::to_string(b) + ": out of range, this session has slots 0 .. " + std::to_string(s.B - 1));
        if (seen[b]) return fail(who + ": slot " + std::to_string(b) + ": named twice in one call");
        seen[b] = 1;
    }
    return 0;
}

int record_pitch(const Session& s, const std::string& who, int b, int enc_frames, int dec_frames, size_t pitch) {
    const size_t need = s.rec.floats(enc_frames, dec_frames);
    if (pitch < need)
        return fail(who + ": slot " + std::to_string(b) + ": pitch_floats = " + std::to_string(pitch) + " is too small, the slot's record holds " +
                    std::to_string(need) + " floats (fc_slotrec_floats)");
    return 0;
}

// the named slots (s.rec.refs[0 .. n), filled by the caller) in one copy, then the one launch
int record_launch(Session& s, const std::string& who, bool import, int n, float* records, size_t pitch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int frames = 0;
    for (int i = 0; i < n; ++i) frames = std::max(frames, std::max(s.rec.refs[i].enc_frames, s.rec.refs[i].dec_frames));
    const long long longest = std::max((long long)s.rec.max_len, (long long)s.rec.max_rows * fc::seq_cache_pitch(frames));
    // pageable memory that the next call overwrites: the runtime stages such a copy before it returns (slots_upload says why that holds)
    hipError_t er = hipMemcpyAsync(s.rec.refs_dev, s.rec.refs.data(), (size_t)n * sizeof(fc::SlotRef), hipMemcpyHostToDevice, st);
    if (er == hipSuccess)
        er = fc::launch_slot_record(import, s.state, s.rec.segs_dev, (int)s.rec.segs.size(), s.rec.refs_dev, n, records, pitch, longest, st);
    if (er != hipSuccess) return fail(who + ": slot record launch failed: " + hipGetErrorString(er));
    return 0;
}

// fc_slotrec_export and fc_slotrec_export_stream: both kinds of session are one Session with one layout; view(b): the row as its kind
// of session knows it.  The source is only read.
template <typename View>
int record_export(Session& s, const std::string& who, int enc_pushes, int dec_pushes, int n, const int32_t* slots, float* records, size_t pitch,
                  fc_slot_meta* meta, void* stream, View&& view) {
    if (record_args(s, who, n, slots, records, meta)) return 1;
    std::vector<fc_slot_meta> out(n);                   // a refused call changes nothing, the caller's meta included
    for (int i = 0; i < n; ++i) {
        const int b = slots[i];
        RowView v = view(b);
        if (v.enc_phase == fc_slots::Poisoned || v.dec_phase == fc_slots::Poisoned)
            return fail(who + ": slot " + std::to_string(b) + ": a push of this session failed after it had begun to write carries: the slot's state is "
                        "invalid and is not exported; START begins its next utterance");
        const bool enc_live = v.enc_phase == fc_slots::Running, dec_live = v.dec_phase == fc_slots::Running;
        const bool cached = s.max_frames > 0;
        fc_slot_meta& m = out[i];
        m.layout = s.rec.layout; m.enc_phase = v.enc_phase; m.dec_phase = v.dec_phase;
        m.enc_frames = cached && enc_live ? v.enc_frames : 0;
        m.dec_frames = cached && dec_live ? v.dec_frames : 0;
        if (record_pitch(s, who, b, m.enc_frames, m.dec_frames, pitch)) return 1;
        fc::SlotRef& r = s.rec.refs[i];
        r.slot = b; r.enc_frames = m.enc_frames; r.dec_frames = m.dec_frames;
        r.bits = (enc_pushes & 1) | ((dec_pushes & 1) << 1) | (enc_live ? fc::kSlotRecEncLive : 0) | (dec_live ? fc::kSlotRecDecLive : 0);
    }
    if (record_launch(s, who, false, n, records, pitch, stream)) return 1;
    std::copy(out.begin(), out.end(), meta);
    return 0;
}
}  // namespace

extern "C" {

size_t fc_slotrec_floats(const fc_slots* s, int enc_frames, int dec_frames) {
    if (!s || enc_frames < 0 || dec_frames < 0) return 0;
    const bool cached = s->max_frames > 0;
    return s->rec.floats(cached ? enc_frames : 0, cached ? dec_frames : 0);
}

int fc_slotrec_export(fc_slots* Q, int n, const int32_t* slots, float* records, size_t pitch_floats, fc_slot_meta* meta, void* stream) {
    if (slots_ready(Q)) return 1;
    const bool cached = Q->max_frames > 0;
    return record_export(*Q, "slot export", Q->enc_pushes, Q->dec_pushes, n, slots, records, pitch_floats, meta, stream, [&](int b) {
        return RowView{Q->enc_phase[b], Q->dec_phase[b], cached ? Q->enc_frames[b] : 0, cached ? Q->dec_frames[b] : 0};
    });
}

int fc_slotrec_export_stream(fc_stream* S, int n, const int32_t* rows, float* records, size_t pitch_floats, fc_slot_meta* meta, void* stream) {
    if (stream_ready(S)) return 1;                      // a broken stream is refused here
    if (S->enc_pushes < 0) return fail("stream export: fc_stream_reset first");
    // the common counters as phases: the encoder side runs from its first push to its final one, the decoder side has no final push
    const int enc_phase = S->enc_pushes == 0 ? fc_slots::Idle : S->enc_done ? fc_slots::Ended : fc_slots::Running;
    const int dec_phase = S->dec_pushes == 0 ? fc_slots::Idle : fc_slots::Running;
    return record_export(*S, "stream export", S->enc_pushes, S->dec_pushes, n, rows, records, pitch_floats, meta, stream,
                         [&](int) { return RowView{enc_phase, dec_phase, S->enc_frames, S->dec_frames}; });
}

int fc_slotrec_import(fc_slots* Q, int n, const int32_t* slots, const float* records, size_t pitch_floats, const fc_slot_meta* meta, void* stream) {
    if (slots_ready(Q)) return 1;
    const std::string who = "slot import";
    if (record_args(*Q, who, n, slots, records, meta)) return 1;
    const bool cached = Q->max_frames > 0;
    for (int i = 0; i < n; ++i) {
        const fc_slot_meta& m = meta[i];
        const std::string at = who + ": slot " + std::to_string(slots[i]) + ": ";
        const bool rec_cached = (m.layout & 1u) != 0;
        if (rec_cached && !cached)
            return fail(at + "the record holds a key / value cache and this session has none (fc_seqslots_create opens one, with max_frames); nothing was changed");
        if (!rec_cached && cached)
            return fail(at + "the record holds no key / value cache and this session has one (max_frames = " + std::to_string(Q->max_frames) +
                        "); nothing was changed");
        if (m.layout != Q->rec.layout)
            return fail(at + "the record's layout " + std::to_string(m.layout) + " is not this session's " + std::to_string(Q->rec.layout) +
                        ": it comes from another architecture (the fingerprint of the segments' kinds and lengths); nothing was changed");
        for (int side = 0; side < 2; ++side) {
            const int phase = side ? m.dec_phase : m.enc_phase, frames = side ? m.dec_frames : m.enc_frames;
            const char* name = side ? "decoder" : "encoder";
            if (phase < fc_slots::Idle || phase > fc_slots::Ended) return fail(at + "the " + name + " phase of the record is none of idle, running, ended");
            if (frames < 0 || (phase != fc_slots::Running && frames != 0))
                return fail(at + "the " + name + " frames of the record: a side that is not running holds 0 frames, a running one 0 or more");
            if (frames > 0 && !cached) return fail(at + "the record holds " + std::to_string(frames) + " frames and this session has no key / value cache");
            if (frames > Q->max_frames)
                return fail(at + "this record of " + std::to_string(frames) + " " + name + " frames would take the utterance to " + std::to_string(frames) +
                            " frames, past the session's max_frames = " + std::to_string(Q->max_frames) +
                            " (the size of its key / value cache); nothing was changed");
        }
        if (record_pitch(*Q, who, slots[i], m.enc_frames, m.dec_frames, pitch_floats)) return 1;
    }
    for (int i = 0; i < n; ++i) {
        const fc_slot_meta& m = meta[i];
        fc::SlotRef& r = Q->rec.refs[i];
        r.slot = slots[i]; r.enc_frames = m.enc_frames; r.dec_frames = m.dec_frames;
        // the halves this session's next pushes read
        r.bits = (Q->enc_pushes & 1) | ((Q->dec_pushes & 1) << 1) | (m.enc_phase == fc_slots::Running ? fc::kSlotRecEncLive : 0) |
                 (m.dec_phase == fc_slots::Running ? fc::kSlotRecDecLive : 0);
    }
    if (record_launch(*Q, who, true, n, const_cast<float*>(records), pitch_floats, stream)) {
        for (int i = 0; i < n; ++i) Q->enc_phase[slots[i]] = Q->dec_phase[slots[i]] = (char)fc_slots::Poisoned;      // as a failed push does, for the slots named
        return 2;                                       // not a refusal: the caller's own books must follow (include/funcodec_amd.h)
    }
    for (int i = 0; i < n; ++i) {                       // whatever the slot held is abandoned, as START does
        const int b = slots[i];
        Q->enc_phase[b] = (char)meta[i].enc_phase; Q->dec_phase[b] = (char)meta[i].dec_phase;
        if (cached) { Q->enc_frames[b] = meta[i].enc_frames; Q->dec_frames[b] = meta[i].dec_frames; }
    }
    return 0;
}

int fc_slots_create(fc_engine* e, int S, int max_chunk_samples, int n_q, void* state, size_t state_bytes, fc_slots** out) {
    return slots_create(e, S, max_chunk_samples, n_q, 0, state, state_bytes, "slot state: a 16-byte aligned device buffer of fc_slots_state_bytes() bytes", out);
}

int fc_seqslots_create(fc_engine* e, int S, int max_chunk_samples, int n_q, int max_frames, void* state, size_t state_bytes, fc_slots** out) {
    if (max_frames <= 0) return fail("max_frames must be positive: the most frames a slot's utterance may hold per side");
    return slots_create(e, S, max_chunk_samples, n_q, max_frames, state, state_bytes,
                        "slot state: a 16-byte aligned device buffer of fc_seqslots_state_bytes() bytes", out);
}

void fc_slots_destroy(fc_slots* s) { delete s; }

int fc_slots_min_first(const fc_slots* s, int decode) { return s ? (decode ? s->dec_min_first : s->enc_min_first) : 0; }

int fc_graphslots_set(fc_slots* Q, int on) { return Q ? session_set_graph(Q, on) : fail("null slot session"); }
int fc_graphslots_enabled(const fc_slots* Q) { return Q && Q->graph_on ? 1 : 0; }
int fc_graphslots_counts(const fc_slots* Q, int64_t counts[4]) { return session_graph_counts(Q, counts); }

size_t fc_slots_workspace_bytes(const fc_slots* cq) {
    fc_slots* Q = const_cast<fc_slots*>(cq);
    if (!Q) return 0;
    const int Tf = ceil_div_i(Q->max_chunk, total_hop(Q->e));
    float mark;                                    // optional outputs: the pointer only marks presence in a dry pass
    // the largest encode push (no enc_out: its rows are then a buffer of the pass)
    Ctx ce = dry_ctx(Q->e, Q->B);
    slots_encode_pass(Q, ce, nullptr, Q->max_chunk, nullptr, nullptr, nullptr, nullptr, &mark, nullptr);
    // the largest decode push: decode_codes, with the first buffer as wide as decode_emb's
    Ctx cd = dry_ctx(Q->e, Q->B);
    const Pass p = slots_pass(Q, cd, true, nullptr, nullptr);
    const fc::RagLen rows;
    slots_decode_pass(Q, cd, p, decoder_input_codes(Q->e, cd, nullptr, Tf, Q->n_q, nullptr, &rows, true), Tf, 1, nullptr);
    return std::max(ce.off, cd.off) + 4096;
}

int fc_slots_encode(fc_slots* Q, const float* wav, int Tc, const int32_t* samples, const int32_t* flags, const float* scale, int64_t* codes,
                    float* quantized, float* enc_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (slots_ready(Q)) return 1;
    if (!wav || !samples || !flags || !codes) return fail("bad argument");
    if (slots_check(Q, false, samples, flags, Tc, Q->max_chunk)) return 1;
    if (counts_check_encode(Q->e, "fc_slots_encode", Q->B, Q->n_q, true)) return 1;
    const Session::GraphKey key = graph_key(*Q, kFormEncode, Tc, Q->enc_pushes, 0, {wav, codes, quantized, enc_out, scale}, workspace, workspace_bytes, stream);
    const int err = session_push(
        Q, &key, workspace, workspace_bytes, stream, [&](hipStream_t st) { return slots_upload(Q, false, samples, flags, workspace, workspace_bytes, st); },
        [&](Ctx& cx, bool captured) { return slots_encode_pass(Q, cx, wav, Tc, samples, flags, scale, codes, quantized, enc_out, captured); });
    slots_commit(Q, false, samples, flags, !err);
    return err ? 1 : 0;
}

int fc_slots_decode_emb(fc_slots* Q, const float* emb, int Tfc, const int32_t* frames, const int32_t* flags, int use_scale, float* wav,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (slots_ready(Q)) return 1;
    if (!emb || !frames || !flags || !wav) return fail("bad argument");
    if (slots_check(Q, true, frames, flags, Tfc, ceil_div_i(Q->max_chunk, total_hop(Q->e)))) return 1;
    const Session::GraphKey key = graph_key(*Q, kFormDecodeEmb, Tfc, Q->dec_pushes, use_scale, {emb, wav}, workspace, workspace_bytes, stream);
    const int err = session_push(
        Q, &key, workspace, workspace_bytes, stream, [&](hipStream_t st) { return slots_upload(Q, true, frames, flags, workspace, workspace_bytes, st); },
        [&](Ctx& cx, bool captured) {
            const Pass p = slots_pass(Q, cx, true, frames, flags, !captured);
            return slots_decode_pass(Q, cx, p, decoder_input_emb(Q->e, cx, emb, Tfc), Tfc, use_scale, wav);
        });
    slots_commit(Q, true, frames, flags, !err);
    return err ? 1 : 0;
}

int fc_slots_decode_codes(fc_slots* Q, const int64_t* codes, int Tfc, const int32_t* frames, const int32_t* flags, int use_scale, float* wav,
                          float* emb_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (slots_ready(Q)) return 1;
    if (!codes || !frames || !flags || !wav) return fail("bad argument");
    if (slots_check(Q, true, frames, flags, Tfc, ceil_div_i(Q->max_chunk, total_hop(Q->e)))) return 1;
    if (counts_check_decode(Q->e, "fc_slots_decode_codes", Q->B, Tfc, Q->n_q, true)) return 1;
    const Session::GraphKey key = graph_key(*Q, kFormDecodeCodes, Tfc, Q->dec_pushes, use_scale, {codes, wav, emb_out}, workspace, workspace_bytes, stream);
    const int err = session_push(
        Q, &key, workspace, workspace_bytes, stream, [&](hipStream_t st) { return slots_upload(Q, true, frames, flags, workspace, workspace_bytes, st); },
        [&](Ctx& cx, bool captured) {
            const Pass p = slots_pass(Q, cx, true, frames, flags, !captured);
            fc::RagLen rows; rows.lens = p.lengths;
            return slots_decode_pass(Q, cx, p, decoder_input_codes(Q->e, cx, codes, Tfc, Q->n_q, emb_out, &rows, false, Q->e->push_nq.table), Tfc, use_scale, wav);
        });
    slots_commit(Q, true, frames, flags, !err);
    return err ? 1 : 0;
}

// Test hook: the SLSTM stage of a slot push alone: the rows with start[b] != 0 begin from zeros, row b takes steps[b] <= T steps.
// steps, start host [S].  It does not look at the slots' phases and does not change them.
int fc_slots_lstm_forward(fc_slots* Q, int decoder, const float* x, int T, const int32_t* steps, const int32_t* start, float* y, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (slots_ready(Q)) return 1;
    const int S = Q->B;
    const LstmBlock* lb = lstm_hook_block(*Q, decoder, x && y && steps && start && T > 0);
    if (!lb) return 1;
    std::vector<int32_t> fl(S);
    for (int b = 0; b < S; ++b) {
        if (steps[b] < 0 || steps[b] > T) return fail("fc_slots_lstm_forward: slot " + std::to_string(b) + ": steps lie in [0, T]");
        fl[b] = start[b] ? FC_SLOT_START : 0;
    }
    Ctx cx = make_ctx(Q->e, S, workspace, workspace_bytes, stream);
    const Pass p = slots_pass(Q, cx, decoder != 0, steps, fl.data());
    cx.launch("slots start", "", [&] {      // the LSTM state alone: the slots' scales stay
        return fc::launch_slots_start(p.flags, S, lstm_state(*Q, decoder != 0), (int)lb->layers.size(), lb->H, nullptr, nullptr, cx.st);
    });
    fc::RagLen st; st.lens = p.lengths;
    if (lstm_hook_run(*Q, cx, *lb, decoder, x, T, &st, y)) slots_commit(Q, decoder != 0, steps, fl.data(), false);
    return cx.err;
}

// Test hook: the transformer stage of a slot push alone (TransformerEncoder.forward without the res_seq skip) on the session's key / value
// cache of one side: the rows with start[b] != 0 begin at position 0, row b takes frames[b] <= T frames (zeros behind).  frames, start
// host [S].  It advances the side's per-slot frame counts as a push does, refuses a row past max_frames before anything is enqueued, and
// does not look at the slots' phases.  x, y dev f32 [S][C][T].
int fc_seqslots_forward(fc_slots* Q, int decoder, const float* x, int T, const int32_t* frames, const int32_t* start, float* y, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (slots_ready(Q)) return 1;
    const int S = Q->B;
    if (!x || !y || !frames || !start || T <= 0) return fail("bad argument");
    const TfBlock& tb = decoder ? Q->e->dec_tf : Q->e->enc_tf;
    if (!tb.C || Q->max_frames <= 0) return fail("this session has no transformer bottleneck (fc_seqslots_create opens one)");
    const std::vector<int32_t>& have = decoder ? Q->dec_frames : Q->enc_frames;
    std::vector<int32_t> fl(S);
    for (int b = 0; b < S; ++b) {
        if (frames[b] < 0 || frames[b] > T) return fail("fc_seqslots_forward: slot " + std::to_string(b) + ": frames lie in [0, T]");
        fl[b] = start[b] ? FC_SLOT_START : 0;
        const int to = (start[b] ? 0 : have[b]) + frames[b];
        if (frames[b] > 0 && to > Q->max_frames)
            return fail("fc_seqslots_forward: slot " + std::to_string(b) + ": these " + std::to_string(frames[b]) + " frames would take the utterance to " +
                        std::to_string(to) + " frames, past the session's max_frames = " + std::to_string(Q->max_frames) + "; nothing was changed");
    }
    Ctx cx = make_ctx(Q->e, S, workspace, workspace_bytes, stream);
    const Pass p = slots_pass(Q, cx, decoder != 0, frames, fl.data());
    TfCache kv = tf_cache(*Q, decoder != 0, 0);
    kv.rows = true; kv.len.lens = p.lengths; kv.pos_dev = p.pos; kv.host_len = p.host_push; kv.host_pos = p.host_push + 2 * S;
    Act in; in.raw = const_cast<float*>(x); in.C = tb.C; in.T = T;
    Act out = run_transformer(Q->e, cx, tb, in, T, &kv);
    cx.launch("copy", "y", [&] { return hipMemcpyAsync(y, out.raw, (size_t)S * tb.C * T * sizeof(float), hipMemcpyDeviceToDevice, cx.st); });
    cx.launch("ragged mask", "y", [&] { return fc::launch_ragged_mask_f32(y, 1, S, tb.C, T, 1, kv.len, cx.st); });      // as a push masks its outputs
    if (cx.err) slots_commit(Q, decoder != 0, frames, fl.data(), false);
    else slots_advance(Q, decoder != 0, frames, fl.data(), 1);
    return cx.err;
}

}  // extern "C"
