// LauraTTS generation engine: plan, checkpoint ingestion / weight re-layout, workspace planning and the fc_laura_* part of the
// C ABI (include/funcodec_amd.h).  Every Linear exists in up to two device layouts: the packed image of the codec's implicit-GEMM
// conv kernel (full-sequence form) and MFMA-fragment order (decoding step, LM only).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/funcodec_amd.h"
#include "kernels.h"
#include "laura_kernels.h"

// fc_last_error()'s thread-local message lives in engine.hip
extern "C" void fc_set_last_error_(const char* msg);

namespace {

namespace lk = fc::laura;

int fail(const std::string& msg) { fc_set_last_error_(msg.c_str()); return 1; }
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

int ceil_div_i(int a, int b) { return (a + b - 1) / b; }
int pad4(int n) { return (n + 3) & ~3; }

struct HostTensor {
    std::vector<int64_t> dims;
    std::vector<float> data;
    bool set = false;
};

// One Linear of the checkpoint.
struct Lin {
    std::string name;       // state_dict prefix ("...linear_qkv" = rows of linear_q, linear_k, linear_v stacked)
    int cin = 0, cout = 0;
    // full-sequence form: k = 1 layer of conv_mfma_kernel
    int BM = 128, BN = 128, CC = 2, nchunk = 1, Mpad = 0;
    bool row = false;
    float *wt = nullptr, *bias = nullptr;
    int* koff = nullptr;
    // step form
    float* wf = nullptr;    // fragment order, null if the layer never runs in a decoding step
};

struct Block {
    Lin qkv, out, ff1, ff2;
    float *n1g = nullptr, *n1b = nullptr, *n2g = nullptr, *n2b = nullptr;   // attention norm, FFN norm
    float *bu = nullptr, *bv = nullptr;                                       // pos_bias_u / v flattened [d]
    float* ptab = nullptr;                                                    // [d][PR]
};

struct Stack {
    std::string prefix;
    fc_laura_stack s;
    Lin embed;
    float *eg = nullptr, *eb = nullptr, *ag = nullptr, *ab = nullptr;         // input-layer LayerNorm, after_norm
    std::vector<Block> blocks;
    bool step = false;
};

struct Ctx {
    int B = 0;
    hipStream_t st = nullptr;
    char* base = nullptr;
    size_t cap = 0, off = 0;
    bool dry = false;
    int err = 0;
    template <typename T>
    T* alloc(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = dry ? nullptr : (T*)(base + off);
        off += n * sizeof(T);
        if (!dry && off > cap) { err = 1; fail("workspace too small"); return nullptr; }
        return p;
    }
    bool live() const { return !dry && !err; }
    void check(hipError_t e, const char* what) {
        if (e != hipSuccess && !err) { err = 1; fail(std::string(what) + ": " + hipGetErrorString(e)); }
    }
};

}  // namespace

struct fc_laura {
    fc_laura_arch arch;
    int device = 0;
    bool finalized = false;
    int R = 0, PR = 0;      // relative positions -(R-1) .. R-1; row stride of the position tables
    std::vector<std::pair<std::string, std::vector<int64_t>>> expected;
    std::map<std::string, HostTensor> host;
    Stack text_encoder, codec_lm, codec_encoder;
    Lin text_out, lm_decoder, codec_out;
    float *lm_emb = nullptr, *cb = nullptr, *tok_emb = nullptr, *pe_abs = nullptr;
    float* lm_embed_wt = nullptr;      // codec_lm.encoder.embed.0.weight transposed [D][d] (the sampler's fused input layer)
    lk::StepLayer* step_layers = nullptr;   // device table of the LM's blocks for the persistent decoding step (laura_persist.hip)
    int persist_grid = 0;              // workgroups of the persistent step launch, 0 = not available on this device / for this model
    bool persist_on = !(getenv("FC_LAURA_PERSIST") && atoi(getenv("FC_LAURA_PERSIST")) == 0);   // fc_laura_set_persistent_step
    int persist_fallbacks = 0;         // calls that timed out at a hand-off of the persistent step and were re-run on the kernel chain
    std::map<std::string, Lin*> lin_by_name;
    std::vector<void*> dev_allocs;
    int vocab() const { return arch.predict_nq * (arch.codebook_size + 1); }
};

namespace {

template <typename T>
int upload(fc_laura* e, const std::vector<T>& h, T** out) {
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, h.size() * sizeof(T) + 16));
    HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    e->dev_allocs.push_back(d);
    *out = (T*)d;
    return 0;
}

// ---- plan ------------------------------------------------------------------------------------------------------------------
void expect(fc_laura* e, const std::string& name, std::vector<int64_t> dims) { e->expected.push_back({name, std::move(dims)}); }

void lin_tiling(Lin& L) {
    // the same choices engine.hip::choose_tiling makes for a k = 1, stride 1 layer whose input is already materialised
    if (L.cout > 64) { L.BM = 128; L.BN = 128; }
    else if (L.cout > 32) { L.BM = 64; L.BN = 256; }
    else { L.BM = 32; L.BN = 256; }
    const size_t lds_budget = (size_t)(160 / fc::conv_wgs_per_cu(L.BM)) * 1024;
    int cin_p2 = 2;
    while (cin_p2 < L.cin) cin_p2 *= 2;
    int cc = 2;
    for (;;) {
        const int n = cc * 2;
        if (n > 32 || n > cin_p2) break;
        if (!fc::conv_slab_fits(1, 1, 1, n, L.BN, L.BM, false)) break;
        if (fc::conv_lds_bytes_for(1, 1, 1, n, L.BM, L.BN, L.cin, 0, 0) > lds_budget) break;
        cc = n;
    }
    L.row = false;
    int best = 0;
    for (int n = 4; n <= 64 && n <= L.cin; n *= 2) {
        if (!fc::conv_row_ok(1, 1, 1, n, L.BM, L.BN, L.cin, false)) continue;
        if (fc::conv_lds_bytes_for(1, 1, 1, n, L.BM, L.BN, L.cin, 0, 1) > lds_budget) continue;
        best = n;
    }
    if (best > cc) { L.row = true; cc = best; }
    L.CC = cc;
    L.nchunk = ceil_div_i(L.cin, cc);
    L.Mpad = ceil_div_i(L.cout, L.BM) * L.BM;
}

Lin mk_lin(fc_laura* e, const std::string& name, int cin, int cout, bool bias, bool in_ckpt = true) {
    Lin L;
    L.name = name; L.cin = cin; L.cout = cout;
    lin_tiling(L);
    if (in_ckpt) {
        expect(e, name + ".weight", {cout, cin});
        if (bias) expect(e, name + ".bias", {cout});
    }
    return L;
}

void plan_stack(fc_laura* e, Stack& S, const std::string& prefix, const fc_laura_stack& s, bool step) {
    S.prefix = prefix; S.s = s; S.step = step;
    const int d = s.d_model, dk = d / s.heads;
    S.embed = mk_lin(e, prefix + ".embed.0", s.idim, d, true);
    expect(e, prefix + ".embed.1.weight", {d});
    expect(e, prefix + ".embed.1.bias", {d});
    const char* n_att = s.norm_style ? "norm1" : "norm_mha";
    const char* n_ff = s.norm_style ? "norm2" : "norm_ff";
    S.blocks.resize(s.layers);
    for (int i = 0; i < s.layers; ++i) {
        Block& b = S.blocks[i];
        const std::string p = prefix + ".encoders." + std::to_string(i);
        expect(e, p + ".self_attn.pos_bias_u", {s.heads, dk});
        expect(e, p + ".self_attn.pos_bias_v", {s.heads, dk});
        for (const char* n : {"linear_q", "linear_k", "linear_v"}) {
            expect(e, p + ".self_attn." + n + ".weight", {d, d});
            expect(e, p + ".self_attn." + n + ".bias", {d});
        }
        b.qkv = mk_lin(e, p + ".self_attn.linear_qkv", d, 3 * d, true, false);
        b.out = mk_lin(e, p + ".self_attn.linear_out", d, d, true);
        expect(e, p + ".self_attn.linear_pos.weight", {d, d});
        b.ff1 = mk_lin(e, p + ".feed_forward.w_1", d, s.ff, true);
        b.ff2 = mk_lin(e, p + ".feed_forward.w_2", s.ff, d, true);
        for (const char* n : {n_att, n_ff}) {
            expect(e, p + "." + n + ".weight", {d});
            expect(e, p + "." + n + ".bias", {d});
        }
    }
    expect(e, prefix + ".after_norm.weight", {d});
    expect(e, prefix + ".after_norm.bias", {d});
}

void register_lins(fc_laura* e) {
    auto reg = [&](Lin& L) { e->lin_by_name[L.name] = &L; };
    for (Stack* S : {&e->text_encoder, &e->codec_lm, &e->codec_encoder}) {
        reg(S->embed);
        for (Block& b : S->blocks) { reg(b.qkv); reg(b.out); reg(b.ff1); reg(b.ff2); }
    }
    reg(e->text_out); reg(e->lm_decoder); reg(e->codec_out);
}

// ---- packing ---------------------------------------------------------------------------------------------------------------
// W [cout][cin] row-major (torch Linear) -> conv_mfma_kernel's chunk images [m_tile][chunk][tap 0][local channel][BM rows]
int pack_full(fc_laura* e, Lin& L, const std::vector<float>& W, const std::vector<float>& bias) {
    const int mtiles = L.Mpad / L.BM;
    const int wbuf = fc::conv_wbuf_floats(1, L.CC, L.BM);
    std::vector<float> packed((size_t)mtiles * L.nchunk * wbuf, 0.f);
    for (int mt = 0; mt < mtiles; ++mt)
        for (int ch = 0; ch < L.nchunk; ++ch)
            for (int cl = 0; cl < L.CC; ++cl) {
                const int ci = ch * L.CC + cl;
                if (ci >= L.cin) continue;
                float* img = &packed[(size_t)(mt * L.nchunk + ch) * wbuf];
                for (int mm = 0; mm < L.BM; ++mm) {
                    const int m = mt * L.BM + mm;
                    if (m < L.cout) img[fc::conv_pack_index(1, L.CC, L.BM, 0, cl, mm)] = W[(size_t)m * L.cin + ci];
                }
            }
    std::vector<float> bpad(L.Mpad, 0.f);
    for (int m = 0; m < L.cout && m < (int)bias.size(); ++m) bpad[m] = bias[m];
    if (upload(e, packed, &L.wt)) return 1;
    if (upload(e, bpad, &L.bias)) return 1;
    if (upload(e, fc::conv_koff_table(1, 1, 1, L.CC, L.BN, L.row ? 1 : 0), &L.koff)) return 1;
    return 0;
}

// fragment order of the decoding step's GEMV: [16-row tile][16-wide k chunk][lane = 16 g + r][j] = W[16 tile + r][16 chunk + 4 g + j]
int pack_step(fc_laura* e, Lin& L, const std::vector<float>& W) {
    if (L.cin % 16) return fail("decoding-step GEMV needs an input width that is a multiple of 16: " + L.name);
    const int tiles = ceil_div_i(L.cout, 16), nch = L.cin / 16;
    std::vector<float> f((size_t)tiles * nch * 256, 0.f);
    for (int t = 0; t < tiles; ++t)
        for (int c = 0; c < nch; ++c)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 15, g = lane >> 4, n = 16 * t + r;
                if (n >= L.cout) continue;
                for (int j = 0; j < 4; ++j)
                    f[((size_t)(t * nch + c) * 64 + lane) * 4 + j] = W[(size_t)n * L.cin + 16 * c + 4 * g + j];
            }
    return upload(e, f, &L.wf);
}

int pack_lin(fc_laura* e, Lin& L, bool step, const std::vector<float>* Wp = nullptr, const std::vector<float>* Bp = nullptr) {
    static const std::vector<float> none;
    const std::vector<float>& W = Wp ? *Wp : e->host[L.name + ".weight"].data;
    const std::vector<float>& Bv = Bp ? *Bp : (e->host.count(L.name + ".bias") ? e->host[L.name + ".bias"].data : none);
    if (pack_full(e, L, W, Bv)) return 1;
    if (step && pack_step(e, L, W)) return 1;
    return 0;
}

hipError_t launch_lin_full(const Lin& L, const float* in, int B, int T, float* out, hipStream_t st) {
    fc::ConvLaunch c;
    c.s0.ptr = in; c.s0.used = 1;
    c.wt = L.wt; c.bias = L.bias; c.koff = L.koff;
    c.out = out; c.out_sB = (long long)L.cout * T; c.out_sM = T; c.out_sT = 1;
    c.B = B; c.Cin = L.cin; c.Tin = T; c.M = L.cout; c.Tout = T;
    c.k = 1; c.stride = 1; c.padL = 0; c.padR = 0; c.dil = 1; c.pad_zero = 1;
    c.BM = L.BM; c.BN = L.BN; c.CC = L.CC; c.nchunk = L.nchunk; c.row = L.row ? 1 : 0;
    return fc::launch_conv(c, st);
}

// RelPositionalEncoding.extend_pe (funcodec/modules/embedding.py:293-306) evaluated the way torch evaluates it in fp32:
// div_term = exp(float(2m) * float(-(ln 10000 / d))), pe(r)[2m] = sin(r * div_term), pe(r)[2m+1] = cos(r * div_term); negative
// relative positions are sin / cos of the negated product.  Feature-major [d][PR], column = r + R - 1.
std::vector<float> rel_pe_fm(int d, int R, int PR) {
    std::vector<float> pe((size_t)d * PR, 0.f);
    for (int m = 0; m < d / 2; ++m) {
        const float div = expf((float)(2 * m) * (float)(-(std::log(10000.0) / (double)d)));
        for (int col = 0; col < PR; ++col) {
            const int r = col - (R - 1);
            const float a = (float)(r < 0 ? -r : r) * div;
            const float sn = sinf(a), cs = cosf(a);
            pe[(size_t)(2 * m) * PR + col] = r < 0 ? -sn : sn;
            pe[(size_t)(2 * m + 1) * PR + col] = cs;
        }
    }
    return pe;
}

int pack_stack(fc_laura* e, Stack& S, const float* pe_dev, void* ws, size_t ws_bytes) {
    (void)ws; (void)ws_bytes;
    const int d = S.s.d_model;
    auto H = [&](const std::string& k) -> const std::vector<float>& { return e->host[k].data; };
    if (pack_lin(e, S.embed, S.step)) return 1;
    if (upload(e, H(S.prefix + ".embed.1.weight"), &S.eg)) return 1;
    if (upload(e, H(S.prefix + ".embed.1.bias"), &S.eb)) return 1;
    if (upload(e, H(S.prefix + ".after_norm.weight"), &S.ag)) return 1;
    if (upload(e, H(S.prefix + ".after_norm.bias"), &S.ab)) return 1;
    const char* n_att = S.s.norm_style ? "norm1" : "norm_mha";
    const char* n_ff = S.s.norm_style ? "norm2" : "norm_ff";
    for (int i = 0; i < S.s.layers; ++i) {
        Block& b = S.blocks[i];
        const std::string p = S.prefix + ".encoders." + std::to_string(i);
        std::vector<float> W((size_t)3 * d * d), Bv((size_t)3 * d);
        int part = 0;
        for (const char* n : {"linear_q", "linear_k", "linear_v"}) {
            const auto& w = H(p + ".self_attn." + n + ".weight");
            const auto& bb = H(p + ".self_attn." + n + ".bias");
            std::copy(w.begin(), w.end(), W.begin() + (size_t)part * d * d);
            std::copy(bb.begin(), bb.end(), Bv.begin() + (size_t)part * d);
            ++part;
        }
        if (pack_lin(e, b.qkv, S.step, &W, &Bv)) return 1;
        if (pack_lin(e, b.out, S.step)) return 1;
        if (pack_lin(e, b.ff1, S.step)) return 1;
        if (pack_lin(e, b.ff2, S.step)) return 1;
        if (upload(e, H(p + "." + n_att + ".weight"), &b.n1g)) return 1;
        if (upload(e, H(p + "." + n_att + ".bias"), &b.n1b)) return 1;
        if (upload(e, H(p + "." + n_ff + ".weight"), &b.n2g)) return 1;
        if (upload(e, H(p + "." + n_ff + ".bias"), &b.n2b)) return 1;
        if (upload(e, H(p + ".self_attn.pos_bias_u"), &b.bu)) return 1;
        if (upload(e, H(p + ".self_attn.pos_bias_v"), &b.bv)) return 1;
        // position table of the block: linear_pos (no bias) applied to every relative-position encoding, on the device
        Lin pos;
        pos.name = p + ".self_attn.linear_pos"; pos.cin = d; pos.cout = d;
        lin_tiling(pos);
        if (pack_lin(e, pos, false)) return 1;
        void* tab = nullptr;
        HIP_TRY(hipMalloc(&tab, (size_t)d * e->PR * sizeof(float)));
        e->dev_allocs.push_back(tab);
        b.ptab = (float*)tab;
        HIP_TRY(launch_lin_full(pos, pe_dev, 1, e->PR, b.ptab, nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// ---- execution ---------------------------------------------------------------------------------------------------------------
struct KvOut {            // LM prefix pass: K / V rows of every block go to the decoding step's caches
    float* kc = nullptr;  // [layers][rows][d][Tcap]
    float* vc = nullptr;  // [layers][rows][Tcap][d]
    int Tcap = 0;
    size_t layer_stride = 0;   // floats from one block's cache to the next: rows * d * Tcap
    size_t row_base = 0;       // where the pass's row 0 lies inside a block's cache (a decoding session's slot: slot * d * Tcap)
    const lk::RowSlots* slots = nullptr;   // a session slot per batch row instead (fc_laura_slots_start_many), S slots in the session
    int S = 0;
};

// debugging aid (fc_laura_debug_probe): copy one intermediate tensor of the next full-sequence stack run to a caller buffer
struct Probe { float* dst = nullptr; size_t cap = 0; int layer = -1, what = -1, stack = -1; };
thread_local Probe g_probe;
void probe(Ctx& cx, const Stack& S, int what, int layer, const float* src, size_t n) {
    if (!g_probe.dst || !cx.live() || g_probe.what != what || g_probe.layer != layer) return;
    if (g_probe.stack >= 0 && g_probe.stack != (S.prefix == "text_encoder" ? 0 : S.prefix == "codec_lm.encoder" ? 1 : 2)) return;
    if (n * sizeof(float) > g_probe.cap) n = g_probe.cap / sizeof(float);
    cx.check(hipMemcpyAsync(g_probe.dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, cx.st), "probe");
}

// The attention of block b of stack S over one QKV buffer [B][3 d][T]: what run_stack_full launches, and fc_laura_attention (the per-op
// test entry) with it.
lk::AttnFull attn_full_args(const fc_laura* e, const Stack& S, const Block& b, const float* qkv, const int* lens, const int* bidir,
                            int causal, float* ctx, int B, int T) {
    lk::AttnFull a;
    a.qkv = qkv; a.ptab = b.ptab; a.bias_u = b.bu; a.bias_v = b.bv; a.lens = lens; a.bidir = bidir; a.causal = causal; a.ctx = ctx;
    a.B = B; a.H = S.s.heads; a.DK = S.s.d_model / S.s.heads; a.T = T; a.R = e->R; a.PR = e->PR;
    return a;
}

// The stack on feature-major input [B][idim][T]; returns after_norm(x) [B][d][T].
float* run_stack_full(fc_laura* e, Ctx& cx, const Stack& S, const float* in, int T, const int* lens, const int* bidir, int causal,
                      const KvOut* kv) {
    const int B = cx.B, d = S.s.d_model, ff = S.s.ff;
    float* x = cx.alloc<float>((size_t)B * d * T);
    float* xn = cx.alloc<float>((size_t)B * d * T);
    float* dl = cx.alloc<float>((size_t)B * d * T);
    float* qkv = cx.alloc<float>((size_t)B * 3 * d * T);
    float* ctx = cx.alloc<float>((size_t)B * d * T);
    float* hb = cx.alloc<float>((size_t)B * ff * T);
    if (!cx.live()) return xn;
    cx.check(launch_lin_full(S.embed, in, B, T, dl, cx.st), "embed GEMM");
    // Linear -> LayerNorm(eps 1e-5) -> [ReLU] -> x * sqrt(d)   (conformer_encoder.py:372-378, transformer_encoder.py:463-470)
    cx.check(lk::launch_layernorm_fm(dl, nullptr, nullptr, S.eg, S.eb, 1e-5f, S.s.embed_relu, sqrtf((float)d), x, B, d, T, cx.st), "embed LayerNorm");
    probe(cx, S, 0, 0, x, (size_t)B * d * T);
    const float* pending = nullptr;
    for (int i = 0; i < S.s.layers && !cx.err; ++i) {
        const Block& b = S.blocks[i];
        cx.check(lk::launch_layernorm_fm(x, pending, pending ? x : nullptr, b.n1g, b.n1b, 1e-12f, 0, 1.f, xn, B, d, T, cx.st), "LayerNorm");
        probe(cx, S, 5, i, x, (size_t)B * d * T);
        probe(cx, S, 1, i, xn, (size_t)B * d * T);
        cx.check(launch_lin_full(b.qkv, xn, B, T, qkv, cx.st), "QKV GEMM");
        probe(cx, S, 2, i, qkv, (size_t)B * 3 * d * T);
        if (kv && kv->slots)
            cx.check(lk::launch_kv_store_slots(qkv, lens, *kv->slots, kv->S, d, T, kv->Tcap, kv->kc + (size_t)i * kv->layer_stride,
                                               kv->vc + (size_t)i * kv->layer_stride, cx.st), "kv store");
        else if (kv) cx.check(lk::launch_kv_store(qkv, lens, B, d, T, kv->Tcap, kv->kc + (size_t)i * kv->layer_stride + kv->row_base,
                                             kv->vc + (size_t)i * kv->layer_stride + kv->row_base, cx.st), "kv store");
        cx.check(lk::launch_attn_full(attn_full_args(e, S, b, qkv, lens, bidir, causal, ctx, B, T), cx.st), "attention");
        probe(cx, S, 3, i, ctx, (size_t)B * d * T);
        cx.check(launch_lin_full(b.out, ctx, B, T, dl, cx.st), "out GEMM");
        cx.check(lk::launch_layernorm_fm(x, dl, x, b.n2g, b.n2b, 1e-12f, 0, 1.f, xn, B, d, T, cx.st), "LayerNorm");
        cx.check(launch_lin_full(b.ff1, xn, B, T, hb, cx.st), "FFN GEMM 1");
        cx.check(lk::launch_act(hb, (size_t)B * ff * T, S.s.act, cx.st), "activation");
        cx.check(launch_lin_full(b.ff2, hb, B, T, dl, cx.st), "FFN GEMM 2");
        pending = dl;
    }
    cx.check(lk::launch_layernorm_fm(x, pending, pending ? x : nullptr, S.ag, S.ab, 1e-12f, 0, 1.f, xn, B, d, T, cx.st), "after_norm");
    probe(cx, S, 5, S.s.layers, x, (size_t)B * d * T);
    return xn;
}

struct LenPack { int v[64]; };
__global__ void set_lens_kernel(LenPack p, int* dst, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = p.v[threadIdx.x];
}

// Lengths travel BY VALUE in kernel arguments (64 per launch): the caller's arrays are temporaries of the binding, and an asynchronous
// copy from pageable host memory is allowed to read them after the call has returned.
int* upload_lens(Ctx& cx, const int32_t* host, int B, int fill = 0) {
    int* d = cx.alloc<int>(B);
    if (!cx.live()) return d;
    if (host) {
        for (int b0 = 0; b0 < B; b0 += 64) {
            LenPack p;
            const int n = B - b0 < 64 ? B - b0 : 64;
            for (int i = 0; i < 64; ++i) p.v[i] = i < n ? host[b0 + i] : 0;
            hipLaunchKernelGGL(set_lens_kernel, dim3(1), dim3(64), 0, cx.st, p, d + b0, n);
        }
        cx.check(hipGetLastError(), "lengths upload");
    } else cx.check(lk::launch_fill_i32(d, fill, B, cx.st), "fill");
    return d;
}

int check_lens(const int32_t* lens, int B, int lo, int hi, const char* what) {
    for (int b = 0; b < B; ++b)
        if (lens[b] < lo || lens[b] > hi) return fail(std::string(what) + " out of range");
    return 0;
}

Ctx make_ctx(int B, void* ws, size_t ws_bytes, void* stream) {
    Ctx cx;
    cx.B = B; cx.st = (hipStream_t)stream; cx.base = (char*)ws; cx.cap = ws_bytes;
    cx.dry = ws == nullptr;
    return cx;
}

int max_of(const int32_t* v, int n) {
    int m = 0;
    for (int i = 0; i < n; ++i) m = std::max(m, (int)v[i]);
    return m;
}

// text side: token-major text_outs [B][L][D] -> feature-major [B][D][Tt]
float* text_to_fm(fc_laura* e, Ctx& cx, const float* text_outs, const int* tl_dev, int L, int* Tt_out) {
    const int D = e->arch.codebook_dim, Tt = pad4(L);
    float* fm = cx.alloc<float>((size_t)cx.B * D * Tt);
    if (cx.live()) cx.check(lk::launch_tm_to_fm(text_outs, tl_dev, cx.B, L, D, Tt, fm, cx.st), "text transpose");
    *Tt_out = Tt;
    return fm;
}

int do_encode(fc_laura* e, Ctx& cx, const float* text_emb, const int64_t* text_ids, const int32_t* text_lens, int L, float* text_outs) {
    const int B = cx.B, idim = e->arch.input_size, D = e->arch.codebook_dim, T = pad4(L);
    int* tl = upload_lens(cx, text_lens, B);
    float* in = cx.alloc<float>((size_t)B * idim * T);
    if (cx.live()) {
        if (text_ids) cx.check(lk::launch_token_embed_fm(text_ids, e->tok_emb, e->arch.vocab_size, B, L, idim, T, in, cx.st), "token embedding");
        else cx.check(lk::launch_tm_to_fm(text_emb, tl, B, L, idim, T, in, cx.st), "text transpose");
    }
    float* h = run_stack_full(e, cx, e->text_encoder, in, T, tl, nullptr, 0, nullptr);
    float* o = cx.alloc<float>((size_t)B * D * T);
    if (cx.live()) {
        cx.check(launch_lin_full(e->text_out, h, B, T, o, cx.st), "text_enc_out_layer");
        cx.check(lk::launch_fm_to_tm(o, tl, B, D, T, L, text_outs, cx.st), "output transpose");
    }
    return cx.err;
}

int do_lm_logprobs(fc_laura* e, Ctx& cx, const float* text_outs, const int32_t* text_lens, int L, const int64_t* codec,
                   const int32_t* codec_lens, int Cmax, float* logp, int Tseq) {
    const int B = cx.B, D = e->arch.codebook_dim, V = e->vocab();
    const int T = pad4(Tseq);
    int* tl = upload_lens(cx, text_lens, B);
    int* cl = upload_lens(cx, codec ? codec_lens : nullptr, B, 0);
    int Tt = 0;
    float* tfm = text_to_fm(e, cx, text_outs, tl, L, &Tt);
    float* seq = cx.alloc<float>((size_t)B * D * T);
    int* seq_len = cx.alloc<int>(B);
    int* bidir = cx.alloc<int>(B);
    if (cx.live())
        cx.check(lk::launch_lm_assemble(tfm, Tt, tl, e->lm_emb, e->cb, e->arch.codebook_size, e->arch.predict_nq, codec, cl, Cmax, B, D, T,
                                        seq, seq_len, bidir, cx.st), "LM input");
    float* h = run_stack_full(e, cx, e->codec_lm, seq, T, seq_len, e->arch.bidirectional_inputs ? bidir : nullptr, 1, nullptr);
    float* lg = cx.alloc<float>((size_t)B * V * T);
    if (cx.live()) {
        cx.check(launch_lin_full(e->lm_decoder, h, B, T, lg, cx.st), "LM decoder GEMM");
        cx.check(lk::launch_logsoftmax_fm(lg, seq_len, B, V, T, Tseq, logp, cx.st), "log-softmax");
    }
    return cx.err;
}

int do_codec_emb(fc_laura* e, Ctx& cx, const float* text_outs, const int32_t* text_lens, int L, const int64_t* codec, int nq_cols,
                 const int32_t* codec_lens, int Cmax, float* emb, int Tmax) {
    const int B = cx.B, D = e->arch.codebook_dim, T = pad4(Tmax);
    int* tl = upload_lens(cx, text_lens, B);
    int* cl = upload_lens(cx, codec_lens, B);
    int Tt = 0;
    float* tfm = text_to_fm(e, cx, text_outs, tl, L, &Tt);
    float* in = cx.alloc<float>((size_t)B * D * T);
    int* seq_len = cx.alloc<int>(B);
    if (cx.live())
        cx.check(lk::launch_nar_assemble(tfm, Tt, tl, e->cb, e->arch.codebook_size, e->arch.predict_nq, codec, cl, Cmax, nq_cols, e->pe_abs,
                                         e->arch.pos_emb_split, B, D, T, in, seq_len, cx.st), "predictor input");
    float* h = run_stack_full(e, cx, e->codec_encoder, in, T, seq_len, nullptr, 0, nullptr);
    float* o = cx.alloc<float>((size_t)B * D * T);
    if (cx.live()) {
        cx.check(launch_lin_full(e->codec_out, h, B, T, o, cx.st), "codec_encoder_out_layer");
        cx.check(lk::launch_nar_extract(o, tl, cl, B, D, T, Cmax, emb, cx.st), "predictor output");
    }
    return cx.err;
}

hipError_t step_gemv(const Lin& L, const float* x, int B, const float* gamma, const float* beta, float eps, int act, int mode, float* y,
                     int ldy, hipStream_t st, float* kc = nullptr, float* vc = nullptr, const int* pos = nullptr, int d = 0, int Tcap = 0,
                     const float* apart = nullptr, int H = 0, int DK = 0, int NS = 0, int stage = 0, int wide = 0) {
    lk::Gemv g;
    g.stage = stage; g.wide = wide;
    g.apart = apart; g.H = H; g.DK = DK; g.NS = NS;
    g.x = x; g.wf = L.wf; g.bias = L.bias; g.gamma = gamma; g.beta = beta; g.eps = eps; g.act = act; g.mode = mode; g.y = y; g.ldy = ldy;
    g.kc = kc; g.vc = vc; g.pos = pos; g.d = d; g.Tcap = Tcap; g.B = B; g.K = L.cin; g.N = L.cout;
    return lk::launch_gemv(g, st);
}

__global__ void copy_prompt_kernel(const int64_t* src, const int* lens, int Cmax, int nq, int64_t* dst, int stride) {
    const int b = blockIdx.x;
    const int n = lens[b] * nq;
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[(size_t)b * stride * nq + i] = src[(size_t)b * Cmax * nq + i];
}

// Everything a decoding step of B rows keeps between two samples: the caches, the positions and counters, the token vectors of the kernel
// chain, the persistent step's edge buffers and arrival counters.  A decode_codec call lays it out in its workspace, a decoding session
// in its state.
struct StepMem {
    int B = 0, Tcap = 0, NS = 1, KS2 = 1;
    int* pos = nullptr;                 // [B] = sequence length after the prefix pass: the cache fill
    int* ctr = nullptr;                 // n_gen[B], done[B], step[B], n_done
    float *kc = nullptr, *vc = nullptr; // [layers][B][d][Tcap], [layers][B][Tcap][d]
    float *xs = nullptr, *qb = nullptr, *apart = nullptr, *hb = nullptr, *lg = nullptr, *nemb = nullptr, *edge = nullptr;
    unsigned *psync = nullptr, *pseq = nullptr;
    size_t edge_stride = 0, sync_words = 0, o_q = 0, o_ap = 0, o_xm = 0, o_hb = 0, o_xo = 0;
    int* n_gen() const { return ctr; }
    int* done() const { return ctr + B; }
    int* step() const { return ctr + 2 * B; }
    int* n_done() const { return ctr + 3 * B; }
    unsigned* error_word() const { return psync + sync_words - 64; }
};

// rows of the step's token vectors: the GEMV's column blocks are whole
int step_rows(int B) { return 16 * ((B + 15) / 16); }

StepMem alloc_step_mem(fc_laura* e, Ctx& cx, int B, int Tcap) {
    const Stack& S = e->codec_lm;
    const int D = e->arch.codebook_dim, V = e->vocab(), d = S.s.d_model, ff = S.s.ff, NL = S.s.layers;
    const int heads = S.s.heads, dkh = d / S.s.heads;
    StepMem m;
    m.B = B; m.Tcap = Tcap;
    m.pos = cx.alloc<int>(B);
    m.ctr = cx.alloc<int>(3 * B + 4);
    m.kc = cx.alloc<float>((size_t)NL * B * d * Tcap);
    m.vc = cx.alloc<float>((size_t)NL * B * d * Tcap);
    const size_t RW = (size_t)step_rows(B);     // whole column blocks of the GEMV: 16 up to 16 rows
    m.xs = cx.alloc<float>(RW * d);
    m.qb = cx.alloc<float>(RW * d);
    m.NS = 256 / (B * heads);                   // key ranges per (utterance, head): fill the chip's 256 CUs
    m.NS = m.NS < 1 ? 1 : (m.NS > 8 ? 8 : m.NS);
    m.apart = cx.alloc<float>(RW * heads * 8 * (dkh + 2));
    m.hb = cx.alloc<float>(RW * ff);
    m.lg = cx.alloc<float>(RW * V);
    m.nemb = cx.alloc<float>(RW * D);
    // the decoding step as ONE persistent launch (laura_persist.hip, B <= 16 only): per-block edge buffers, arrival counters, the launch counter
    m.KS2 = lk::step_persist_ksplit(d, ff);
    auto pad32 = [](size_t n) { return (n + 31) & ~(size_t)31; };
    m.o_q = 0; m.o_ap = m.o_q + pad32((size_t)16 * d); m.o_xm = m.o_ap + pad32((size_t)16 * heads * 8 * (dkh + 4));
    m.o_hb = m.o_xm + pad32((size_t)16 * d); m.o_xo = m.o_hb + pad32((size_t)16 * ff);
    m.edge_stride = m.o_xo + pad32((size_t)m.KS2 * 16 * d);
    m.edge = cx.alloc<float>(m.edge_stride * NL);
    m.sync_words = lk::step_persist_sync_words(NL);
    m.psync = cx.alloc<unsigned>(m.sync_words + 32);
    m.pseq = m.psync ? m.psync + m.sync_words : nullptr;            // one word behind the counters
    return m;
}

bool step_persist_ok(const fc_laura* e, const StepMem& m) {
    const fc_laura_stack& s = e->codec_lm.s;
    return e->persist_on && e->persist_grid > 0 &&
           lk::step_persist_supported(m.B, s.d_model, s.ff, s.heads, s.d_model / s.heads, e->vocab(), m.NS);
}

// the model's side of a sample: the group layout, the codebook table, the LM's fused input layer.  The one statement of these fields, for
// a step over the engine's own rows (step_sampler) and for fc_laura_sample (the per-op test entry) over the caller's
lk::Sample model_sampler(const fc_laura* e) {
    const Stack& S = e->codec_lm;
    lk::Sample sm;
    sm.K = e->arch.codebook_size; sm.nq = e->arch.predict_nq;
    sm.cb = e->cb; sm.D = e->arch.codebook_dim;
    // the sampler also runs the LM's input layer on the new token (Linear + LayerNorm + ReLU + x * sqrt(d)): xs is ready for block 0
    sm.emb_wt = e->lm_embed_wt; sm.emb_bias = S.embed.bias; sm.emb_g = S.eg; sm.emb_b = S.eb; sm.dm = S.s.d_model; sm.emb_relu = S.s.embed_relu;
    sm.xscale = sqrtf((float)S.s.d_model);
    return sm;
}

// the sampler of a step over m's rows; the caller adds what is its own (the call's or the rows' parameters, the token buffers)
lk::Sample step_sampler(const fc_laura* e, const StepMem& m) {
    lk::Sample sm = model_sampler(e);
    sm.logits = m.lg; sm.B = m.B;
    sm.n_gen = m.n_gen(); sm.done = m.done(); sm.n_done = m.n_done(); sm.pos = m.pos; sm.step = m.step();
    sm.next_emb = m.nemb; sm.xs = m.xs;
    sm.launch_seq = m.pseq;                // every sampler launch numbers the persistent step launch that follows it (1, 2, ...)
    return sm;
}

lk::StepPersistArgs step_persist_args(const fc_laura* e, const StepMem& m, unsigned long long* ptrace) {
    const Stack& S = e->codec_lm;
    lk::StepPersistArgs pa{};
    pa.layers = e->step_layers; pa.wdec = e->lm_decoder.wf; pa.bdec = e->lm_decoder.bias; pa.ag = S.ag; pa.ab = S.ab;
    pa.xs = m.xs; pa.logits = m.lg; pa.edge = m.edge; pa.kc = m.kc; pa.vc = m.vc; pa.pos = m.pos; pa.sync = m.psync; pa.seq = m.pseq;
    pa.edge_stride = m.edge_stride; pa.o_q = (int)m.o_q; pa.o_ap = (int)m.o_ap; pa.o_xm = (int)m.o_xm; pa.o_hb = (int)m.o_hb; pa.o_xo = (int)m.o_xo;
    pa.B = m.B; pa.d = S.s.d_model; pa.ff = S.s.ff; pa.H = S.s.heads; pa.DK = S.s.d_model / S.s.heads; pa.NL = S.s.layers; pa.V = e->vocab();
    pa.Tcap = m.Tcap; pa.R = e->R; pa.PR = e->PR; pa.NS = m.NS;
    pa.act = S.s.act; pa.G = e->persist_grid; pa.KS2 = m.KS2; pa.trace = ptrace;
    { const char* t = getenv("FC_LAURA_PERSIST_TEST"); pa.test_timeout = t && std::string(t) == "timeout"; }
    return pa;
}

// One LM block of the kernel chain's decoding step on B rows, in place on xs: what run_step launches per block, and fc_laura_step_block
// (the per-op test entry) with it.
struct StepBlockBufs {
    float *xs, *qb, *apart, *hb;        // [rows][d] residual stream (in / out), [rows][d] q, [rows][H][NS][DK + 2] partials, [rows][ff]
    float *kc, *vc;                     // this block's caches [rows][d][Tcap], [rows][Tcap][d]
    const int* pos;                     // device [rows]
    int NS;
};
void run_step_block(fc_laura* e, Ctx& cx, const Block& b, const StepBlockBufs& m, int B, int Tcap, int wide, hipStream_t st) {
    const Stack& S = e->codec_lm;
    const int d = S.s.d_model, ff = S.s.ff, heads = S.s.heads, dkh = d / S.s.heads;
    cx.check(step_gemv(b.qkv, m.xs, B, b.n1g, b.n1b, 1e-12f, 0, 2, m.qb, d, st, m.kc, m.vc, m.pos, d, Tcap, nullptr, 0, 0, 0, 0, wide), "QKV GEMV");
    lk::AttnStep a;
    a.q = m.qb; a.kc = m.kc; a.vc = m.vc; a.ptab = b.ptab; a.bias_u = b.bu; a.bias_v = b.bv; a.pos = m.pos; a.part = m.apart; a.NS = m.NS;
    a.B = B; a.H = heads; a.DK = dkh; a.Tcap = Tcap; a.R = e->R; a.PR = e->PR;
    cx.check(lk::launch_attn_step(a, st), "step attention");
    // linear_out reads the key-range partials and combines them while staging its input
    cx.check(step_gemv(b.out, nullptr, B, nullptr, nullptr, 0.f, 0, 1, m.xs, d, st, nullptr, nullptr, nullptr, 0, 0, m.apart, heads, dkh, m.NS, 0, wide), "out GEMV");
    cx.check(step_gemv(b.ff1, m.xs, B, b.n2g, b.n2b, 1e-12f, S.s.act, 0, m.hb, ff, st, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, 0, 0, 0, wide),
             "FFN GEMV 1");
    cx.check(step_gemv(b.ff2, m.hb, B, nullptr, nullptr, 0.f, 0, 1, m.xs, d, st, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, 0, 0, 0, wide),
             "FFN GEMV 2");
}

// One decoding step: the newest token of every row through the LM against its KV cache, then the sampler.  Every kernel reads its
// positions from device memory, so the launch sequence is identical from step to step.  pa null: the kernel chain.
// q (a queued session): the refill phase first -- ended slots retire, free slots claim waiting tickets and draw their first sample.
// rows > 0 (an elastic session of more than 16 slots, the kernel chain): the step over rows [0, rows) only, rows a multiple of 16 below
// m.B.  Every launch is the full step's with its row count cut -- the GEMV's grid.y, the attention's grid.y, the sampler's blocks -- and
// nothing else: the pointers, the layer strides (m.B rows per layer), NS, and the GEMV instantiations over column blocks (Gemv::wide).
// Every step kernel indexes per-row memory from row 0 and no row reads another's, so rows [0, rows) get the full step's bits.
void run_step(fc_laura* e, Ctx& cx, const StepMem& m, const lk::StepPersistArgs* pa, const lk::Sample& sm0, hipStream_t st,
              const lk::QueuePhase* q = nullptr, int rows = 0) {
    const Stack& S = e->codec_lm;
    const int SB = m.B, B = rows > 0 ? rows : m.B, wide = rows > 0 ? 1 : 0;
    lk::Sample sm = sm0;
    if (rows > 0) { sm.row0 = 0; sm.nrows = rows; }
    const int d = S.s.d_model, NL = S.s.layers, V = e->vocab(), Tcap = m.Tcap;
    if (q) {
        cx.check(lk::launch_queue_phase(*q, 1, st), "queue phase");
        lk::Sample first = sm;
        first.launch_seq = nullptr;        // as slots_prefix: only the full-width launch numbers a persistent step
        cx.check(lk::launch_sample_claims(first, *q, st), "sampling of the claimed slots");
    }
    if (pa) {
        cx.check(lk::launch_step_persist(*pa, st), "persistent decoding step");
        cx.check(lk::launch_sample(sm, st), "sampling");
        return;
    }
    for (int i = 0; i < NL; ++i)
        run_step_block(e, cx, S.blocks[i], StepBlockBufs{m.xs, m.qb, m.apart, m.hb, m.kc + (size_t)i * SB * d * Tcap,
                                                         m.vc + (size_t)i * SB * d * Tcap, m.pos, m.NS}, B, Tcap, wide, st);
    cx.check(step_gemv(e->lm_decoder, m.xs, B, S.ag, S.ab, 1e-12f, 0, 0, m.lg, V, st, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, 0, 0, 0, wide),
             "decoder GEMV");
    cx.check(lk::launch_sample(sm, st), "sampling");
}

bool graph_enabled() {
    static const bool on = !(getenv("FC_LAURA_GRAPH") && atoi(getenv("FC_LAURA_GRAPH")) == 0);
    return on;
}

// one step captured on st as an executable graph (62 small launches on the chain: the loop is launch-bound otherwise); null if the
// stream cannot be captured.  A launch that fails while capturing sets cx.err.
hipGraphExec_t capture_step(fc_laura* e, Ctx& cx, const StepMem& m, const lk::StepPersistArgs* pa, const lk::Sample& sm, hipStream_t st,
                            const lk::QueuePhase* q = nullptr, int rows = 0) {
    hipGraphExec_t gexec = nullptr;
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    run_step(e, cx, m, pa, sm, st, q, rows);
    const hipError_t ec = hipStreamEndCapture(st, &graph);
    if (ec != hipSuccess || cx.err || hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0) != hipSuccess) gexec = nullptr;
    if (graph) (void)hipGraphDestroy(graph);
    if (!cx.err) (void)hipGetLastError();
    return gexec;
}

int do_decode(fc_laura* e, Ctx& cx, const float* text_outs, const int32_t* text_lens, int L, const int64_t* continual,
              const int32_t* cont_lens, int Cmax, int max_length, int mode, int ki, float pf, uint64_t seed, const int64_t* forced,
              int64_t* tokens, int32_t* out_lens, float* step_logp, int max_prefix) {
    const Stack& S = e->codec_lm;
    const int B = cx.B, D = e->arch.codebook_dim, V = e->vocab(), d = S.s.d_model;
    const int nq = e->arch.predict_nq, K = e->arch.codebook_size;
    const int T = pad4(max_prefix);
    const int Tcap = pad4(max_prefix + max_length);
    int* tl = upload_lens(cx, text_lens, B);
    int* cl = upload_lens(cx, continual ? cont_lens : nullptr, B, 0);
    int Tt = 0;
    float* tfm = text_to_fm(e, cx, text_outs, tl, L, &Tt);
    float* seq = cx.alloc<float>((size_t)B * D * T);
    int* bidir = cx.alloc<int>(B);
    const StepMem m = alloc_step_mem(e, cx, B, Tcap);
    int* pos = m.pos;
    KvOut kv;
    kv.Tcap = Tcap; kv.kc = m.kc; kv.vc = m.vc; kv.layer_stride = (size_t)B * d * Tcap;
    static const char* trace_path = getenv("FC_LAURA_TRACE");        // tuning aid: s_memtime stamps of the LAST persistent step -> file
    unsigned long long* ptrace = trace_path ? cx.alloc<unsigned long long>((size_t)256 * 64 * 8) : nullptr;
    const bool persist = step_persist_ok(e, m);
    if (cx.live()) {
        cx.check(lk::launch_lm_assemble(tfm, Tt, tl, e->lm_emb, e->cb, K, nq, continual, cl, Cmax, B, D, T, seq, pos, bidir, cx.st), "LM input");
        cx.check(lk::launch_fill_i32(m.ctr, 0, 3 * B + 4, cx.st), "counters");
        cx.check(lk::launch_fill_i32((int*)m.psync, 0, (int)m.sync_words + 32, cx.st), "arrival counters");
        if (continual) hipLaunchKernelGGL(copy_prompt_kernel, dim3(B), dim3(256), 0, cx.st, continual, cl, Cmax, nq, tokens, Cmax + max_length);
    }
    float* h = run_stack_full(e, cx, S, seq, T, pos, e->arch.bidirectional_inputs ? bidir : nullptr, 1, &kv);
    if (cx.dry || cx.err) return cx.err;
    cx.check(lk::launch_gather_last(h, pos, B, d, T, m.xs, cx.st), "last position");
    cx.check(step_gemv(e->lm_decoder, m.xs, B, nullptr, nullptr, 0.f, 0, 0, m.lg, V, cx.st), "decoder GEMV");
    lk::Sample sm = step_sampler(e, m);
    sm.mode = mode; sm.ki = ki; sm.pf = pf; sm.seed = seed; sm.forced = forced; sm.max_steps = max_length;
    sm.tokens = tokens; sm.tok_stride = Cmax + max_length; sm.tok_off = cl; sm.logp_out = step_logp;
    cx.check(lk::launch_sample(sm, cx.st), "sampling");
    int host_done = 0;
    const lk::StepPersistArgs pa = step_persist_args(e, m, ptrace);
    if (ptrace && cx.live()) cx.check(hipMemsetAsync(ptrace, 0, (size_t)256 * 64 * 8 * sizeof(unsigned long long), cx.st), "trace");
    auto step = [&](hipStream_t st) { run_step(e, cx, m, persist ? &pa : nullptr, sm, st); };
    bool timed_out = false;
    auto all_done = [&]() -> bool {       // all utterances finished? (one small read-back)
        unsigned perr = 0;             // both words in the same stream-ordered read-back: one synchronisation, no null-stream copy
        hipError_t ea = hipMemcpyAsync(&host_done, m.n_done(), sizeof(int), hipMemcpyDeviceToHost, cx.st);
        if (ea == hipSuccess && persist) ea = hipMemcpyAsync(&perr, m.error_word(), sizeof(unsigned), hipMemcpyDeviceToHost, cx.st);
        if (ea != hipSuccess || hipStreamSynchronize(cx.st) != hipSuccess) { cx.err = 1; fail("decode_codec: status read-back failed"); return true; }
        if (perr) {                    // stop replaying steps once a hand-off has timed out; the caller re-runs the call on the kernel chain
            cx.err = 1;
            timed_out = true;
            return true;
        }
        return host_done >= B;
    };
    int s = 1;
    if (s < max_length && !cx.err) { step(cx.st); ++s; }              // first step eagerly (also sets the kernels' LDS attributes)
    // the remaining steps replay ONE captured HIP graph of the step
    hipGraphExec_t gexec = nullptr;
    if (graph_enabled() && cx.st != nullptr && max_length - s >= 4 && !cx.err) {
        gexec = capture_step(e, cx, m, persist ? &pa : nullptr, sm, cx.st);
        if (cx.err) return 1;                                           // a launch failed while capturing
    }
    for (; s < max_length && !cx.err; ++s) {
        if (gexec) cx.check(hipGraphLaunch(gexec, cx.st), "graph launch");
        else step(cx.st);
        if ((s & 15) == 15 && s + 1 < max_length && all_done()) break;
    }
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (timed_out) {
        (void)hipStreamSynchronize(cx.st);
        e->persist_on = false;
        return 2;
    }
    if (cx.err) return 1;
    if (persist && ptrace) {
        std::vector<unsigned long long> tr((size_t)256 * 64 * 8);
        HIP_TRY(hipMemcpyAsync(tr.data(), ptrace, tr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, cx.st));
        HIP_TRY(hipStreamSynchronize(cx.st));
        if (FILE* f = fopen(trace_path, "wb")) { fwrite(tr.data(), sizeof(unsigned long long), tr.size(), f); fclose(f); }
    }
    if (persist) {      // a hand-off of the persistent step timed out (a workgroup not resident, a lost store): never a silent result
        unsigned perr = 0;
        HIP_TRY(hipMemcpyAsync(&perr, m.error_word(), sizeof(unsigned), hipMemcpyDeviceToHost, cx.st));
        HIP_TRY(hipStreamSynchronize(cx.st));
        if (perr) {
            e->persist_on = false;         // never a silent result: the caller (fc_laura_decode_codec) re-runs this call on the kernel chain
            return 2;
        }
    }
    std::vector<int> gen(B);
    HIP_TRY(hipMemcpyAsync(gen.data(), m.n_gen(), (size_t)B * sizeof(int), hipMemcpyDeviceToHost, cx.st));
    HIP_TRY(hipStreamSynchronize(cx.st));
    for (int b = 0; b < B; ++b) out_lens[b] = (continual ? cont_lens[b] : 0) + gen[b];
    return 0;
}

// ---- decoding session ----------------------------------------------------------------------------------------------------
enum SlotState { SLOT_FREE = 0, SLOT_RUNNING = 1, SLOT_DONE = 2, SLOT_FAILED = 3 };

// what the host keeps per slot of a decoding session
struct Slot {
    int state = SLOT_FREE, n_gen = 0, cont_len = 0, max_len = 0;
    int text_len = 0, prefix = 0;           // of the prompt the slot holds: text tokens, prefix positions P = text_len + 2 + cont_len
    int forced_on = 0;                      // the slot's utterance follows forced tokens (rows [0, max_len) of its forced row)
    lk::SampleRow rules{};                  // the rule fields only (fc_laura_slots_set_rules): into the slot's row at every start / fork
    bool holds() const { return state == SLOT_RUNNING || state == SLOT_DONE; }     // an utterance, running or ended
};

}  // namespace

// S slots over ONE StepMem of S rows: a slot is a row of the step.  Everything that survives a call lies in the caller's state allocation,
// so every pointer of a step is fixed and the step is captured once.
struct fc_laura_slots {
    fc_laura* e = nullptr;
    int S = 0, R = 0;                       // slots; positions per slot (the pitch of the caches, token and log-probability rows)
    bool with_logp = false, with_score = false;
    StepMem m;
    lk::SampleRow* rows = nullptr;          // device [S]
    int* tok_off = nullptr;                 // device [S]: the slot's continual prompt length
    int64_t *tokens = nullptr, *forced = nullptr;     // [S][R][nq]
    float* logp = nullptr;                  // [S][R][V] or null
    float* score = nullptr;                 // [S][R] or null: the log-probability of every step's picks (sample_kernel)
    float* lg0 = nullptr;                   // [S][V]: the logits every slot's prefix pass ended with (the step overwrites m.lg)
    std::vector<Slot> slot;                 // [S]
    hipGraphExec_t gexec = nullptr;         // the captured step, and the form it holds
    // an elastic session (fc_laura_slots_set_elastic): a call steps the column blocks up to the highest running slot.  Beyond 16 slots one
    // more captured step per cut width, [nb - 1] = the first nb blocks, captured on first use; the full width is gexec, as ever
    bool elastic = false;
    hipGraphExec_t gexec_cut[3] = {nullptr, nullptr, nullptr};
    int last_blocks = 0;                    // column blocks the last step call launched (0: it launched nothing)
    int* move_table = nullptr;              // device [lk::FC_SLOT_MOVES_WORDS]: the lines of the last fc_laura_slots_move
    bool g_persist = false, g_timeout = false;
    bool warmed[2] = {false, false};        // one eager step run per form (sets the kernels' LDS attributes, which a capture cannot)
    bool chain_only = false;                // after a hand-off timeout
    unsigned long long persist_steps = 0;   // persistent launches since the arrival counters were zeroed
    hipStream_t last = nullptr;
    int* status = nullptr;                  // pinned host [2 S + 1]: the read-back of a step (n_gen, done, error word)
    // a queued session (fc_laura_slots_create_queued); Q = 0: none, and nothing below is used
    int Q = 0;                              // result entries
    const fc_laura_slots* from = nullptr;   // the source session: tickets name its rows
    lk::QueuePhase qp;                      // the refill phase's view of both sessions
    struct Entry { int state = 0, ticket = -1, n_tok = 0, n_gen = 0, eos = 0, seq = 0; };   // state: 0 free, 1 waiting or running, 2 finished, 3 failed
    std::vector<Entry> entries;             // host mirror of the result entries, as of the last step's read-back
    std::vector<int> slot_ticket;           // per slot, the ticket it runs (-1: none), as of the last step's read-back
    long long submitted = 0, claimed = 0, finished = 0, collected = 0, failed = 0;
    int queue_words() const { return lk::FC_QUEUE_WORDS + Q * lk::FC_QUEUE_META; }
};

namespace {

void slots_layout(fc_laura* e, Ctx& cx, int S, int R, bool with_logp, bool with_score, fc_laura_slots& s, int Q = 0) {
    const int nq = e->arch.predict_nq, V = e->vocab();
    s.m = alloc_step_mem(e, cx, S, R);
    s.rows = cx.alloc<lk::SampleRow>(S);
    s.tok_off = cx.alloc<int>(S);
    s.tokens = cx.alloc<int64_t>((size_t)S * R * nq);
    s.forced = cx.alloc<int64_t>((size_t)S * R * nq);
    s.logp = with_logp ? cx.alloc<float>((size_t)S * R * V) : nullptr;
    s.lg0 = cx.alloc<float>((size_t)S * V);
    s.score = with_score ? cx.alloc<float>((size_t)S * R) : nullptr;       // behind everything a session without scores has
    if (Q > 0) {                            // behind everything a session without a queue has
        lk::QueuePhase& q = s.qp;
        q.qw = cx.alloc<int>((size_t)lk::FC_QUEUE_WORDS + (size_t)Q * lk::FC_QUEUE_META);
        q.ring = cx.alloc<lk::QueueTicket>(Q);
        q.claims = cx.alloc<lk::QueueClaim>(64);
        q.retires = cx.alloc<lk::QueueRetire>(64);
        q.ring_tokens = cx.alloc<int64_t>((size_t)Q * R * nq);
        q.ring_score = with_score ? cx.alloc<float>((size_t)Q * R) : nullptr;
    }
    s.move_table = cx.alloc<int>(lk::FC_SLOT_MOVES_WORDS);                 // behind everything else (fc_laura_slots_move)
}

lk::Sample slots_sampler(const fc_laura_slots* s) {
    lk::Sample sm = step_sampler(s->e, s->m);
    sm.rows = s->rows; sm.row_stride = s->R; sm.forced = s->forced;
    sm.tokens = s->tokens; sm.tok_stride = s->R; sm.tok_off = s->tok_off; sm.logp_out = s->logp;
    sm.score_out = s->score;
    return sm;
}

// arrival counters to zero, launch number to 1: the first persistent launch after this is launch 1 again
void slots_reset_sync(fc_laura_slots* s, Ctx& cx) {
    cx.check(lk::launch_fill_i32((int*)s->m.psync, 0, (int)s->m.sync_words + 32, cx.st), "arrival counters");
    cx.check(lk::launch_fill_i32((int*)s->m.pseq, 1, 1, cx.st), "launch counter");
    s->persist_steps = 0;
}

// slot `slot` back to "nothing generated" with `row` in the sampling table: slot_reset_kernel.  continual [cont_len][nq]; forced_src
// [row.max_steps][nq] or null
void slot_reset(fc_laura_slots* s, Ctx& cx, int slot, const lk::SampleRow& row, int cont_len, const int64_t* continual, const int64_t* forced_src) {
    const StepMem& m = s->m;
    lk::SlotReset r;
    r.slot = slot; r.n_gen = m.n_gen(); r.done = m.done(); r.step = m.step(); r.pos = m.pos; r.tok_off = s->tok_off;
    r.rows = s->rows; r.row = row; r.xs = m.xs; r.dm = s->e->codec_lm.s.d_model; r.tokens = s->tokens; r.tok_stride = s->R;
    r.nq = s->e->arch.predict_nq; r.cont_len = cont_len; r.continual = continual; r.forced = s->forced; r.forced_src = forced_src;
    r.logp = s->logp; r.V = s->e->vocab(); r.score = s->score;
    cx.check(lk::launch_slot_reset(r, cx.st), "slot reset");
}

// the slot's first sample, from the logits its prefix ended with: the sampler on one row
void sample_first(const fc_laura_slots* s, Ctx& cx, int slot) {
    lk::Sample sm = slots_sampler(s);
    sm.row0 = slot; sm.nrows = 1;
    sm.launch_seq = nullptr;               // only the full-width launch that precedes a persistent step numbers it
    cx.check(lk::launch_sample(sm, cx.st), "sampling");
}

// the first P cache positions and the prefix logits of slot `src` of `from` into slot `dst` of `s` (the same session: dst != src), pos[dst] = P
void prefix_import(fc_laura_slots* s, Ctx& cx, int dst, const fc_laura_slots* from, int src, int P, const char* what) {
    const StepMem& m = s->m;
    lk::PrefixImport c;
    c.kc_src = from->m.kc; c.vc_src = from->m.vc; c.kc_dst = m.kc; c.vc_dst = m.vc;
    c.lg0_src = from->lg0; c.lg_dst = m.lg; c.lg0_dst = s->lg0; c.pos_dst = m.pos;
    c.NL = s->e->codec_lm.s.layers; c.d = s->e->codec_lm.s.d_model; c.V = s->e->vocab();
    c.S_src = from->S; c.Tcap_src = from->m.Tcap; c.S_dst = s->S; c.Tcap_dst = m.Tcap;
    c.P = P; c.src = src; c.dst = dst;
    cx.check(lk::launch_prefix_import(c, cx.st), what);
}

// From here on the slot's previous utterance is gone (a start on a running slot abandons it): the facts of the new prompt, and failed
// until its launches are out.  n_gen > 0: a fork that keeps so many tokens.
void slot_restart(fc_laura_slots* s, int slot, int text_len, int cont_len, int max_length, int forced_on, int n_gen = 0) {
    Slot& x = s->slot[slot];
    x.state = SLOT_FAILED; x.n_gen = n_gen; x.cont_len = cont_len; x.max_len = max_length;
    x.text_len = text_len; x.prefix = text_len + 2 + cont_len; x.forced_on = forced_on;
}

// the prefix pass of ONE prompt (B = 1) into row `slot`, and the slot's first sample
int slots_prefix(fc_laura_slots* s, Ctx& cx, int slot, const float* text_outs, int text_len, const int64_t* continual, int cont_len,
                 const lk::SampleRow& row, const int64_t* forced) {
    fc_laura* e = s->e;
    const Stack& S = e->codec_lm;
    const int D = e->arch.codebook_dim, V = e->vocab(), d = S.s.d_model, nq = e->arch.predict_nq, K = e->arch.codebook_size;
    const int T = pad4(text_len + 2 + cont_len);
    const int32_t tl_h = text_len, cl_h = cont_len;
    int* tl = upload_lens(cx, &tl_h, 1);
    int* cl = upload_lens(cx, &cl_h, 1);
    int Tt = 0;
    float* tfm = text_to_fm(e, cx, text_outs, tl, text_len, &Tt);
    float* seq = cx.alloc<float>((size_t)D * T);
    int* bidir = cx.alloc<int>(1);
    const StepMem& m = s->m;
    int* pos = m.pos ? m.pos + slot : nullptr;
    if (cx.live()) {
        slot_reset(s, cx, slot, row, cont_len, continual, forced);
        cx.check(lk::launch_lm_assemble(tfm, Tt, tl, e->lm_emb, e->cb, K, nq, continual, cl, cont_len, 1, D, T, seq, pos, bidir, cx.st), "LM input");
    }
    KvOut kv;
    kv.Tcap = m.Tcap; kv.kc = m.kc; kv.vc = m.vc;
    kv.layer_stride = (size_t)s->S * d * m.Tcap; kv.row_base = (size_t)slot * d * m.Tcap;
    float* h = run_stack_full(e, cx, S, seq, T, pos, e->arch.bidirectional_inputs ? bidir : nullptr, 1, &kv);
    if (cx.dry || cx.err) return cx.err;
    cx.check(lk::launch_gather_last(h, pos, 1, d, T, m.xs + (size_t)slot * d, cx.st), "last position");
    cx.check(step_gemv(e->lm_decoder, m.xs + (size_t)slot * d, 1, nullptr, nullptr, 0.f, 0, 0, m.lg + (size_t)slot * V, V, cx.st), "decoder GEMV");
    // kept for fc_laura_slots_start_from: the step overwrites the slot's row of m.lg
    cx.check(hipMemcpyAsync(s->lg0 + (size_t)slot * V, m.lg + (size_t)slot * V, (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, cx.st),
             "prefix logits");
    sample_first(s, cx, slot);
    return cx.err;
}

// ONE prefix pass of n different prompts (B = n, T = pad4(Tmax), Tmax >= every row's prefix length) into the rows rs names, and each
// slot's first sample.  Only the stack, the text transpose and the input assembly run at B = n: a column of the stack depends on its own
// row's columns alone, so every slot holds the bits slots_prefix gives it.  What surrounds the stack stays one
// launch per slot, exactly the launches of slots_prefix: the reset, the decoder GEMV on one row, the copy of the prefix logits, the
// one-row sampler.  text_outs [n][L][D], continual [n][Cmax][nq] or null; the lengths are host arrays (null in a dry run).
int slots_prefix_many(fc_laura_slots* s, Ctx& cx, const lk::RowSlots& rs, const float* text_outs, const int32_t* text_lens, int L,
                      const int64_t* continual, const int32_t* cont_lens, int Cmax, const lk::SampleRow* rows, int Tmax) {
    fc_laura* e = s->e;
    const Stack& S = e->codec_lm;
    const int D = e->arch.codebook_dim, V = e->vocab(), d = S.s.d_model, nq = e->arch.predict_nq, K = e->arch.codebook_size;
    const int n = rs.n, T = pad4(Tmax);
    int* tl = upload_lens(cx, text_lens, n);
    int* cl = upload_lens(cx, continual ? cont_lens : nullptr, n, 0);
    int Tt = 0;
    float* tfm = text_to_fm(e, cx, text_outs, tl, L, &Tt);
    float* seq = cx.alloc<float>((size_t)n * D * T);
    int* seq_len = cx.alloc<int>(n);
    int* bidir = cx.alloc<int>(n);
    const StepMem& m = s->m;
    if (cx.live()) {
        for (int b = 0; b < n; ++b) {
            const int cont_len = continual ? cont_lens[b] : 0;
            slot_reset(s, cx, rs.slot[b], rows[b], cont_len, cont_len ? continual + (size_t)b * Cmax * nq : nullptr, nullptr);
        }
        cx.check(lk::launch_lm_assemble(tfm, Tt, tl, e->lm_emb, e->cb, K, nq, continual, cl, Cmax, n, D, T, seq, seq_len, bidir, cx.st), "LM input");
    }
    KvOut kv;
    kv.Tcap = m.Tcap; kv.kc = m.kc; kv.vc = m.vc;
    kv.layer_stride = (size_t)s->S * d * m.Tcap; kv.slots = &rs; kv.S = s->S;
    float* h = run_stack_full(e, cx, S, seq, T, seq_len, e->arch.bidirectional_inputs ? bidir : nullptr, 1, &kv);
    if (cx.dry || cx.err) return cx.err;
    cx.check(lk::launch_gather_last_slots(h, seq_len, rs, s->S, d, T, m.xs, m.pos, cx.st), "last position");
    for (int b = 0; b < n && !cx.err; ++b) {
        const int slot = rs.slot[b];
        cx.check(step_gemv(e->lm_decoder, m.xs + (size_t)slot * d, 1, nullptr, nullptr, 0.f, 0, 0, m.lg + (size_t)slot * V, V, cx.st), "decoder GEMV");
        cx.check(hipMemcpyAsync(s->lg0 + (size_t)slot * V, m.lg + (size_t)slot * V, (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, cx.st),
                 "prefix logits");
        sample_first(s, cx, slot);
    }
    return cx.err;
}

std::string slot_who(int slot) { return "decoding session: slot " + std::to_string(slot); }

// the rules `r` against the sampling mode of the start / start_from / fork / submit that is about to write them; `who` heads the message
int check_rules_mode(const lk::SampleRow& r, int mode, const std::string& who) {
    if (r.top_p > 0.f && mode != 2) return fail(who + "top_p applies with top-k sampling (an integer `sampling`) only");
    if (r.repeat_window > 0 && mode == 0) return fail(who + "the repeat rule needs a drawing mode, not greedy");
    return 0;
}

// what is wrong with a set of rules, as the tail of a message; empty: nothing
std::string rules_problem(float temperature, int min_length, float top_p, int repeat_window, int repeat_count) {
    if (!std::isfinite(temperature) || !(temperature > 0.f)) return "temperature must be finite and > 0";
    if (min_length < 0) return "min_length " + std::to_string(min_length) + " < 0";
    if (!(top_p >= 0.f && top_p <= 1.f)) return "top_p must lie in (0, 1], or be 0 for none";
    if (repeat_window < 0 || repeat_window > 256) return "repeat_window " + std::to_string(repeat_window) + " outside 0 .. 256";
    if (repeat_window > 0 && (repeat_count < 1 || repeat_count > repeat_window))
        return "repeat_count " + std::to_string(repeat_count) + " outside 1 .. repeat_window " + std::to_string(repeat_window);
    return "";
}

// checked rules as a row that holds the rule fields only
lk::SampleRow rules_row(float temperature, int min_length, float top_p, int repeat_window, int repeat_count) {
    lk::SampleRow r{};
    r.temperature = temperature; r.min_length = min_length; r.top_p = top_p;
    r.repeat_window = repeat_window; r.repeat_count = repeat_window > 0 ? repeat_count : 1;
    return r;
}

// a row of the sampling table: `rules` (the rule fields of a slot or a ticket) with the sampling of one utterance
lk::SampleRow make_row(const lk::SampleRow& rules, int mode, int k, float p, int max_length, uint64_t seed, int forced_on) {
    lk::SampleRow row = rules;
    row.mode = mode; row.ki = k; row.pf = p; row.max_steps = max_length; row.seed = seed;
    row.forced_on = forced_on; row.rng_row = 0u;           // the slot index is NOT in the Philox counter: a slot's draws are its own
    return row;
}

const char* sampling_problem(int mode, int k, float p) {
    if (mode < 0 || mode > 3) return "sampling_mode must be 0..3";
    if (mode == 2 && k < 1) return "top-k sampling needs sampling_k >= 1";
    if (mode == 3 && !(p > 0.f)) return "nucleus sampling needs sampling_p > 0";
    return nullptr;
}

int check_sampling(int mode, int k, float p) {
    const char* why = sampling_problem(mode, k, p);
    return why ? fail(why) : 0;
}

// Slot `src` of session `from` as the source of a copy: in range, and it holds an utterance.  `who` names it at the head of both messages
// and `of` follows its range; a submit names the row otherwise in the second message (`holder`) and says a prompt is what it holds.
int check_source(const fc_laura_slots* from, int src, const std::string& who, const std::string& of = "", std::string holder = "",
                 const char* holds = " holds no utterance (") {
    if (src < 0 || src >= from->S) return fail(who + " outside 0 .. " + std::to_string(from->S - 1) + of);
    if (holder.empty()) holder = who + of;
    if (!from->slot[src].holds())
        return fail(holder + holds + (from->slot[src].state == SLOT_FAILED ? "failed" : "free or never started") + ")");
    return 0;
}

// a prompt of P prefix positions and max_length steps in a session of R positions per slot
int check_fits(const std::string& who, int P, int max_length, int R) {
    if (P + max_length <= R) return 0;
    return fail(who + "text_len + 2 + cont_len + max_length = " + std::to_string(P + max_length) + " exceeds the session's max_positions " +
                std::to_string(R));
}

// Slot `dst` of `s` from the prompt slot `src` of `from` holds (the same session or another of the engine): the reset, the copy of the
// source's prefix, the first sample from the prefix logits.  The caller has checked everything.  The same slot (a rewind to nothing
// generated) keeps its own prefix and needs no copy.
int slots_from_prefix(fc_laura_slots* s, int dst, const fc_laura_slots* from, int src, int max_length, int sampling_mode, int sampling_k,
                      float sampling_p, uint64_t seed, const int64_t* forced, void* stream) {
    const Slot& held = from->slot[src];
    const int P = held.prefix, cont_len = held.cont_len;
    const StepMem& m = s->m;
    const int V = s->e->vocab();
    const lk::SampleRow row = make_row(s->slot[dst].rules, sampling_mode, sampling_k, sampling_p, max_length, seed, forced ? 1 : 0);
    slot_restart(s, dst, held.text_len, cont_len, max_length, forced ? 1 : 0);
    Ctx cx = make_ctx(1, (void*)m.pos, 0, stream);          // launches only: nothing is allocated
    s->last = cx.st;
    // the source's prompt tokens, in its session's token row: generation never changes rows [0, cont_len)
    slot_reset(s, cx, dst, row, cont_len, from->tokens + (size_t)src * from->R * s->e->arch.predict_nq, forced);
    if (from != s || dst != src) {
        prefix_import(s, cx, dst, from, src, P, from != s ? "prefix import" : "prefix copy");
    } else {
        cx.check(hipMemcpyAsync(m.lg + (size_t)dst * V, s->lg0 + (size_t)dst * V, (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, cx.st),
                 "prefix logits");
        cx.check(lk::launch_fill_i32(m.pos + dst, P, 1, cx.st), "position");
    }
    sample_first(s, cx, dst);
    if (cx.err) return 1;
    s->slot[dst].state = SLOT_RUNNING;
    return 0;
}

// a queued session is fed by its queue only: the calls that put a prompt into a slot or take one out are refused, changing nothing
int refuse_queued(const fc_laura_slots* s, const char* call) {
    if (!s->Q) return 0;
    return fail(std::string("decoding session: ") + call + ": a queued session is fed by its queue only (fc_laura_slots_submit, fc_laura_slots_collect)");
}

void slots_report(const fc_laura_slots* s, int32_t* done_out, int32_t* n_gen_out) {
    for (int i = 0; i < s->S; ++i) {
        if (done_out) done_out[i] = s->slot[i].state;
        if (n_gen_out) n_gen_out[i] = s->slot[i].n_gen;
    }
}

// After a hand-off of the persistent step timed out (the caller has failed what ran): the session stays on the kernel chain, the event
// is counted, and the device words go back to "nothing runs" -- every slot ended, of a queued session no slot with a ticket, the
// arrival counters at zero.  Never a silent result.
int after_timeout(fc_laura_slots* s, Ctx& cx) {
    s->chain_only = true;
    s->e->persist_fallbacks++;
    if (s->gexec) { (void)hipGraphExecDestroy(s->gexec); s->gexec = nullptr; }
    cx.check(lk::launch_fill_i32(s->m.done(), 1, s->S, cx.st), "done flags");
    if (s->Q) cx.check(lk::launch_fill_i32(s->qp.qw + lk::FC_QUEUE_SLOT_TICKET, -1, 64, cx.st), "slot tickets");
    slots_reset_sync(s, cx);
    if (hipStreamSynchronize(cx.st) != hipSuccess || cx.err) return fail("decoding session: reset after a timed-out step failed");
    return 0;
}

// The host's side of a queued session's step, behind the read-back: the mirrors of the counters, the slots' tickets and the result
// entries.  A hand-off time-out of the persistent step fails every ticket that ran in this call -- those still in a slot and those the
// call retired, whose tokens come from steps that cannot be trusted -- and the queue goes on over the kernel chain.
int queue_after_step(fc_laura_slots* s, Ctx& cx, hipError_t ea, int32_t* done_out, int32_t* n_gen_out) {
    const int S = s->S, Q = s->Q;
    const int* host = s->status;
    const int* qw = host + 2 * S + 1;
    if (ea != hipSuccess) {
        if (!cx.err) fail(std::string("decoding session: status read-back failed: ") + hipGetErrorString(ea));
        return 1;
    }
    const unsigned perr = (unsigned)host[2 * S];
    s->claimed = qw[lk::FC_QUEUE_HEAD];
    for (int en = 0; en < Q; ++en) {
        const int* meta = qw + lk::FC_QUEUE_WORDS + en * lk::FC_QUEUE_META;
        fc_laura_slots::Entry& E = s->entries[en];
        if (E.state != 1 || meta[lk::FC_QMETA_STATE] != 2 || meta[lk::FC_QMETA_TICKET] != E.ticket) continue;
        if (perr) { E.state = 3; s->failed++; continue; }
        E.state = 2; E.n_tok = meta[lk::FC_QMETA_NTOK]; E.n_gen = meta[lk::FC_QMETA_NGEN]; E.eos = meta[lk::FC_QMETA_EOS];
        E.seq = meta[lk::FC_QMETA_SEQ];
        s->finished++;
    }
    for (int i = 0; i < S; ++i) {
        s->slot_ticket[i] = qw[lk::FC_QUEUE_SLOT_TICKET + i];
        const bool runs = s->slot_ticket[i] >= 0;
        s->slot[i].state = runs ? (host[S + i] ? SLOT_DONE : SLOT_RUNNING) : SLOT_FREE;
        s->slot[i].n_gen = runs ? host[i] : 0;
    }
    if (perr) {
        for (int i = 0; i < S; ++i) {
            if (s->slot_ticket[i] < 0) continue;
            fc_laura_slots::Entry& E = s->entries[qw[lk::FC_QUEUE_SLOT_ENTRY + i]];
            if (E.state == 1 && E.ticket == s->slot_ticket[i]) { E.state = 3; s->failed++; }
            s->slot_ticket[i] = -1;
            s->slot[i].state = SLOT_FREE; s->slot[i].n_gen = 0;
        }
        if (after_timeout(s, cx)) return 1;
    }
    slots_report(s, done_out, n_gen_out);
    return 0;
}

int check_ready(fc_laura* e) {
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("engine not finalized");
    HIP_TRY(hipSetDevice(e->device));
    return 0;
}

int check_stack(const fc_laura_stack& s, const char* name, bool step = false) {
    if (s.idim < 1 || s.d_model < 64 || s.heads < 1 || s.ff < 16 || s.layers < 1) return fail(std::string(name) + ": bad sizes");
    if (s.d_model % s.heads) return fail(std::string(name) + ": d_model must be a multiple of heads");
    const int dk = s.d_model / s.heads;
    if (dk != 32 && dk != 64) return fail(std::string(name) + ": head dimension must be 32 or 64");
    if (s.d_model % 16 || s.ff % 16) return fail(std::string(name) + ": d_model and ff must be multiples of 16");
    if (s.act != 1 && s.act != 2) return fail(std::string(name) + ": activation must be 1 (relu) or 2 (swish)");
    // limits of the kernels, refused HERE with a reason instead of a hipErrorInvalidValue at the first call: the LayerNorm kernels
    // and the sampler's fused input layer hold a row of <= 1024 channels; the step form's GEMV stages (16 + 1) x (K + 4) floats of input
    // plus 16 KiB of partial tiles in the 160 KiB of LDS, K = ff for w_2 (ff <= 2112), or stages them in windows of <= 1024 columns
    // (launch_gemv); windows are accepted up to ff = 4 d, the ratio of both recipes
    if (s.d_model > 1024) return fail(std::string(name) + ": d_model above 1024 is not supported (LayerNorm / sampler kernels)");
    if (step && !(s.ff <= 2112 || s.ff <= 4 * s.d_model))
        return fail(std::string(name) + ": feed-forward width too large for the decoding step's GEMV: ff <= 2112 or ff <= 4 * d_model");
    return 0;
}

}  // namespace

extern "C" {

int fc_laura_create(const fc_laura_arch* arch, int device, fc_laura** out) {
    if (!arch || !out) return fail("null argument");
    if (arch->abi_version != FC_ABI_VERSION) return fail("fc_laura_arch.abi_version mismatch");
    if (arch->codebook_size != 1024) return fail("codebook_size must be 1024 (the reference's codec_index_shift is hard-wired to it)");
    if (arch->predict_nq < 1 || arch->predict_nq > 8 || arch->predict_nq > arch->num_quantizers) return fail("bad predict_nq");
    if (arch->codebook_dim % 16 || arch->codebook_dim < 16) return fail("codebook_dim must be a multiple of 16");
    if (arch->max_positions < 16 || arch->max_positions > 2048) return fail("max_positions must be in [16, 2048]");
    if (arch->max_positions % 4) return fail("max_positions must be a multiple of 4 (time axes are padded to whole quads)");
    if (check_stack(arch->text_encoder, "text_encoder") || check_stack(arch->codec_lm, "codec_lm", true) ||
        check_stack(arch->codec_encoder, "codec_encoder")) return 1;
    if (arch->codec_lm.idim != arch->codebook_dim || arch->codec_encoder.idim != arch->codebook_dim)
        return fail("codec_lm / codec_encoder input width must equal codebook_dim");
    if (arch->text_encoder.idim != arch->input_size) return fail("text_encoder input width must equal input_size");
    auto e = std::make_unique<fc_laura>();
    e->arch = *arch;
    e->device = device;
    e->R = arch->max_positions;
    e->PR = pad4(2 * e->R - 1);
    const int D = arch->codebook_dim;
    plan_stack(e.get(), e->text_encoder, "text_encoder", arch->text_encoder, false);
    e->text_out = mk_lin(e.get(), "text_enc_out_layer", arch->text_encoder.d_model, D, true);
    if (arch->vocab_size > 0) expect(e.get(), "token_embedding.weight", {arch->vocab_size, arch->input_size});
    expect(e.get(), "lm_embedding.weight", {2, D});
    plan_stack(e.get(), e->codec_lm, "codec_lm.encoder", arch->codec_lm, true);
    e->lm_decoder = mk_lin(e.get(), "codec_lm.decoder", arch->codec_lm.d_model, e->vocab(), true);
    plan_stack(e.get(), e->codec_encoder, "codec_encoder", arch->codec_encoder, false);
    e->codec_out = mk_lin(e.get(), "codec_encoder_out_layer", arch->codec_encoder.d_model, D, true);
    expect(e.get(), "quantizer_codebook.embed", {arch->num_quantizers, arch->codebook_size, D});
    register_lins(e.get());
    *out = e.release();
    return 0;
}

void fc_laura_destroy(fc_laura* e) {
    if (!e) return;
    for (void* p : e->dev_allocs) (void)hipFree(p);
    delete e;
}

int fc_laura_num_weights(const fc_laura* e) { return e ? (int)e->expected.size() : 0; }

int fc_laura_weight_info(const fc_laura* e, int i, const char** name, int64_t* dims) {
    if (!e || i < 0 || i >= (int)e->expected.size()) return -1;
    *name = e->expected[i].first.c_str();
    const auto& d = e->expected[i].second;
    for (size_t k = 0; k < d.size(); ++k) dims[k] = d[k];
    return (int)d.size();
}

int fc_laura_set_weight(fc_laura* e, const char* name, const float* host, const int64_t* dims, int ndim) {
    if (!e || !name || !host) return fail("null argument");
    for (const auto& ex : e->expected) {
        if (ex.first != name) continue;
        size_t n = 1;
        bool ok = (int)ex.second.size() == ndim;
        for (int k = 0; ok && k < ndim; ++k) { ok = ex.second[k] == dims[k]; n *= (size_t)dims[k]; }
        if (!ok) return fail(std::string("shape mismatch for ") + name);
        HostTensor& t = e->host[name];
        t.dims.assign(dims, dims + ndim);
        t.data.assign(host, host + n);
        t.set = true;
        return 0;
    }
    fail(std::string("unknown weight: ") + name);
    return 2;
}

int fc_laura_finalize(fc_laura* e) {
    if (!e) return fail("null engine");
    if (e->finalized) return 0;
    for (const auto& ex : e->expected)
        if (!e->host.count(ex.first) || !e->host[ex.first].set) return fail("missing weight: " + ex.first);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= e->device) return fail("no HIP device: the engine has no CPU path");
    HIP_TRY(hipSetDevice(e->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, e->device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) return fail(std::string("gfx950 (MI355X) required, found ") + prop.gcnArchName);
    // relative-position encodings, one table per distinct model width
    std::map<int, float*> pe_dev;
    for (Stack* S : {&e->text_encoder, &e->codec_lm, &e->codec_encoder}) {
        const int d = S->s.d_model;
        if (!pe_dev.count(d)) {
            float* p = nullptr;
            if (upload(e, rel_pe_fm(d, e->R, e->PR), &p)) return 1;
            pe_dev[d] = p;
        }
        if (pack_stack(e, *S, pe_dev[d], nullptr, 0)) return 1;
    }
    {
        const auto& W = e->host["codec_lm.encoder.embed.0.weight"].data;       // [d][D]
        const int d = e->arch.codec_lm.d_model, D = e->arch.codebook_dim;
        std::vector<float> wt((size_t)D * d);
        for (int n = 0; n < d; ++n)
            for (int k = 0; k < D; ++k) wt[(size_t)k * d + n] = W[(size_t)n * D + k];
        if (upload(e, wt, &e->lm_embed_wt)) return 1;
    }
    if (pack_lin(e, e->text_out, false)) return 1;
    if (pack_lin(e, e->lm_decoder, true)) return 1;
    if (pack_lin(e, e->codec_out, false)) return 1;
    if (upload(e, e->host["lm_embedding.weight"].data, &e->lm_emb)) return 1;
    if (upload(e, e->host["quantizer_codebook.embed"].data, &e->cb)) return 1;
    if (e->arch.vocab_size > 0 && upload(e, e->host["token_embedding.weight"].data, &e->tok_emb)) return 1;
    {   // PositionalEncoding table of width codebook_dim (embedding.py:63-77), token-major [R][D]
        const int D = e->arch.codebook_dim;
        std::vector<float> pe((size_t)e->R * D);
        for (int m = 0; m < D / 2; ++m) {
            const float div = expf((float)(2 * m) * (float)(-(std::log(10000.0) / (double)D)));
            for (int r = 0; r < e->R; ++r) {
                pe[(size_t)r * D + 2 * m] = sinf((float)r * div);
                pe[(size_t)r * D + 2 * m + 1] = cosf((float)r * div);
            }
        }
        if (upload(e, pe, &e->pe_abs)) return 1;
    }
    {   // the persistent decoding step's view of the LM blocks
        const Stack& S = e->codec_lm;
        std::vector<lk::StepLayer> tab(S.blocks.size());
        for (size_t i = 0; i < S.blocks.size(); ++i) {
            const Block& b = S.blocks[i];
            tab[i] = lk::StepLayer{b.qkv.wf, b.qkv.bias, b.out.wf, b.out.bias, b.ff1.wf, b.ff1.bias, b.ff2.wf, b.ff2.bias,
                                   b.n1g, b.n1b, b.n2g, b.n2b, b.bu, b.bv, b.ptab};
        }
        if (upload(e, tab, &e->step_layers)) return 1;
        e->persist_grid = lk::step_persist_grid(e->device, S.s.d_model, S.s.ff);
    }
    e->host.clear();
    e->finalized = true;
    return 0;
}

size_t fc_laura_workspace_bytes(const fc_laura* ce, int B, int L, int Cmax, int max_length) {
    fc_laura* e = const_cast<fc_laura*>(ce);
    if (!e || B < 1 || L < 1) return 0;
    size_t need = 0;
    std::vector<int32_t> tl(B, L), cl(B, Cmax);
    {
        Ctx cx = make_ctx(B, nullptr, 0, nullptr);
        do_encode(e, cx, nullptr, nullptr, tl.data(), L, nullptr);
        need = std::max(need, cx.off);
    }
    {
        Ctx cx = make_ctx(B, nullptr, 0, nullptr);
        do_lm_logprobs(e, cx, nullptr, tl.data(), L, nullptr, cl.data(), Cmax, nullptr, L + 2 + Cmax + max_length);
        need = std::max(need, cx.off);
    }
    {
        Ctx cx = make_ctx(B, nullptr, 0, nullptr);
        do_codec_emb(e, cx, nullptr, tl.data(), L, nullptr, 1, cl.data(), Cmax + max_length, nullptr, L + Cmax + max_length);
        need = std::max(need, cx.off);
    }
    {
        Ctx cx = make_ctx(B, nullptr, 0, nullptr);
        do_decode(e, cx, nullptr, tl.data(), L, nullptr, cl.data(), Cmax, max_length > 0 ? max_length : 1, 0, 0, 0.f, 0, nullptr, nullptr,
                  nullptr, nullptr, L + 2 + Cmax);
        need = std::max(need, cx.off);
    }
    return need + 4096;
}

int fc_laura_encode(fc_laura* e, const float* text_emb, const int64_t* text_ids, const int32_t* text_lens, int B, int L, float* text_outs,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if ((text_emb == nullptr) == (text_ids == nullptr)) return fail("exactly one of text_emb / text_ids");
    if (text_ids && e->arch.vocab_size <= 0) return fail("the checkpoint has no token_embedding");
    if (!text_lens || !text_outs || !workspace || B < 1 || L < 1) return fail("bad argument");
    if (L > e->R) return fail("text longer than max_positions");
    if (check_lens(text_lens, B, 1, L, "text_lens")) return 1;
    Ctx cx = make_ctx(B, workspace, workspace_bytes, stream);
    return do_encode(e, cx, text_emb, text_ids, text_lens, L, text_outs);
}

int fc_laura_lm_logprobs(fc_laura* e, const float* text_outs, const int32_t* text_lens, int B, int L, const int64_t* codec,
                         const int32_t* codec_lens, int Cmax, float* logp, int Tseq, void* workspace, size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!text_outs || !text_lens || !logp || !workspace || B < 1 || L < 1) return fail("bad argument");
    if (check_lens(text_lens, B, 1, L, "text_lens")) return 1;
    if (codec && (!codec_lens || check_lens(codec_lens, B, 0, Cmax, "codec_lens"))) return fail("bad codec_lens");
    int need = 0;
    for (int b = 0; b < B; ++b) need = std::max(need, text_lens[b] + 2 + (codec ? codec_lens[b] : 0));
    if (Tseq < need) return fail("Tseq too small");
    if (Tseq > e->R) return fail("sequence longer than max_positions");
    Ctx cx = make_ctx(B, workspace, workspace_bytes, stream);
    return do_lm_logprobs(e, cx, text_outs, text_lens, L, codec, codec_lens, Cmax, logp, Tseq);
}

int fc_laura_decode_codec(fc_laura* e, const float* text_outs, const int32_t* text_lens, int B, int L, const int64_t* continual,
                          const int32_t* cont_lens, int Cmax, int max_length, int sampling_mode, int sampling_k, float sampling_p,
                          uint64_t seed, const int64_t* forced, int64_t* tokens, int32_t* out_lens, float* step_logp, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!text_outs || !text_lens || !tokens || !out_lens || !workspace || B < 1 || B > 16 || L < 1 || max_length < 1)
        return fail("bad argument (1 <= B <= 16 utterances per call)");
    if (check_sampling(sampling_mode, sampling_k, sampling_p)) return 1;
    if (check_lens(text_lens, B, 1, L, "text_lens")) return 1;
    if (continual && (!cont_lens || check_lens(cont_lens, B, 0, Cmax, "cont_lens"))) return fail("bad cont_lens");
    int prefix = 0;
    for (int b = 0; b < B; ++b) prefix = std::max(prefix, text_lens[b] + 2 + (continual ? cont_lens[b] : 0));
    if (prefix + max_length > e->R) return fail("prefix + max_length exceeds max_positions");
    Ctx cx = make_ctx(B, workspace, workspace_bytes, stream);
    int rc = do_decode(e, cx, text_outs, text_lens, L, continual, cont_lens, Cmax < 0 ? 0 : Cmax, max_length, sampling_mode, sampling_k,
                       sampling_p, seed, forced, tokens, out_lens, step_logp, prefix);
    if (rc == 2) {
        // A hand-off of the persistent decoding step timed out (its workgroups were not all resident: another stream or process held CUs --
        // the launch is not cooperative; or a lost store).  Bounded spins, the launch has ended, nothing of its output is used: THIS call is
        // run again from the start on the kernel chain (a generation is a function of its seed, so the result is the one the chain gives),
        // later calls stay on the chain until fc_laura_set_persistent_step(e, 1).  The event is counted, not hidden.
        e->persist_fallbacks++;
        Ctx cx2 = make_ctx(B, workspace, workspace_bytes, stream);
        rc = do_decode(e, cx2, text_outs, text_lens, L, continual, cont_lens, Cmax < 0 ? 0 : Cmax, max_length, sampling_mode, sampling_k,
                       sampling_p, seed, forced, tokens, out_lens, step_logp, prefix);
        if (rc == 2) return fail("decode_codec: the decoding step timed out on the kernel chain as well");
    }
    return rc;
}

int fc_laura_persistent_step_fallbacks(const fc_laura* e) { return e ? e->persist_fallbacks : -1; }

/* ---- decoding session: S slots that start and end independently in one running batch ---- */
// What is wrong with the sizes of a session, for the create and the state-bytes side alike (e is not null); empty: nothing.  max_slots is
// 16 for the calls that predate the wide session, and they say so.
static std::string create_problem(const fc_laura* e, int slots, int max_positions, int max_slots) {
    if (slots < 1 || slots > max_slots)
        return (max_slots > 16 ? "a wide decoding session has 1 .. 64 slots (4 column blocks of the step form's 16 MFMA columns), got "
                               : "a decoding session has 1 .. 16 slots (the step form's 16 MFMA columns), got ") + std::to_string(slots);
    if (max_positions < 16 || max_positions % 4 || max_positions > e->R)
        return "a decoding session's max_positions must be a multiple of 4 in [16, " + std::to_string(e->R) + "] (the engine's), got " +
               std::to_string(max_positions);
    return "";
}
static std::string queue_problem(int queue) {
    if (queue < 1 || queue > 65536) return "a queued decoding session has 1 .. 65536 result entries, got " + std::to_string(queue);
    return "";
}

// every byte count: queue = 0 is the session without a queue
static size_t slots_state_bytes(const fc_laura* ce, int slots, int max_positions, int with_logp, int with_score, int queue, int max_slots) {
    fc_laura* e = const_cast<fc_laura*>(ce);
    if (!e || !create_problem(e, slots, max_positions, max_slots).empty()) return 0;
    Ctx cx = make_ctx(slots, nullptr, 0, nullptr);
    fc_laura_slots s;
    slots_layout(e, cx, slots, max_positions, with_logp != 0, with_score != 0, s, queue);
    return cx.off + 4096;
}

size_t fc_laura_slots_state_bytes(const fc_laura* e, int slots, int max_positions, int with_logp) {
    return slots_state_bytes(e, slots, max_positions, with_logp, 0, 0, 16);
}

size_t fc_laura_slots_state_bytes_scored(const fc_laura* e, int slots, int max_positions, int with_logp, int with_score) {
    return slots_state_bytes(e, slots, max_positions, with_logp, with_score, 0, 16);
}

size_t fc_laura_slots_state_bytes_wide(const fc_laura* e, int slots, int max_positions, int with_logp, int with_score) {
    return slots_state_bytes(e, slots, max_positions, with_logp, with_score, 0, 64);
}

size_t fc_laura_slots_state_bytes_queued(const fc_laura* e, int slots, int max_positions, int with_score, int queue) {
    return queue_problem(queue).empty() ? slots_state_bytes(e, slots, max_positions, 0, with_score, queue, 64) : 0;
}

// every create: Q = 0 is the session without a queue, call for call what fc_laura_slots_create_wide always did
static int slots_create(fc_laura* e, int slots, int max_positions, int with_logp, int with_score, int Q, const fc_laura_slots* from,
                        void* state, size_t state_bytes, fc_laura_slots** out, int max_slots = 64) {
    if (check_ready(e)) return 1;
    const std::string why = create_problem(e, slots, max_positions, max_slots);
    if (!why.empty()) return fail(why);
    if (!state || !out) return fail("null argument");
    auto s = std::make_unique<fc_laura_slots>();
    s->e = e; s->S = slots; s->R = max_positions; s->with_logp = with_logp != 0; s->with_score = with_score != 0;
    Ctx cx = make_ctx(slots, state, state_bytes, nullptr);
    slots_layout(e, cx, slots, max_positions, s->with_logp, s->with_score, *s, Q);
    if (cx.err) return fail("decoding session: state allocation too small (fc_laura_slots_state_bytes)");
    s->slot.assign(slots, Slot{});                          // free, the neutral rules
    // a never-started slot: done = 1, pos = 0, a zero xs row -- it goes through every step with finite values and the sampler skips it
    const StepMem& m = s->m;
    const Stack& S = e->codec_lm;
    const int d = S.s.d_model, heads = S.s.heads, dkh = d / heads;
    HIP_TRY(hipMemset(m.pos, 0, (size_t)slots * sizeof(int)));
    HIP_TRY(hipMemset(m.ctr, 0, (size_t)(3 * slots + 4) * sizeof(int)));
    const size_t RW = (size_t)step_rows(slots);
    HIP_TRY(hipMemset(m.xs, 0, RW * d * sizeof(float)));
    HIP_TRY(hipMemset(m.qb, 0, RW * d * sizeof(float)));
    HIP_TRY(hipMemset(m.apart, 0, RW * heads * 8 * (dkh + 2) * sizeof(float)));
    HIP_TRY(hipMemset(m.hb, 0, RW * S.s.ff * sizeof(float)));
    HIP_TRY(hipMemset(m.lg, 0, RW * e->vocab() * sizeof(float)));
    HIP_TRY(hipMemset(m.nemb, 0, RW * e->arch.codebook_dim * sizeof(float)));
    HIP_TRY(hipMemset(m.edge, 0, m.edge_stride * S.s.layers * sizeof(float)));
    HIP_TRY(hipMemset(m.psync, 0, (m.sync_words + 32) * sizeof(unsigned)));
    const std::vector<lk::SampleRow> neutral(slots, lk::SampleRow{});
    HIP_TRY(hipMemcpy(s->rows, neutral.data(), (size_t)slots * sizeof(lk::SampleRow), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(s->tok_off, 0, (size_t)slots * sizeof(int)));
    if (s->score) HIP_TRY(hipMemset(s->score, 0, (size_t)slots * max_positions * sizeof(float)));
    std::vector<int> ones(slots, 1);
    const unsigned one = 1u;
    HIP_TRY(hipMemcpy(m.done(), ones.data(), (size_t)slots * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m.pseq, &one, sizeof(unsigned), hipMemcpyHostToDevice));
    if (Q > 0) {
        // the queue: nothing waits, no slot runs a ticket, every result entry is free
        s->Q = Q; s->from = from;
        s->entries.assign(Q, fc_laura_slots::Entry{});
        s->slot_ticket.assign(slots, -1);
        lk::QueuePhase& q = s->qp;
        q.Q = Q; q.S = slots;
        q.n_gen = m.n_gen(); q.done = m.done(); q.step = m.step(); q.pos = m.pos; q.tok_off = s->tok_off; q.rows = s->rows;
        q.tokens = s->tokens; q.score = s->score; q.xs = m.xs; q.kc = m.kc; q.vc = m.vc; q.lg = m.lg; q.lg0 = s->lg0;
        q.R = max_positions; q.nq = e->arch.predict_nq; q.dm = d; q.NL = S.s.layers; q.d = d; q.V = e->vocab();
        q.kc_src = from->m.kc; q.vc_src = from->m.vc; q.lg0_src = from->lg0; q.tokens_src = from->tokens; q.S_src = from->S; q.R_src = from->R;
        std::vector<int> words((size_t)s->queue_words(), 0);
        for (int i = 0; i < 64; ++i) words[lk::FC_QUEUE_SLOT_TICKET + i] = -1;
        HIP_TRY(hipMemcpy(q.qw, words.data(), words.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipHostMalloc((void**)&s->status, (size_t)(2 * slots + 1 + (Q > 0 ? s->queue_words() : 0)) * sizeof(int), hipHostMallocDefault));
    *out = s.release();
    return 0;
}

int fc_laura_slots_create(fc_laura* e, int slots, int max_positions, int with_logp, void* state, size_t state_bytes, fc_laura_slots** out) {
    return slots_create(e, slots, max_positions, with_logp, 0, 0, nullptr, state, state_bytes, out, 16);
}

int fc_laura_slots_create_scored(fc_laura* e, int slots, int max_positions, int with_logp, int with_score, void* state, size_t state_bytes,
                                 fc_laura_slots** out) {
    return slots_create(e, slots, max_positions, with_logp, with_score, 0, nullptr, state, state_bytes, out, 16);
}

int fc_laura_slots_create_wide(fc_laura* e, int slots, int max_positions, int with_logp, int with_score, void* state, size_t state_bytes,
                               fc_laura_slots** out) {
    return slots_create(e, slots, max_positions, with_logp, with_score, 0, nullptr, state, state_bytes, out);
}

int fc_laura_slots_create_queued(fc_laura* e, int slots, int max_positions, int with_score, int queue, const fc_laura_slots* source,
                                 void* state, size_t state_bytes, fc_laura_slots** out) {
    if (check_ready(e)) return 1;
    const std::string why = queue_problem(queue);
    if (!why.empty()) return fail(why);
    if (!source) return fail("a queued decoding session needs a source session (its tickets name the source's rows)");
    if (source->e != e) return fail("a queued decoding session: the source session belongs to another engine (other weights: its prefix is not this engine's)");
    if (source->Q) return fail("a queued decoding session: the source session is itself queued (it holds no prompts)");
    return slots_create(e, slots, max_positions, 0, with_score, queue, source, state, state_bytes, out);
}

void fc_laura_slots_destroy(fc_laura_slots* s) {
    if (!s) return;
    if (s->gexec) (void)hipGraphExecDestroy(s->gexec);
    for (hipGraphExec_t g : s->gexec_cut)
        if (g) (void)hipGraphExecDestroy(g);
    if (s->status) (void)hipHostFree(s->status);
    delete s;
}

size_t fc_laura_slots_workspace_bytes(const fc_laura_slots* cs, int L, int Cmax) {
    fc_laura_slots* s = const_cast<fc_laura_slots*>(cs);
    if (!s || L < 1 || Cmax < 0) return 0;
    Ctx cx = make_ctx(1, nullptr, 0, nullptr);
    slots_prefix(s, cx, 0, nullptr, L, nullptr, Cmax, lk::SampleRow{}, nullptr);
    return cx.off + 4096;
}

int fc_laura_slots_start(fc_laura_slots* s, int slot, const float* text_outs, int text_len, const int64_t* continual, int cont_len,
                         int max_length, int sampling_mode, int sampling_k, float sampling_p, uint64_t seed, const int64_t* forced,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!s) return fail("null session");
    if (refuse_queued(s, "start")) return 1;
    if (check_ready(s->e)) return 1;
    if (slot < 0 || slot >= s->S) return fail("decoding session: slot " + std::to_string(slot) + " outside 0 .. " + std::to_string(s->S - 1));
    if (!text_outs || !workspace || text_len < 1 || max_length < 1 || cont_len < 0 || (cont_len > 0 && !continual))
        return fail("decoding session: bad argument for slot " + std::to_string(slot));
    if (check_sampling(sampling_mode, sampling_k, sampling_p) || check_rules_mode(s->slot[slot].rules, sampling_mode, slot_who(slot) + ": ")) return 1;
    if (check_fits(slot_who(slot) + ": ", text_len + 2 + cont_len, max_length, s->R)) return 1;
    const lk::SampleRow row = make_row(s->slot[slot].rules, sampling_mode, sampling_k, sampling_p, max_length, seed, forced ? 1 : 0);
    {
        Ctx dry = make_ctx(1, nullptr, 0, nullptr);
        slots_prefix(s, dry, slot, nullptr, text_len, nullptr, cont_len, row, nullptr);
        if (dry.off > workspace_bytes) return fail("workspace too small");
    }
    slot_restart(s, slot, text_len, cont_len, max_length, forced ? 1 : 0);
    s->last = (hipStream_t)stream;
    Ctx cx = make_ctx(1, workspace, workspace_bytes, stream);
    if (slots_prefix(s, cx, slot, text_outs, text_len, cont_len ? continual : nullptr, cont_len, row, forced)) return 1;
    s->slot[slot].state = SLOT_RUNNING;
    return 0;
}

int fc_laura_slots_start_from(fc_laura_slots* s, int dst, int src, int max_length, int sampling_mode, int sampling_k, float sampling_p,
                              uint64_t seed, const int64_t* forced, void* stream) {
    if (!s) return fail("null session");
    if (refuse_queued(s, "start_from")) return 1;
    if (check_ready(s->e)) return 1;
    if (dst < 0 || dst >= s->S) return fail(slot_who(dst) + " outside 0 .. " + std::to_string(s->S - 1));
    if (dst == src) return fail(slot_who(dst) + " cannot be started from itself");      // dst is in range: so is this src
    if (check_source(s, src, "decoding session: source slot " + std::to_string(src))) return 1;
    if (max_length < 1) return fail("decoding session: bad argument for slot " + std::to_string(dst));
    if (check_sampling(sampling_mode, sampling_k, sampling_p) || check_rules_mode(s->slot[dst].rules, sampling_mode, slot_who(dst) + ": ")) return 1;
    if (check_fits(slot_who(dst) + ": ", s->slot[src].prefix, max_length, s->R)) return 1;
    return slots_from_prefix(s, dst, s, src, max_length, sampling_mode, sampling_k, sampling_p, seed, forced, stream);
}

size_t fc_laura_slots_start_many_workspace_bytes(const fc_laura_slots* cs, int n, int L, int Cmax) {
    fc_laura_slots* s = const_cast<fc_laura_slots*>(cs);
    if (!s || n < 1 || n > 16 || n > s->S || L < 1 || Cmax < 0) return 0;
    Ctx cx = make_ctx(n, nullptr, 0, nullptr);
    lk::RowSlots rs;
    rs.n = n;
    slots_prefix_many(s, cx, rs, nullptr, nullptr, L, nullptr, nullptr, Cmax, nullptr, L + 2 + Cmax);
    return cx.off + 4096;
}

int fc_laura_slots_start_many(fc_laura_slots* s, int n, const int32_t* slots, const float* text_outs, const int32_t* text_lens, int L,
                              const int64_t* continual, const int32_t* cont_lens, int Cmax, const int32_t* max_lengths,
                              const int32_t* sampling_modes, const int32_t* sampling_ks, const float* sampling_ps, const uint64_t* seeds,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!s) return fail("null session");
    if (refuse_queued(s, "start_many")) return 1;
    if (check_ready(s->e)) return 1;
    if (!slots || !text_outs || !text_lens || !max_lengths || !sampling_modes || !sampling_ks || !sampling_ps || !seeds || !workspace ||
        n < 1 || L < 1 || Cmax < 0 || (continual && !cont_lens))
        return fail("decoding session: start_many: bad argument");
    // every rule for every row before the first launch: a refused call changes nothing for any slot
    const int nmax = std::min(16, s->S);
    if (n > nmax)
        return fail("decoding session: slot " + std::to_string(slots[nmax]) + ": start_many takes at most min(16, slots) = " +
                    std::to_string(nmax) + " prompts per call, got " + std::to_string(n));
    lk::RowSlots rs;
    rs.n = n;
    lk::SampleRow rows[16];
    int Tmax = 0;
    for (int b = 0; b < n; ++b) {
        const int slot = slots[b];
        const std::string who = slot_who(slot);
        if (slot < 0 || slot >= s->S) return fail(who + " outside 0 .. " + std::to_string(s->S - 1));
        for (int j = 0; j < b; ++j)
            if (slots[j] == slot) return fail(who + " is named twice in one start_many");
        const int cont_len = continual ? cont_lens[b] : 0;
        if (text_lens[b] < 1 || text_lens[b] > L || max_lengths[b] < 1 || cont_len < 0 || cont_len > Cmax)
            return fail("decoding session: bad argument for slot " + std::to_string(slot));
        if (const char* why = sampling_problem(sampling_modes[b], sampling_ks[b], sampling_ps[b])) return fail(who + ": " + why);
        if (check_rules_mode(s->slot[slot].rules, sampling_modes[b], who + ": ")) return 1;
        const int P = text_lens[b] + 2 + cont_len;
        if (check_fits(who + ": ", P, max_lengths[b], s->R)) return 1;
        Tmax = std::max(Tmax, P);
        rs.slot[b] = slot;
        rows[b] = make_row(s->slot[slot].rules, sampling_modes[b], sampling_ks[b], sampling_ps[b], max_lengths[b], seeds[b], 0);
    }
    {
        Ctx dry = make_ctx(n, nullptr, 0, nullptr);
        slots_prefix_many(s, dry, rs, nullptr, nullptr, L, nullptr, nullptr, Cmax, nullptr, Tmax);
        if (dry.off > workspace_bytes) return fail("workspace too small");
    }
    for (int b = 0; b < n; ++b) slot_restart(s, slots[b], text_lens[b], continual ? cont_lens[b] : 0, max_lengths[b], 0);
    s->last = (hipStream_t)stream;
    Ctx cx = make_ctx(n, workspace, workspace_bytes, stream);
    if (slots_prefix_many(s, cx, rs, text_outs, text_lens, L, continual, cont_lens, Cmax, rows, Tmax)) return 1;
    for (int b = 0; b < n; ++b) s->slot[slots[b]].state = SLOT_RUNNING;
    return 0;
}

int fc_laura_slots_start_from_session(fc_laura_slots* s, int dst, const fc_laura_slots* from, int src, int max_length, int sampling_mode,
                                      int sampling_k, float sampling_p, uint64_t seed, const int64_t* forced, void* stream) {
    if (!s || !from) return fail("null session");
    if (refuse_queued(s, "start_from_session")) return 1;
    if (check_ready(s->e)) return 1;
    if (dst < 0 || dst >= s->S) return fail(slot_who(dst) + " outside 0 .. " + std::to_string(s->S - 1));
    if (from->e != s->e)
        return fail(slot_who(dst) + ": the source session belongs to another engine (other weights: its prefix is not this engine's)");
    if (from == s) return fail(slot_who(dst) + ": the source session is this session (fc_laura_slots_start_from copies inside one)");
    if (check_source(from, src, "decoding session: source slot " + std::to_string(src), " of the source session")) return 1;
    if (max_length < 1) return fail("decoding session: bad argument for slot " + std::to_string(dst));
    if (check_sampling(sampling_mode, sampling_k, sampling_p) || check_rules_mode(s->slot[dst].rules, sampling_mode, slot_who(dst) + ": ")) return 1;
    if (check_fits(slot_who(dst) + ": ", from->slot[src].prefix, max_length, s->R)) return 1;
    return slots_from_prefix(s, dst, from, src, max_length, sampling_mode, sampling_k, sampling_p, seed, forced, stream);
}

int fc_laura_slots_fork(fc_laura_slots* s, int dst, int src, int keep, int max_length, int sampling_mode, int sampling_k, float sampling_p,
                        uint64_t seed, void* stream) {
    if (!s) return fail("null session");
    if (refuse_queued(s, "fork")) return 1;
    if (check_ready(s->e)) return 1;
    const std::string who = slot_who(dst) + ": ";
    if (dst < 0 || dst >= s->S) return fail(slot_who(dst) + " outside 0 .. " + std::to_string(s->S - 1));
    if (check_source(s, src, "decoding session: source slot " + std::to_string(src))) return 1;
    const Slot& held = s->slot[src];
    const int g = held.n_gen;
    if (keep < 0) keep = g;
    if (keep > g)
        return fail(who + "keep " + std::to_string(keep) + " outside 0 .. " + std::to_string(g) + ", the tokens source slot " +
                    std::to_string(src) + " has generated as last reported");
    if (max_length < 1) max_length = held.max_len;
    if (max_length <= keep)
        return fail(who + "max_length " + std::to_string(max_length) + " leaves nothing to generate after keep " + std::to_string(keep));
    if (check_sampling(sampling_mode, sampling_k, sampling_p) || check_rules_mode(s->slot[dst].rules, sampling_mode, who)) return 1;
    const int P = held.prefix, cont_len = held.cont_len;
    if (check_fits(who, P, max_length, s->R)) return 1;
    if (keep == 0) return slots_from_prefix(s, dst, s, src, max_length, sampling_mode, sampling_k, sampling_p, seed, nullptr, stream);
    const int forced_on = held.forced_on, forced_rows = held.max_len;
    if (forced_on && max_length > forced_rows)
        return fail(who + "source slot " + std::to_string(src) + " follows " + std::to_string(forced_rows) + " forced tokens, max_length " +
                    std::to_string(max_length) + " goes past them");
    const StepMem& m = s->m;
    // in place the slot's own utterance is kept up to token `keep`
    slot_restart(s, dst, held.text_len, cont_len, max_length, forced_on, keep);
    Ctx cx = make_ctx(1, (void*)m.pos, 0, stream);          // launches only: nothing is allocated
    s->last = cx.st;
    // positions [0, P + keep - 1): the prefix and kept tokens 0 .. keep - 2; token keep - 1 is the next step's input.  Sets pos[dst].
    if (dst != src) prefix_import(s, cx, dst, s, src, P + keep - 1, "cache copy");
    const lk::Sample sm = slots_sampler(s);
    lk::SlotBranch r;
    r.S = s->S; r.dst = dst; r.src = src; r.keep = keep; r.P = P;
    r.n_gen = m.n_gen(); r.done = m.done(); r.step = m.step(); r.pos = m.pos; r.tok_off = s->tok_off; r.rows = s->rows;
    r.row = make_row(s->slot[dst].rules, sampling_mode, sampling_k, sampling_p, max_length, seed, forced_on);
    r.tokens = s->tokens; r.tok_stride = s->R; r.nq = s->e->arch.predict_nq; r.cont_len = cont_len; r.forced = s->forced;
    r.forced_rows = forced_rows; r.logp = s->logp; r.V = s->e->vocab(); r.score = s->score;
    r.cb = sm.cb; r.K = sm.K; r.D = sm.D; r.next_emb = sm.next_emb; r.emb_wt = sm.emb_wt; r.emb_bias = sm.emb_bias; r.emb_g = sm.emb_g;
    r.emb_b = sm.emb_b; r.dm = sm.dm; r.emb_relu = sm.emb_relu; r.xscale = sm.xscale; r.xs = sm.xs;
    cx.check(lk::launch_slot_branch(r, cx.st), "slot branch");
    if (cx.err) return 1;
    s->slot[dst].state = SLOT_RUNNING;
    return 0;
}

int fc_laura_slots_set_rules(fc_laura_slots* s, int slot, float temperature, int min_length, float top_p, int repeat_window, int repeat_count) {
    if (!s) return fail("null session");
    if (slot < 0 || slot >= s->S) return fail("decoding session: slot " + std::to_string(slot) + " outside 0 .. " + std::to_string(s->S - 1));
    const std::string why = rules_problem(temperature, min_length, top_p, repeat_window, repeat_count);
    if (!why.empty()) return fail(slot_who(slot) + ": " + why);
    s->slot[slot].rules = rules_row(temperature, min_length, top_p, repeat_window, repeat_count);
    return 0;
}

int fc_laura_slots_set_elastic(fc_laura_slots* s, int on) {
    if (!s) return fail("null session");
    if (s->Q) return fail("decoding session: set_elastic: a queued session claims its slots on the device, the host cannot know the busy rows");
    s->elastic = on != 0;
    return 0;
}

int fc_laura_slots_step_blocks(const fc_laura_slots* s) { return s ? s->last_blocks : 0; }

int fc_laura_slots_move(fc_laura_slots* s, int n, const int32_t* src, const int32_t* dst, void* stream) {
    if (!s) return fail("null session");
    if (refuse_queued(s, "move")) return 1;
    if (check_ready(s->e)) return 1;
    const int S = s->S;
    if (n < 1 || n > S) return fail("decoding session: move: 1 .. " + std::to_string(S) + " moves per call, got " + std::to_string(n));
    if (!src || !dst) return fail("null argument");
    // every rule for every line before the first launch: a refused call changes nothing for any slot
    lk::SlotMoveLines lines;
    lines.n = n;
    unsigned long long srcs = 0, dsts = 0;
    for (int i = 0; i < n; ++i) {
        const int a = src[i], b = dst[i];
        const std::string range = " outside 0 .. " + std::to_string(S - 1);
        if (a < 0 || a >= S) return fail("decoding session: move: source slot " + std::to_string(a) + range);
        if (b < 0 || b >= S) return fail("decoding session: move: slot " + std::to_string(b) + range);
        if ((srcs | dsts) >> a & 1ull)
            return fail("decoding session: move: source slot " + std::to_string(a) + (srcs >> a & 1ull ? " is named twice" : " is also a destination"));
        if (((srcs | dsts) >> b & 1ull) || a == b)
            return fail("decoding session: move: slot " + std::to_string(b) + (dsts >> b & 1ull ? " is named twice" : " is also a source"));
        if (check_source(s, a, "decoding session: move: source slot " + std::to_string(a))) return 1;      // in range: whether it holds one
        srcs |= 1ull << a; dsts |= 1ull << b;
        lines.src[i] = a; lines.dst[i] = b;
    }
    for (int i = 0; i < n; ++i) {
        const int st = s->slot[dst[i]].state;
        if (st != SLOT_FREE)
            return fail("decoding session: move: slot " + std::to_string(dst[i]) + " is not free (" +
                        (st == SLOT_RUNNING ? "running" : st == SLOT_DONE ? "ended, not taken" : "failed") + ")");
    }
    fc_laura* e = s->e;
    const StepMem& m = s->m;
    lk::SlotMoves mv;
    mv.table = s->move_table; mv.kc = m.kc; mv.vc = m.vc; mv.n_gen = m.n_gen(); mv.done = m.done(); mv.step = m.step(); mv.pos = m.pos;
    mv.tok_off = s->tok_off; mv.rows = s->rows; mv.tokens = s->tokens; mv.forced = s->forced; mv.logp = s->logp; mv.score = s->score;
    mv.lg = m.lg; mv.lg0 = s->lg0; mv.xs = m.xs; mv.nemb = m.nemb;
    mv.NL = e->codec_lm.s.layers; mv.S = S; mv.d = e->codec_lm.s.d_model; mv.Tcap = m.Tcap; mv.V = e->vocab(); mv.R = s->R;
    mv.nq = e->arch.predict_nq; mv.D = e->arch.codebook_dim;
    Ctx cx = make_ctx(1, (void*)m.pos, 0, stream);          // launches only: nothing is allocated
    s->last = cx.st;
    // from here on a failure leaves the named slots failed, as a start that fails half-way
    cx.check(lk::launch_slot_moves(mv, lines, cx.st), "slot move");
    if (cx.err) {
        for (int i = 0; i < n; ++i) s->slot[src[i]].state = SLOT_FAILED;
        return 1;
    }
    // the host mirror of every moved slot; the rules of the two rows change places
    for (int i = 0; i < n; ++i) {
        Slot &a = s->slot[src[i]], &b = s->slot[dst[i]];
        const lk::SampleRow rules_b = b.rules;
        b = a;
        a.rules = rules_b;
        a.state = SLOT_FREE; a.n_gen = 0;
    }
    return 0;
}

int fc_laura_slots_step(fc_laura_slots* s, int n_steps, int32_t* done_out, int32_t* n_gen_out, void* stream) {
    if (!s) return fail("null session");
    if (check_ready(s->e)) return 1;
    if (n_steps < 1) return fail("decoding session: n_steps must be >= 1");
    bool any = false;
    for (const Slot& x : s->slot) any = any || x.state == SLOT_RUNNING;
    if (s->Q) any = s->submitted > s->finished + s->failed;             // a ticket waits or runs
    s->last_blocks = 0;
    if (!any) { slots_report(s, done_out, n_gen_out); return 0; }
    // an elastic session: the width of this call, from the host mirror of the slot states.  No slot can start inside the call, so the
    // width holds for all n_steps.  cut > 0: the first `cut` rows only (whole column blocks, fewer than S; the kernel chain -- S > 16)
    int cut = 0;
    s->last_blocks = (s->S + 15) / 16;
    if (s->elastic && s->S > 16) {
        int hi = 0;
        for (int i = 0; i < s->S; ++i)
            if (s->slot[i].state == SLOT_RUNNING) hi = i;
        const int rows = std::min(s->S, 16 * (hi / 16 + 1));
        s->last_blocks = (rows + 15) / 16;
        if (rows < s->S) cut = rows;
    }
    hipGraphExec_t& gx = cut ? s->gexec_cut[cut / 16 - 1] : s->gexec;
    const lk::QueuePhase* qp = s->Q ? &s->qp : nullptr;
    fc_laura* e = s->e;
    const StepMem& m = s->m;
    Ctx cx = make_ctx(s->S, (void*)m.pos, 0, stream);       // launches only: nothing is allocated
    s->last = cx.st;
    const bool persist = !s->chain_only && step_persist_ok(e, m);
    const lk::StepPersistArgs pa = step_persist_args(e, m, nullptr);
    lk::Sample sm = slots_sampler(s);
    if (!persist) sm.launch_seq = nullptr;                  // the launch number counts persistent launches only: the forms may alternate
    const lk::StepPersistArgs* pap = persist ? &pa : nullptr;
    // the arrival counters grow by a fixed amount per launch: back to zero long before 32 bits are used up
    if (persist && s->persist_steps + (unsigned long long)n_steps > (1ull << 20)) slots_reset_sync(s, cx);
    if (s->gexec && (s->g_persist != persist || s->g_timeout != (pa.test_timeout != 0))) {
        (void)hipGraphExecDestroy(s->gexec);
        s->gexec = nullptr;
    }
    for (int i = 0; i < n_steps && !cx.err; ++i) {
        if (!s->warmed[persist]) {                          // the form's first step runs eagerly
            run_step(e, cx, m, pap, sm, cx.st, qp, cut);
            s->warmed[persist] = true;
            continue;
        }
        if (!gx && graph_enabled() && cx.st != nullptr) {
            gx = capture_step(e, cx, m, pap, sm, cx.st, qp, cut);
            if (!cut) { s->g_persist = persist; s->g_timeout = pa.test_timeout != 0; }
            if (cx.err) break;
        }
        if (gx) cx.check(hipGraphLaunch(gx, cx.st), "graph launch");
        else run_step(e, cx, m, pap, sm, cx.st, qp, cut);
    }
    if (persist) s->persist_steps += (unsigned long long)n_steps;
    // a queued session retires what the last step ended before the read-back, so a finished ticket never waits for another call
    if (qp && !cx.err) cx.check(lk::launch_queue_phase(*qp, 0, cx.st), "queue phase");
    // one stream-ordered read-back: n_gen [S], done [S] (adjacent) and the persistent step's error word; of a queued session the queue
    // block as well (counters, the ticket of every slot, the result entries' words), ahead of the same one synchronisation
    int* host = s->status;
    host[2 * s->S] = 0;
    hipError_t ea = cx.err ? hipErrorUnknown : hipMemcpyAsync(host, m.ctr, (size_t)2 * s->S * sizeof(int), hipMemcpyDeviceToHost, cx.st);
    if (ea == hipSuccess && persist) ea = hipMemcpyAsync(host + 2 * s->S, m.error_word(), sizeof(unsigned), hipMemcpyDeviceToHost, cx.st);
    if (ea == hipSuccess && qp)
        ea = hipMemcpyAsync(host + 2 * s->S + 1, qp->qw, (size_t)s->queue_words() * sizeof(int), hipMemcpyDeviceToHost, cx.st);
    if (ea == hipSuccess) ea = hipStreamSynchronize(cx.st);
    if (qp) return queue_after_step(s, cx, ea, done_out, n_gen_out);
    const unsigned perr = (unsigned)host[2 * s->S];
    if (ea != hipSuccess) {
        for (Slot& x : s->slot)
            if (x.state == SLOT_RUNNING) x.state = SLOT_FAILED;
        if (!cx.err) fail(std::string("decoding session: status read-back failed: ") + hipGetErrorString(ea));
        return 1;
    }
    if (perr) {
        // A hand-off of the persistent step timed out.  The residual rows are updated in place, so the step cannot be run again: every slot
        // that was running is failed (start revives it).
        for (Slot& x : s->slot)
            if (x.state == SLOT_RUNNING) x.state = SLOT_FAILED;
        if (after_timeout(s, cx)) return 1;
    } else {
        for (int i = 0; i < s->S; ++i) {
            if (s->slot[i].state != SLOT_RUNNING) continue;
            s->slot[i].n_gen = host[i];
            if (host[s->S + i]) s->slot[i].state = SLOT_DONE;
        }
    }
    slots_report(s, done_out, n_gen_out);
    return 0;
}

int fc_laura_slots_take(fc_laura_slots* s, int slot, int64_t* tokens, int cap, int32_t* len_out, float* logp_out) {
    if (!s) return fail("null session");
    if (refuse_queued(s, "take")) return 1;
    if (check_ready(s->e)) return 1;
    if (slot < 0 || slot >= s->S) return fail("decoding session: slot " + std::to_string(slot) + " outside 0 .. " + std::to_string(s->S - 1));
    if (s->slot[slot].state == SLOT_FAILED) return fail("decoding session: slot " + std::to_string(slot) + " failed (a hand-off of the persistent step timed out); start it again");
    if (s->slot[slot].state != SLOT_DONE) return fail("decoding session: slot " + std::to_string(slot) + " has not ended");
    if (!tokens || !len_out) return fail("null argument");
    const int nq = s->e->arch.predict_nq, V = s->e->vocab();
    const int n = s->slot[slot].cont_len + s->slot[slot].n_gen;
    if (cap < n) return fail("decoding session: slot " + std::to_string(slot) + " holds " + std::to_string(n) + " tokens, room for " + std::to_string(cap));
    if (logp_out && !s->logp) return fail("decoding session: opened without per-step log-probabilities");
    if (n > 0) HIP_TRY(hipMemcpyAsync(tokens, s->tokens + (size_t)slot * s->R * nq, (size_t)n * nq * sizeof(int64_t), hipMemcpyDeviceToDevice, s->last));
    if (logp_out)
        HIP_TRY(hipMemcpyAsync(logp_out, s->logp + (size_t)slot * s->R * V, (size_t)s->slot[slot].max_len * V * sizeof(float), hipMemcpyDeviceToDevice, s->last));
    HIP_TRY(hipStreamSynchronize(s->last));
    *len_out = n;
    s->slot[slot].state = SLOT_FREE;
    return 0;
}

int fc_laura_slots_score(fc_laura_slots* s, int slot, float* terms, int cap, int32_t* count_out, int32_t* end_out) {
    if (!s) return fail("null session");
    if (refuse_queued(s, "score")) return 1;
    if (check_ready(s->e)) return 1;
    if (slot < 0 || slot >= s->S) return fail("decoding session: slot " + std::to_string(slot) + " outside 0 .. " + std::to_string(s->S - 1));
    if (!s->score) return fail("decoding session: slot " + std::to_string(slot) + ": the session was opened without scores");
    const Slot& x = s->slot[slot];
    if (x.state == SLOT_FAILED) return fail("decoding session: slot " + std::to_string(slot) + " failed (a hand-off of the persistent step timed out); start it again");
    if (!x.holds()) return fail("decoding session: slot " + std::to_string(slot) + " holds no utterance");
    if (!terms || !count_out || !end_out) return fail("null argument");
    if (cap < s->R) return fail("decoding session: slot " + std::to_string(slot) + ": a score row has " + std::to_string(s->R) + " terms, room for " + std::to_string(cap));
    HIP_TRY(hipMemcpyAsync(terms, s->score + (size_t)slot * s->R, (size_t)s->R * sizeof(float), hipMemcpyDeviceToHost, s->last));
    HIP_TRY(hipStreamSynchronize(s->last));
    // a slot that ended below its max_length ended on <eos>: that step ran and has a term, but no token
    const bool ended = x.state == SLOT_DONE, eos = ended && x.n_gen < x.max_len;
    *count_out = x.n_gen + (eos ? 1 : 0);
    *end_out = eos ? 2 : (ended ? 1 : 0);
    return 0;
}

int fc_laura_slots_submit(fc_laura_slots* s, int row, int max_length, int sampling_mode, int sampling_k, float sampling_p, uint64_t seed,
                          float temperature, int min_length, float top_p, int repeat_window, int repeat_count, int32_t* ticket_out,
                          void* stream) {
    if (!s) return fail("null session");
    if (check_ready(s->e)) return 1;
    if (!s->Q) return fail("decoding session: submit: the session was created without a queue (fc_laura_slots_create_queued)");
    if (!ticket_out) return fail("null argument");
    const fc_laura_slots* from = s->from;
    const long long ticket = s->submitted;
    const std::string who = "decoding session: ticket " + std::to_string(ticket) + " (row " + std::to_string(row) + "): ";
    if (ticket >= 0x7fffffff) return fail(who + "the session has run out of ticket numbers");
    if (check_source(from, row, who + "row", " of the source session", who + "the row of the source session", " holds no prompt (")) return 1;
    if (max_length < 1) return fail(who + "max_length must be >= 1");
    if (const char* why = sampling_problem(sampling_mode, sampling_k, sampling_p)) return fail(who + why);
    // the rules, as fc_laura_slots_set_rules and the start that follows it check them
    const std::string why = rules_problem(temperature, min_length, top_p, repeat_window, repeat_count);
    if (!why.empty()) return fail(who + why);
    const lk::SampleRow rules = rules_row(temperature, min_length, top_p, repeat_window, repeat_count);
    if (check_rules_mode(rules, sampling_mode, who)) return 1;
    const int P = from->slot[row].prefix, cont_len = from->slot[row].cont_len;
    if (check_fits(who, P, max_length, s->R)) return 1;
    if (s->submitted - s->collected >= s->Q)
        return fail(who + "all " + std::to_string(s->Q) + " result entries are in flight or uncollected (fc_laura_slots_collect frees them)");
    int entry = -1;
    for (int i = 0; i < s->Q && entry < 0; ++i)
        if (s->entries[i].state == 0) entry = i;
    if (entry < 0) return fail(who + "no free result entry");
    lk::QueueTicket t;
    t.row = row; t.P = P; t.cont_len = cont_len; t.entry = entry;
    t.srow = make_row(rules, sampling_mode, sampling_k, sampling_p, max_length, seed, 0);
    s->last = (hipStream_t)stream;
    const hipError_t el = lk::launch_queue_put(s->qp, t, (int)ticket, s->last);
    if (el != hipSuccess) return fail(who + "queue put: " + hipGetErrorString(el));
    fc_laura_slots::Entry& E = s->entries[entry];
    E = fc_laura_slots::Entry{};
    E.state = 1; E.ticket = (int)ticket;
    s->submitted++;
    *ticket_out = (int32_t)ticket;
    return 0;
}

int fc_laura_slots_queue_status(const fc_laura_slots* s, int64_t* submitted, int64_t* claimed, int64_t* finished, int64_t* failed,
                                int64_t* collected, int32_t* slot_tickets) {
    if (!s) return fail("null session");
    if (!s->Q) return fail("decoding session: queue_status: the session was created without a queue (fc_laura_slots_create_queued)");
    if (submitted) *submitted = s->submitted;
    if (claimed) *claimed = s->claimed;
    if (finished) *finished = s->finished;
    if (failed) *failed = s->failed;
    if (collected) *collected = s->collected;
    if (slot_tickets)
        for (int i = 0; i < s->S; ++i) slot_tickets[i] = s->slot_ticket[i];
    return 0;
}

int fc_laura_slots_collect(fc_laura_slots* s, int cap, int32_t* tickets, int32_t* states, int32_t* lens, int32_t* n_gens, int32_t* ends,
                           int64_t* tokens, float* scores, int32_t* n_out) {
    if (!s) return fail("null session");
    if (check_ready(s->e)) return 1;
    if (!s->Q) return fail("decoding session: collect: the session was created without a queue (fc_laura_slots_create_queued)");
    if (cap < 0 || !n_out || (cap > 0 && (!tickets || !states || !lens || !n_gens || !ends || !tokens))) return fail("null argument");
    if (scores && !s->score) return fail("decoding session: collect: the session was created without scores");
    // failed tickets first (in ticket order), then the finished ones in the order they finished
    std::vector<int> order;
    for (int i = 0; i < s->Q; ++i)
        if (s->entries[i].state == 2 || s->entries[i].state == 3) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        const fc_laura_slots::Entry &A = s->entries[a], &B = s->entries[b];
        if (A.state != B.state) return A.state > B.state;
        return A.state == 3 ? A.ticket < B.ticket : A.seq < B.seq;
    });
    if ((int)order.size() > cap) order.resize(cap);
    const int nq = s->e->arch.predict_nq;
    const size_t tok_row = (size_t)s->R * nq;
    for (size_t j = 0; j < order.size(); ++j) {
        const fc_laura_slots::Entry& E = s->entries[order[j]];
        tickets[j] = E.ticket; states[j] = E.state;
        lens[j] = E.state == 2 ? E.n_tok : 0; n_gens[j] = E.state == 2 ? E.n_gen : 0; ends[j] = E.state == 2 ? (E.eos ? 2 : 1) : 0;
        if (E.state != 2) continue;         // a failed ticket has no tokens
        if (E.n_tok > 0)
            HIP_TRY(hipMemcpyAsync(tokens + j * tok_row, s->qp.ring_tokens + (size_t)order[j] * tok_row, (size_t)E.n_tok * nq * sizeof(int64_t),
                                   hipMemcpyDeviceToDevice, s->last));
        if (scores)
            HIP_TRY(hipMemcpyAsync(scores + j * s->R, s->qp.ring_score + (size_t)order[j] * s->R, (size_t)s->R * sizeof(float),
                                   hipMemcpyDeviceToHost, s->last));
    }
    if (!order.empty()) HIP_TRY(hipStreamSynchronize(s->last));       // one synchronisation for all of them
    for (int en : order) s->entries[en] = fc_laura_slots::Entry{};
    s->collected += (long long)order.size();
    *n_out = (int32_t)order.size();
    return 0;
}

int fc_laura_codec_emb(fc_laura* e, const float* text_outs, const int32_t* text_lens, int B, int L, const int64_t* codec, int nq_cols,
                       const int32_t* codec_lens, int Cmax, float* emb, void* workspace, size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!text_outs || !text_lens || !codec || !codec_lens || !emb || !workspace || B < 1 || L < 1 || Cmax < 1) return fail("bad argument");
    if (nq_cols < e->arch.predict_nq) return fail("codec has fewer columns than predict_nq");
    if (check_lens(text_lens, B, 1, L, "text_lens") || check_lens(codec_lens, B, 0, Cmax, "codec_lens")) return 1;
    int Tmax = 0;
    for (int b = 0; b < B; ++b) Tmax = std::max(Tmax, text_lens[b] + codec_lens[b]);
    if (Tmax > e->R) return fail("sequence longer than max_positions");
    Ctx cx = make_ctx(B, workspace, workspace_bytes, stream);
    return do_codec_emb(e, cx, text_outs, text_lens, L, codec, nq_cols, codec_lens, Cmax, emb, Tmax);
}

int fc_laura_set_persistent_step(fc_laura* e, int on) {
    if (!e) return -1;
    e->persist_on = on != 0;
    if (!e->persist_on || e->persist_grid <= 0) return 0;
    // usable for this model at SOME batch size: B = 1 is the smallest LDS footprint (do_decode re-checks every call at its own B, NS)
    const fc_laura_stack& s = e->codec_lm.s;
    const int NS = std::min(8, 256 / s.heads);
    return lk::step_persist_supported(1, s.d_model, s.ff, s.heads, s.d_model / s.heads, e->vocab(), std::max(1, NS)) ? 1 : 0;
}

int fc_laura_debug_probe(void* dev_dst, size_t cap_bytes, int stack, int layer, int what) {
    g_probe.dst = (float*)dev_dst; g_probe.cap = cap_bytes; g_probe.stack = stack; g_probe.layer = layer; g_probe.what = what;
    return 0;
}

int fc_laura_linear(fc_laura* e, const char* name, const float* x, int B, int T, int step_form, float* y, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!name || !x || !y || !workspace || B < 1 || T < 1) return fail("bad argument");
    auto it = e->lin_by_name.find(name);
    if (it == e->lin_by_name.end()) return fail(std::string("unknown Linear: ") + name);
    const Lin& L = *it->second;
    Ctx cx = make_ctx(B, workspace, workspace_bytes, stream);
    if (step_form) {
        if (!L.wf) return fail(std::string(name) + " has no decoding-step form");
        if (B * T > 64) return fail("step form: at most 64 rows");
        if (step_form < 1 || step_form > 3) return fail("step_form must be 0 .. 3");
        cx.check(step_gemv(L, x, B * T, nullptr, nullptr, 0.f, 0, 0, y, L.cout, cx.st, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, 0, 0,
                           step_form - 1), "GEMV");
        return cx.err;
    }
    const int Tp = pad4(T);
    float* in = cx.alloc<float>((size_t)B * L.cin * Tp);
    float* o = cx.alloc<float>((size_t)B * L.cout * Tp);
    if (!cx.live()) return 1;
    cx.check(lk::launch_tm_to_fm(x, nullptr, B, T, L.cin, Tp, in, cx.st), "transpose");
    cx.check(launch_lin_full(L, in, B, Tp, o, cx.st), "GEMM");
    cx.check(lk::launch_fm_to_tm(o, nullptr, B, L.cout, Tp, T, y, cx.st), "transpose");
    return cx.err;
}

int fc_laura_attention(fc_laura* e, int stack, int layer, const float* qkv, const int32_t* lens, const int32_t* bidir, int causal, int B,
                       int T, float* ctx, void* workspace, size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!qkv || !lens || !ctx || !workspace || B < 1 || T < 1) return fail("bad argument");
    if (stack < 0 || stack > 2) return fail("stack must be 0 (text_encoder), 1 (codec_lm) or 2 (codec_encoder)");
    const Stack& S = stack == 0 ? e->text_encoder : stack == 1 ? e->codec_lm : e->codec_encoder;
    if (layer < 0 || layer >= S.s.layers) return fail("no such block in " + S.prefix);
    if (T > e->R) return fail("sequence longer than max_positions");
    if (check_lens(lens, B, 1, T, "lens") || (bidir && check_lens(bidir, B, 0, T, "bidir"))) return 1;
    const int d = S.s.d_model, Tp = pad4(T);
    Ctx cx = make_ctx(B, workspace, workspace_bytes, stream);
    int* ld = upload_lens(cx, lens, B);
    int* bd = bidir ? upload_lens(cx, bidir, B) : nullptr;
    float* in = cx.alloc<float>((size_t)B * 3 * d * Tp);
    float* o = cx.alloc<float>((size_t)B * d * Tp);
    if (!cx.live()) return 1;
    // no length masking in the transposes: the caller decides every input value, and sees every output value
    cx.check(lk::launch_tm_to_fm(qkv, nullptr, B, T, 3 * d, Tp, in, cx.st), "transpose");
    cx.check(lk::launch_attn_full(attn_full_args(e, S, S.blocks[layer], in, ld, bd, causal ? 1 : 0, o, B, Tp), cx.st), "attention");
    cx.check(lk::launch_fm_to_tm(o, nullptr, B, d, Tp, T, ctx, cx.st), "transpose");
    return cx.err;
}

int fc_laura_step_block(fc_laura* e, int layer, float* x, float* k_cache, float* v_cache, const int32_t* pos, int B, int Tcap,
                        int key_ranges, int wide, float* q_out, float* part_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!x || !k_cache || !v_cache || !pos || !q_out || !part_out || !workspace) return fail("bad argument");
    const Stack& S = e->codec_lm;
    if (layer < 0 || layer >= S.s.layers) return fail("no such block in " + S.prefix);
    if (B < 1 || B > 64) return fail("a decoding step has 1 .. 64 rows");
    if (wide && B > 16) wide = 0;                 // beyond 16 rows the launches are over column blocks anyway
    if (Tcap < 4 || Tcap % 4) return fail("the cache capacity must be a multiple of 4");
    if (check_lens(pos, B, 0, std::min(Tcap, e->R) - 1, "pos")) return 1;
    const int d = S.s.d_model, heads = S.s.heads, dkh = d / heads;
    const int NS = key_ranges;
    if (NS < 1 || NS > 8) return fail("key_ranges must be 1 .. 8");
    Ctx cx = make_ctx(B, workspace, workspace_bytes, stream);
    const size_t RW = (size_t)step_rows(B);
    int* pd = upload_lens(cx, pos, B);
    StepBlockBufs m{};
    m.xs = cx.alloc<float>(RW * d);
    m.qb = cx.alloc<float>(RW * d);
    m.apart = cx.alloc<float>(RW * heads * 8 * (dkh + 2));
    m.hb = cx.alloc<float>(RW * S.s.ff);
    m.kc = k_cache; m.vc = v_cache; m.pos = pd; m.NS = NS;
    if (!cx.live()) return 1;
    cx.check(hipMemcpyAsync(m.xs, x, (size_t)B * d * sizeof(float), hipMemcpyDeviceToDevice, cx.st), "copy in");
    run_step_block(e, cx, S.blocks[layer], m, B, Tcap, wide ? 1 : 0, cx.st);
    cx.check(hipMemcpyAsync(x, m.xs, (size_t)B * d * sizeof(float), hipMemcpyDeviceToDevice, cx.st), "copy out");
    cx.check(hipMemcpyAsync(q_out, m.qb, (size_t)B * d * sizeof(float), hipMemcpyDeviceToDevice, cx.st), "copy out");
    cx.check(hipMemcpyAsync(part_out, m.apart, (size_t)B * heads * NS * (dkh + 2) * sizeof(float), hipMemcpyDeviceToDevice, cx.st), "copy out");
    return cx.err;
}

int fc_laura_sample(fc_laura* e, const fc_laura_sample_io* io, void* workspace, size_t workspace_bytes, void* stream) {
    if (check_ready(e)) return 1;
    if (!io || !workspace) return fail("bad argument");
    if (!io->logits || !io->step || !io->n_gen || !io->done || !io->pos || !io->tok_off || !io->n_done || !io->tokens || !io->next_emb || !io->xs)
        return fail("sample: null buffer");
    const int B = io->B, R = io->R, K = e->arch.codebook_size, nq = e->arch.predict_nq;
    if (B < 1 || B > 64) return fail("sample: 1 .. 64 rows");
    if (R < 1) return fail("sample: token rows of at least one step");
    const int n = io->nrows > 0 ? io->nrows : B;
    if (io->row0 < 0 || io->nrows < 0 || io->row0 + n > B) return fail("sample: row0 / nrows outside the " + std::to_string(B) + " rows");
    // steps per row of forced / logp / score: the table form's row stride is the token rows' (a session), the call form's is max_steps
    const int steps = io->rows ? R : io->max_steps;
    std::vector<lk::SampleRow> table(B);
    for (int b = 0; b < B; ++b) {
        const std::string who = "sample: row " + std::to_string(b) + ": ";
        lk::SampleRow row;
        if (io->rows) {
            const fc_laura_sample_row& r = io->rows[b];
            const std::string why = rules_problem(r.temperature, r.min_length, r.top_p, r.repeat_window, r.repeat_count);
            if (!why.empty()) return fail(who + why);
            row = make_row(rules_row(r.temperature, r.min_length, r.top_p, r.repeat_window, r.repeat_count), r.mode, r.k, r.p, r.max_steps,
                           r.seed, r.forced_on ? 1 : 0);
            row.rng_row = r.rng_row;
        } else row = make_row(lk::SampleRow{}, io->mode, io->k, io->p, io->max_steps, io->seed, 1);
        if (row.mode < 0 || row.mode > 3) return fail(who + "sampling mode must be 0 .. 3");
        if (row.ki < 0 || !std::isfinite(row.pf)) return fail(who + "bad sampling k / p");
        if (row.max_steps < 1 || row.max_steps > steps) return fail(who + "max_steps outside 1 .. " + std::to_string(steps));
        if (io->step[b] < 0 || io->pos[b] < 0 || io->n_gen[b] < 0 || io->tok_off[b] < 0) return fail(who + "negative state");
        // every token row the kernel can touch lies in the row's R: the write at tok_off + n_gen of a running row, the repeat rule's window behind it
        if (io->tok_off[b] + io->n_gen[b] > R || io->tok_off[b] + row.max_steps > R)
            return fail(who + "tok_off + n_gen and tok_off + max_steps must not exceed the " + std::to_string(R) + " token rows");
        table[b] = row;
    }
    if (io->forced) {       // a forced id indexes the codebook table
        std::vector<int64_t> f((size_t)B * steps * nq);
        if (hipMemcpy(f.data(), io->forced, f.size() * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return fail("sample: forced read-back failed");
        for (int64_t v : f)
            if (v < 0 || v > K) return fail("sample: forced id outside 0 .. " + std::to_string(K));
    }
    Ctx cx = make_ctx(B, workspace, workspace_bytes, stream);
    int* st_d = upload_lens(cx, io->step, B);
    int* ng_d = upload_lens(cx, io->n_gen, B);
    int* dn_d = upload_lens(cx, io->done, B);
    int* ps_d = upload_lens(cx, io->pos, B);
    int* to_d = upload_lens(cx, io->tok_off, B);
    int* nd_d = upload_lens(cx, io->n_done, 1);
    lk::SampleRow* rows_d = cx.alloc<lk::SampleRow>(B);
    if (!cx.live()) return 1;
    lk::Sample sm = model_sampler(e);
    sm.logits = io->logits; sm.B = B;
    sm.step = st_d; sm.n_gen = ng_d; sm.done = dn_d; sm.pos = ps_d; sm.tok_off = to_d; sm.n_done = nd_d;
    sm.tokens = io->tokens; sm.tok_stride = R; sm.forced = io->forced; sm.logp_out = io->logp; sm.score_out = io->score;
    sm.next_emb = io->next_emb; sm.xs = io->xs;
    sm.row0 = io->row0; sm.nrows = io->nrows;
    if (io->rows) {
        cx.check(hipMemcpyAsync(rows_d, table.data(), (size_t)B * sizeof(lk::SampleRow), hipMemcpyHostToDevice, cx.st), "sampling table");
        sm.rows = rows_d; sm.row_stride = R;
    } else { sm.mode = io->mode; sm.ki = io->k; sm.pf = io->p; sm.seed = io->seed; sm.max_steps = io->max_steps; }
    if (cx.err) return 1;
    cx.check(lk::launch_sample(sm, cx.st), "sampling");
    cx.check(hipMemcpyAsync(io->step, st_d, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, cx.st), "state read-back");
    cx.check(hipMemcpyAsync(io->n_gen, ng_d, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, cx.st), "state read-back");
    cx.check(hipMemcpyAsync(io->done, dn_d, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, cx.st), "state read-back");
    cx.check(hipMemcpyAsync(io->pos, ps_d, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, cx.st), "state read-back");
    cx.check(hipMemcpyAsync(io->n_done, nd_d, sizeof(int), hipMemcpyDeviceToHost, cx.st), "state read-back");
    cx.check(hipStreamSynchronize(cx.st), "sampling");      // the host arrays hold the state, `table` may go
    return cx.err;
}

}  // extern "C"
