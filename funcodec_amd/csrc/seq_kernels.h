// Launch interface of the SEANet transformer bottleneck's attention kernel (seq_kernels.hip).
//
// seq_model: transformer (funcodec/modules/normed_modules/transformer.py:26-208) is a plain pre-LayerNorm transformer encoder over
// the bottleneck frames: no positional encoding, no length mask, optionally causal.  Its Linears run on the implicit-GEMM conv kernel
// and its LayerNorms on the LauraTTS feature-major LayerNorm (engine.hip run_transformer); this kernel is the attention.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace fc
