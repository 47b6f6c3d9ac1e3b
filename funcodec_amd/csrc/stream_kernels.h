// Launch interface of the streaming session's staging pass (stream_kernels.hip), used by engine.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace fc {

// The materialised input of one causal conv of a streaming push, the streaming sibling of launch_combine / launch_combine_xq:
//   buf[b][c][p], p in [0, pt + Tc + padR):
//     p <  pt            the layer's left context: the carry of the previous push, or at the first push of an utterance what the
//                        offline call pads with -- the reflection act(x)[pt - p] (SConv1d, pad1d mode "reflect", conv.py:82-99,251-253)
//                        or zeros (the 2-tap GEMM of a ConvTranspose1d, whose column -1 does not exist)
//     p <  pt + Tc       act(x)[p - pt],  act(x) = [elu](s0 / div + s1)
//     else               the reflection of the columns in front of it (the last push's extra_padding, conv.py:57-64), which may reach
//                        back into the carry
//   carry_out[b][c][j] = buf[b][c][Tc + j], j in [0, pt): the last pt columns of [carry | chunk], the next push's left context.
// carry_in and carry_out are different buffers (the session ping-pongs them), so every column has one writer and no reader of a
// location another thread writes.
struct StreamStage {
    Src s0, s1;                       // the chunk [B][C][Tc]; no pending affines (causal nets have no GroupNorm)
    int elu = 0; float alpha = 1.f;
    int B = 0, C = 0, Tc = 0, pt = 0, padR = 0;
    int left = 0;                     // 0 carry, 1 reflect, 2 zeros
    const float* carry_in = nullptr;  // [B][C][pt]
    float* carry_out = nullptr;       // [B][C][pt]
    float* buf = nullptr;             // [B][C][pt + Tc + padR]
};
hipError_t launch_stream_stage(const StreamStage& s, hipStream_t st);

}  // namespace fc
