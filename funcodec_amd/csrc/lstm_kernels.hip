// gfx950 (MI355X / CDNA4) kernels of the SLSTM bottleneck: the layer-wavefront step and the persistent two-layer recurrence.
// fp32 throughout; the recurrent products run on v_mfma_f32_16x16x4_f32 (an fmaf chain in k order).
#include "device_common.h"
#include "kernels.h"

namespace fc {

// =================================================================================================
// LSTM (nn.LSTM inside SLSTM, lstm.py:12-28).  Workgroup j owns the 16 gate rows {i,f,g,o} x 4 hidden units (rows
//    permuted at load time), split-K over its waves, gates + state update fused.
//    gates = (W_hh h_{t-1}) + xproj_t,  xproj = W_ih x_t + b_ih + b_hh computed for all t at once by the conv kernel (k = 1).
// =================================================================================================
// Gate nonlinearities on the hardware exp2 / rcp (1 ulp each): sigmoid(v) = 1 / (1 + 2^(-v log2 e)), tanh(v) = 2 sigmoid(2v) - 1.
// Absolute error <= ~2e-7 (the libm versions are ~40 and ~60 VALU instructions and sit on the recurrence's critical path);
// measured end to end: every golden index still bit-exact, LSTM outputs within 1e-5 of torch (tests/test_gpu_parity.py).
__device__ __forceinline__ float sigmoid_f(float v) {
    const float e = __builtin_amdgcn_exp2f(-1.44269504088896341f * v);      // +inf for very negative v -> rcp gives 0
    return __builtin_amdgcn_rcpf(1.f + e);
}
__device__ __forceinline__ float tanh_f(float v) {
    const float e = __builtin_amdgcn_exp2f(-2.88539008177792681f * v);
    return fmaf(2.f, __builtin_amdgcn_rcpf(1.f + e), -1.f);
}
// c' = f * c + i * g with ONE explicit rounding order -- fma(f, c, round(i * g)) -- in every LSTM kernel: left to hipcc's contraction the
// same expression became v_mul + v_fmac in one kernel and v_pk_mul + v_add in another (one ulp apart; the persistent and the per-step
// forms are tested for bit equality)
__device__ __forceinline__ float lstm_cell(float gf, float c, float gi, float gg) { return __fmaf_rn(gf, c, __fmul_rn(gi, gg)); }

// -------------------------------------------------------------------------------------------------
// Layer-wavefront LSTM step: launch s advances layer l by its timestep t = s - l for ALL layers at once
// (T + L - 1 launches instead of L*T, and no separate x-projection GEMM for layers >= 1, whose input
// h_{l-1}(t) is consumed straight from the previous launch):
//   layer 0 : gates = xproj[t] + W_hh0 . h0(t-1)
//   layer l : gates = bias_l + [W_ih_l | W_hh_l] . [h_{l-1}(t) ; h_l(t-1)]
// hidden states ping-pong on the parity of their own timestep: h[l][t & 1].
// -------------------------------------------------------------------------------------------------
struct LstmWaveArgs {
    const float* w[FC_LSTM_MAX_LAYERS];
    const float* bias[FC_LSTM_MAX_LAYERS];
    const float* xproj;
    float* h;
    float* c;
    float* y;
    int B, H, T, L, s, KS;
    // MASKED form only (a push of a slot session): row b takes ceil(steps[b] / sdiv) * smul of the T steps
    const int* steps;
    int sdiv, smul;
};

// MASKED: a step beyond a row's own count carries h_l across the parity and leaves c alone (y = 0 there), so that after the launch
// sequence every row's last hidden state sits at the same parity whatever its count.  A live step of a row is computed exactly as in the
// plain form (rows are independent columns of the MFMA).
template <int NS, bool MASKED = false>
__global__ __launch_bounds__(256) void lstm_wave_kernel(const LstmWaveArgs p) {
    __shared__ f32x4 red[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, r16 = lane & 15;
    const int H = p.H, B = p.B;
    const int nblk = H >> 2;
    const int layer = blockIdx.x / nblk, blk = blockIdx.x - layer * nblk;
    const int t = p.s - layer;
    if (t < 0 || t >= p.T) return;
    const int kslice = H / p.KS;
    const int nsteps = kslice >> 4;
    const bool active = wid < p.KS;
    const int nseg = layer == 0 ? 1 : 2;
    const int wstride = layer == 0 ? H : 2 * H;
    const float* wbase = p.w[layer] + ((size_t)blk * 16 + r16) * wstride + (active ? wid : 0) * kslice + 4 * g;
    const size_t BH = (size_t)B * H;
    float* hl = p.h + (size_t)layer * 2 * BH;
    const float* h_own_prev = hl + (size_t)((t + 1) & 1) * BH;                  // h_l(t-1): parity (t-1)&1
    const float* h_below = layer ? p.h + (size_t)(layer - 1) * 2 * BH + (size_t)(t & 1) * BH : nullptr;   // h_{l-1}(t)
    float* h_out = hl + (size_t)(t & 1) * BH;
    float* cl = p.c + (size_t)layer * BH;
    constexpr int NA = NS > 0 ? NS : 1;
    const int nbt = (B + 15) >> 4;
    for (int nb = 0; nb < nbt; ++nb) {
        const int brow = nb * 16 + r16;
        const bool bvalid = brow < B;
        const size_t ci = (size_t)(bvalid ? brow : 0) * H + (size_t)blk * 4 + g;
        f32x4 xp = {0.f, 0.f, 0.f, 0.f};
        float cprev = 0.f;
        if (wid == 0) {
            if (layer == 0) xp = *(const f32x4*)(p.xproj + ((size_t)t * B + (bvalid ? brow : 0)) * 4 * H + (size_t)blk * 16 + 4 * g);
            else xp = *(const f32x4*)(p.bias[layer] + (size_t)blk * 16 + 4 * g);
            cprev = cl[ci];
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int seg = 0; seg < nseg; ++seg) {
            const float* wrow = wbase + (nseg == 2 ? seg * H : 0);
            const float* hsrc = (nseg == 2 && seg == 0) ? h_below : h_own_prev;
            const float* hrow = hsrc + (size_t)(bvalid ? brow : 0) * H + (active ? wid : 0) * kslice + 4 * g;
            if (NS > 0) {
                f32x4 a4[NA], b4[NA];
#pragma unroll
                for (int q = 0; q < NA; ++q) {
                    a4[q] = *(const f32x4*)(wrow + 16 * q);
                    b4[q] = *(const f32x4*)(hrow + 16 * q);
                    if (!bvalid) b4[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int q = 0; q < NA; ++q) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (q & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q][j], b4[q][j], acc1, 0, 0, 0);
                        else acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q][j], b4[q][j], acc, 0, 0, 0);
                    }
                }
            } else if (active) {
                for (int q = 0; q < nsteps; ++q) {
                    const f32x4 av = *(const f32x4*)(wrow + 16 * q);
                    f32x4 bv = *(const f32x4*)(hrow + 16 * q);
                    if (!bvalid) bv = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
                }
            }
        }
        acc = acc + acc1;
        if (!active) acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        red[wid][lane] = acc;
        __syncthreads();
        if (wid == 0) {
            f32x4 sgate = red[0][lane];
            for (int w = 1; w < p.KS; ++w) sgate = sgate + red[w][lane];
            bool masked = false;
            if (MASKED) masked = bvalid && t >= (p.steps[brow] + p.sdiv - 1) / p.sdiv * p.smul;
            if (masked) {
                h_out[ci] = h_own_prev[ci];
                if (layer == p.L - 1) p.y[ci * p.T + t] = 0.f;
            } else if (bvalid) {
                const float gi = sigmoid_f(sgate[0] + xp[0]);
                const float gf = sigmoid_f(sgate[1] + xp[1]);
                const float gg = tanh_f(sgate[2] + xp[2]);
                const float go = sigmoid_f(sgate[3] + xp[3]);
                const float cn = lstm_cell(gf, cprev, gi, gg);
                const float hn = go * tanh_f(cn);
                cl[ci] = cn;
                h_out[ci] = hn;
                if (layer == p.L - 1) p.y[ci * p.T + t] = hn;
            }
        }
        __syncthreads();
    }
}

hipError_t launch_lstm_wave(const float* const* w, const float* const* bias, const float* xproj, float* h, float* c,
                            float* y, int B, int H, int T, int L, int s, hipStream_t st, const int* steps, int sdiv, int smul) {
    if (H % 16 != 0 || L < 1 || L > FC_LSTM_MAX_LAYERS || (steps && (sdiv < 1 || smul < 1))) return hipErrorInvalidValue;
    LstmWaveArgs a;
    for (int l = 0; l < FC_LSTM_MAX_LAYERS; ++l) { a.w[l] = l < L ? w[l] : nullptr; a.bias[l] = l < L ? bias[l] : nullptr; }
    a.xproj = xproj; a.h = h; a.c = c; a.y = y; a.B = B; a.H = H; a.T = T; a.L = L; a.s = s;
    a.steps = steps; a.sdiv = sdiv; a.smul = smul;
    int KS = 4;
    while (KS > 1 && (H % (16 * KS)) != 0) KS >>= 1;
    a.KS = KS;
    const int ns = H / (16 * KS);
    dim3 grid(L * (H / 4)), block(256);
    if (steps) {
        switch (ns) {
            case 1: hipLaunchKernelGGL((lstm_wave_kernel<1, true>), grid, block, 0, st, a); break;
            case 2: hipLaunchKernelGGL((lstm_wave_kernel<2, true>), grid, block, 0, st, a); break;
            case 4: hipLaunchKernelGGL((lstm_wave_kernel<4, true>), grid, block, 0, st, a); break;
            case 8: hipLaunchKernelGGL((lstm_wave_kernel<8, true>), grid, block, 0, st, a); break;
            case 16: hipLaunchKernelGGL((lstm_wave_kernel<16, true>), grid, block, 0, st, a); break;
            default: hipLaunchKernelGGL((lstm_wave_kernel<0, true>), grid, block, 0, st, a); break;
        }
        return hipGetLastError();
    }
    switch (ns) {
        case 1: hipLaunchKernelGGL(lstm_wave_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(lstm_wave_kernel<2>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(lstm_wave_kernel<4>, grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL(lstm_wave_kernel<8>, grid, block, 0, st, a); break;
        case 16: hipLaunchKernelGGL(lstm_wave_kernel<16>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(lstm_wave_kernel<0>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------------
// Persistent 2-layer LSTM: ONE launch for the whole recurrence.  Workgroup j keeps the 16 gate rows of layer 0
// (W_hh0) and of layer 1 ([W_ih1 | W_hh1]) for its 4 hidden units in REGISTERS for all T steps (192 KiB per CU,
// one 4-wave workgroup per CU owns the whole 512-register file), cell states stay in registers too.
//
// Hidden-state exchange.  Every wavefront step writes h0(s) / h1(s-1) into a HISTORY buffer that is never
// overwritten inside one launch ([T+1][B][H] per layer, slot 0 = zeros).  Stores are write-through (sc1), so when a
// wave's vmcnt drains its values are in memory; the consumers read slot s only after the grid barrier of step s-1 and
// nobody has touched those addresses before in this launch, so no cache on the chip can hold a stale copy of them:
// the loads are PLAIN loads, the first workgroup of an XCD to touch a line pulls it over the fabric and the other 31
// hit that XCD's L2 (with double-buffered h and sc1 loads every workgroup fetched all 128 KiB over the fabric every
// step: 32 MiB per step, the largest term of the step time).
//
// Grid barrier: 16 arrival counters on separate cache lines (16 arrivals each instead of 256 atomics serialised on
// one address), polled by the 16 low lanes of wave 0 with one load each; monotonic targets, bounded spin (on a
// timeout the error word is set and every workgroup runs to completion instead of hanging).
// Same arithmetic order per accumulator as lstm_wave_kernel (bit-identical results).
// -------------------------------------------------------------------------------------------------
struct LstmPersistArgs {
    const float *w0, *w1, *bias1, *xproj;
    float* hist;         // [BH zeros][T x BH: h0(0..T-1)][T x BH: h1(0..T-1)], BH = 16 * tiles * H; one slot = [batch tile][H/4][16 rows][4 units]:
                         // the 64 lanes of a consumer's B-fragment load read 1 KiB of CONTIGUOUS memory (lane (g, r) = 16 bytes at 16*lane),
                         // and the 64 producer lanes of a workgroup write one contiguous 256-byte piece.  (Row-major [B][H] put the 16 lanes
                         // of a fragment row 4 KiB apart -- every lane of a load on its own cache line: 7.2 us per step instead of 5.1.)
    float* y;
    unsigned* sync;      // 16 counters at [32*i], error flag at [512]; zeroed by the caller before every launch
    unsigned* status;    // host-visible engine status words (kernels.h FC_STATUS_*), or null
    int B, H, T;
    int ablate;          // FC_ABLATE_LSTM in FC_AB_KNOBS builds: 1 no grid barrier (profiling aid, wrong results).  Ignored (FC_ABL) in the shipped library
    int test_timeout;    // test hook (FC_ABLATE_LSTM=64, the only value the shipped library honours): behave as if the grid barrier had timed out
    int tile_base, tiles;   // first 16-row batch tile of this launch / tiles of the whole call (history slot size, barrier word block)
    int groups;          // independent recurrences in one launch: group j = workgroups [j*H/4, (j+1)*H/4) owns batch rows [16j, 16j+16) with
                         // its own barrier words (H = 512 fills only half of the chip: two batch tiles then advance side by side)
};

constexpr int kLstmSyncWords = 1024;
// profiling builds only (FC_BUILD_DEFINES="FC_LSTM_ABL=<mask>", results are garbage): 1 no critical-path MFMAs, 2 no hidden-state loads,
// 4 no shadow MFMAs, 8 no y stores, 16 no store drain before the arrival.  Compile time, because a run-time branch around the loads
// would make hipcc wait for them at the join.
#ifndef FC_LSTM_ABL
#define FC_LSTM_ABL 0
#endif

// split grid barrier: arrive (after this workgroup's stores have drained) ... independent work ... wait
__device__ __forceinline__ void lstm_barrier_arrive(unsigned* sync, int blk) {
    if (!(FC_LSTM_ABL & 16)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every storing wave drains its own write-through stores
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(sync + 32 * (blk & 15), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lstm_barrier_wait(unsigned* sync, unsigned target) {
    if (threadIdx.x < 64) {
        const unsigned* mine = sync + 32 * (threadIdx.x & 15);
        unsigned spins = 0;
        while (true) {
            const unsigned v = __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__all(v >= target)) break;
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 255u) == 0u) {
                if (__hip_atomic_load(sync + 512, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                if (spins > (1u << 21)) { __hip_atomic_store(sync + 512, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            }
        }
    }
    __syncthreads();
}

// Wavefront schedule (T + 2 steps): at step s layer 0 produces h0(s) and layer 1 produces h1(s-2).  Layer 1 runs one
// step later than its data dependence requires so that its input half, P = W_ih1 . h0(s-1), is computed in the SHADOW
// of the grid barrier of step s (after this workgroup has arrived, before it starts polling) and only the two
// recurrent products (W_hh0 . h0(s-1), W_hh1 . h1(s-3)) sit on the critical path between two barriers.
template <int NS>
__global__ __launch_bounds__(256, 1) void lstm_persist_kernel(const LstmPersistArgs p) {
    // batch tiles (16 rows) per workgroup and step.  Fixed at one since round 3: a second tile of a call is a second group (H = 512) or a
    // second launch (H = 1024); the tile loops below are what is left of the two-tiles-per-step form (3.14 vs 2 x 1.26 ms) and fold away.
    constexpr int NBT = 1;
    static_assert(NS % 2 == 0, "k slices are issued in pairs");
    __shared__ f32x4 red[2][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, r16 = lane & 15;
    const int H = p.H, B = p.B, T = p.T;
    const int wgs = H >> 2;                          // workgroups of one recurrence
    const int grp = p.groups > 1 ? blockIdx.x / wgs : 0;
    const int blk = blockIdx.x - grp * wgs;
    const int tile0 = p.tile_base + grp;             // first batch tile of this group (groups > 1 run with NBT == 1)
    const int brow0 = tile0 * 16;                    // its first batch row
    unsigned* const sync = p.sync + (size_t)tile0 * kLstmSyncWords;
    const unsigned arrivals = (unsigned)wgs >> 4;    // per counter per step
    const int kslice = NS * 16;                      // H / 4 waves
    const size_t BH = (size_t)16 * p.tiles * H;      // floats per history slot (batch padded to whole tiles)
    // ---- weights -> registers (once)
    f32x4 a0[NS], a1i[NS], a1h[NS];
    {
        const float* w0r = p.w0 + ((size_t)blk * 16 + r16) * H + wid * kslice + 4 * g;
        const float* w1r = p.w1 + ((size_t)blk * 16 + r16) * 2 * H + wid * kslice + 4 * g;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            a0[q] = *(const f32x4*)(w0r + 16 * q);
            a1i[q] = *(const f32x4*)(w1r + 16 * q);
            a1h[q] = *(const f32x4*)(w1r + H + 16 * q);
        }
    }
    float cst[NBT];                                  // cell state of (batch row, unit): wave 0 -> layer 0, wave 1 -> layer 1
    f32x4 pa[NBT], pb[NBT];                          // P = W_ih1 . h0 of the NEXT step's layer-1 timestep (even / odd k slices)
#pragma unroll
    for (int nb = 0; nb < NBT; ++nb) {
        cst[nb] = 0.f;
        pa[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        pb[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const f32x4 bias1 = *(const f32x4*)(p.bias1 + (size_t)blk * 16 + 4 * g);
    float* const hist0 = p.hist;                     // slot k = h0(k-1), slot 0 = zeros
    float* const hist1 = p.hist + (size_t)T * BH;    // slot k >= 1 = h1(k-1) (slot 0 is never addressed through this base)
    f32x4 b0keep[NS];

    for (int s = 0; s <= T + 1; ++s) {
        const bool act0 = s < T, act1 = s >= 2;
        const float* h0in = hist0 + (size_t)(s <= T ? s : T) * BH;                   // h0(s-1)
        const float* h1in = s >= 3 ? hist1 + (size_t)(s - 2) * BH : hist0;           // h1(s-3)
        float* h0o = hist0 + (size_t)(s + 1) * BH;                                   // h0(s)     (s < T)
        float* h1o = hist1 + (size_t)(s - 1) * BH;                                   // h1(s-2)   (s >= 2)
#pragma unroll
        for (int nb = 0; nb < NBT; ++nb) {
            const int brow = brow0 + nb * 16 + r16;
            const bool bvalid = brow < B;
            // rows >= B of the last tile are never written: their columns compute values nobody stores (MFMA columns are independent)
            const size_t hoff = (size_t)(tile0 + nb) * 16 * H + (size_t)wid * kslice * 16 + 4 * lane;
            f32x4 xp = {0.f, 0.f, 0.f, 0.f};
            if (wid == 0 && act0)
                xp = *(const f32x4*)(p.xproj + ((size_t)s * B + (bvalid ? brow : 0)) * 4 * H + (size_t)blk * 16 + 4 * g);
            f32x4 b0l[NBT == 1 ? 1 : NS], b1[NS];
            f32x4 (&b0)[NS] = *(NBT == 1 ? &b0keep : (f32x4 (*)[NS])&b0l);   // single batch tile: h0(s-1) stays in registers for the shadow phase
            // All 2*NS loads are issued back to back in the order the MFMAs consume them and NOTHING touches the values before
            // their MFMA: the k slices then start as they arrive (counted vmcnt) instead of after the last one (round 1 masked
            // the columns of batch rows >= B right after the loads, which put one vmcnt(0) in front of all 128 MFMAs: 3.3 us
            // of loads and 2.1 us of MFMAs ran back to back).  Columns of rows >= B read row 0 and compute values nobody stores.
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                if (FC_LSTM_ABL & 2) { b0[q] = (f32x4){0.f, 0.f, 0.f, 0.f}; b1[q] = b0[q]; continue; }
                b0[q] = *(const f32x4*)(h0in + hoff + 256 * q);
                b1[q] = *(const f32x4*)(h1in + hoff + 256 * q);
            }
            // four accumulators (layer 0 / layer 1 x even / odd k slice); the ISSUE order interleaves them so that two
            // MFMAs on the same accumulator are never back to back, the order WITHIN each accumulator is that of
            // lstm_wave_kernel (layer 1: the W_ih1 terms -- already in pa / pb -- then the W_hh1 terms)
            f32x4 c0a = {0.f, 0.f, 0.f, 0.f}, c0b = {0.f, 0.f, 0.f, 0.f};
            f32x4 c1a = pa[nb], c1b = pb[nb];
#pragma unroll
            for (int q = 0; q < ((FC_LSTM_ABL & 1) ? 0 : NS); q += 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    c0a = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[q][j], b0[q][j], c0a, 0, 0, 0);
                    c1a = __builtin_amdgcn_mfma_f32_16x16x4f32(a1h[q][j], b1[q][j], c1a, 0, 0, 0);
                    c0b = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[q + 1][j], b0[q + 1][j], c0b, 0, 0, 0);
                    c1b = __builtin_amdgcn_mfma_f32_16x16x4f32(a1h[q + 1][j], b1[q + 1][j], c1b, 0, 0, 0);
                }
            }
            red[0][wid][lane] = c0a + c0b;
            red[1][wid][lane] = c1a + c1b;
            __syncthreads();
            if (wid < 2) {
                const int layer = wid;
                const bool act = layer ? act1 : act0;
                f32x4 sg = red[layer][0][lane];
                for (int w = 1; w < 4; ++w) sg = sg + red[layer][w][lane];
                const f32x4 add = layer ? bias1 : xp;
                if (act && bvalid) {
                    const float gi = sigmoid_f(sg[0] + add[0]);
                    const float gf = sigmoid_f(sg[1] + add[1]);
                    const float gg = tanh_f(sg[2] + add[2]);
                    const float go = sigmoid_f(sg[3] + add[3]);
                    const float cn = lstm_cell(gf, cst[nb], gi, gg);
                    const float hn = go * tanh_f(cn);
                    cst[nb] = cn;
                    const size_t ci = (size_t)brow * H + (size_t)blk * 4 + g;
                    const size_t hi = (size_t)(tile0 + nb) * 16 * H + ((size_t)blk * 16 + r16) * 4 + g;
                    if (layer == 0) __hip_atomic_store(&h0o[hi], hn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else { __hip_atomic_store(&h1o[hi], hn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); if (!(FC_LSTM_ABL & 8)) p.y[ci * T + (s - 2)] = hn; }
                }
            }
            __syncthreads();
        }
        if (s > T) break;
        const bool do_sync = !FC_ABL(p.ablate, 1);
        if (do_sync) lstm_barrier_arrive(sync, blk);
        // ---- barrier shadow: P for the next step's layer-1 timestep t = s - 1 (needs h0(s-1), already visible)
        if (s >= 1) {
#pragma unroll
            for (int nb = 0; nb < NBT; ++nb) {
                const size_t hoff = (size_t)(tile0 + nb) * 16 * H + (size_t)wid * kslice * 16 + 4 * lane;
                f32x4 b0l[NBT == 1 ? 1 : NS];
                f32x4 (&b0)[NS] = *(NBT == 1 ? &b0keep : (f32x4 (*)[NS])&b0l);
                if (NBT > 1) {                        // several batch tiles: re-read (L2 hit) instead of holding NBT x 64 registers
#pragma unroll
                    for (int q = 0; q < NS; ++q) b0[q] = *(const f32x4*)(h0in + hoff + 256 * q);
                }
                f32x4 c1a = {0.f, 0.f, 0.f, 0.f}, c1b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < ((FC_LSTM_ABL & 4) ? 0 : NS); q += 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        c1a = __builtin_amdgcn_mfma_f32_16x16x4f32(a1i[q][j], b0[q][j], c1a, 0, 0, 0);
                        c1b = __builtin_amdgcn_mfma_f32_16x16x4f32(a1i[q + 1][j], b0[q + 1][j], c1b, 0, 0, 0);
                    }
                }
                pa[nb] = c1a; pb[nb] = c1b;
            }
        }
        if (do_sync) lstm_barrier_wait(sync, (unsigned)(s + 1) * arrivals);
    }
    // a barrier that timed out (some workgroup was not resident) must not pass for a result: poison this workgroup's
    // outputs so that the failure is loud downstream (the engine's per-step launch path is the supported fallback)
    if (__hip_atomic_load(sync + 512, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || p.test_timeout) {
        if (p.status && tid == 0) *(volatile unsigned*)(p.status + FC_STATUS_LSTM_TIMEOUT) = 1u;   // read by the host at its next fc_* call
        for (int i = tid; i < 4 * B * T; i += 256) {
            const int t = i % T, bu = i / T;
            p.y[((size_t)(bu / 4) * H + (size_t)blk * 4 + (bu & 3)) * T + t] = __builtin_nanf("");
        }
    }
}

// H = 512 occupies 128 of the 256 CUs: a second batch tile gets its own 128 workgroups (and barrier words) instead of a second pass
static int lstm_persist_groups(int B, int H) { return (H == 512 && B > 16) ? 2 : 1; }

// history slots hold whole 16-row batch tiles (LstmPersistArgs::hist)
static int lstm_persist_tiles(int B) { return (B + 15) / 16; }
static size_t lstm_persist_slot_floats(int B, int H) { return (size_t)16 * lstm_persist_tiles(B) * H; }
size_t lstm_persist_state_floats(int B, int H, int T) { return (size_t)kLstmSyncWords * lstm_persist_tiles(B) + (size_t)(2 * T + 1) * lstm_persist_slot_floats(B, H); }
size_t lstm_persist_clear_floats(int B, int H) { return (size_t)kLstmSyncWords * lstm_persist_tiles(B) + lstm_persist_slot_floats(B, H); }

// `state`: lstm_persist_state_floats() floats whose first lstm_persist_clear_floats() are zero (barrier words + the
// all-zero initial hidden state)
hipError_t launch_lstm_persist(const float* w0, const float* w1, const float* bias1, const float* xproj, float* state, float* y,
                               int B, int H, int T, unsigned* status, hipStream_t st) {
    LstmPersistArgs a;
    const int groups = lstm_persist_groups(B, H);
    const int tiles = lstm_persist_tiles(B);
    a.w0 = w0; a.w1 = w1; a.bias1 = bias1; a.xproj = xproj; a.hist = state + (size_t)kLstmSyncWords * tiles; a.y = y;
    a.sync = (unsigned*)state; a.status = status; a.B = B; a.H = H; a.T = T; a.groups = groups; a.tile_base = 0; a.tiles = tiles;
    // FC_ABLATE_LSTM: the profiling masks are tuning-build knobs (ab_knob); the shipped library honours exactly one value, 64 = the barrier-timeout
    // TEST hook of tests/test_gpu_parity.py (every other value is ignored: mask 1 removes the grid barrier and gives wrong results)
    static const int hook = getenv("FC_ABLATE_LSTM") ? atoi(getenv("FC_ABLATE_LSTM")) : 0;
#ifdef FC_AB_KNOBS
    static const int ablate = hook;
#else
    static const int ablate = 0;         // (not through ab_knob: the variable is legitimately set by the timeout test, no "ignored" notice)
#endif
    a.ablate = ablate & ~64;
    a.test_timeout = (hook == 64 || (ablate & 64)) ? 1 : 0;
    // H = 1024 fills the chip with ONE batch tile: a second tile (17 .. 32 utterances) is a second launch of the same kernel on its own
    // history columns and barrier words (round 3: 2 x 1.26 ms; the two-tiles-per-step instantiation needed 3.14 ms with the new history
    // layout).  H = 512: two tiles side by side as two groups of 128 workgroups in one launch.
    dim3 grid(H / 4 * groups), block(256);
    // FC_LSTM_COOP=1: hipLaunchCooperativeKernel (the runtime validates the grid against the occupancy query at every launch,
    // +15-19 us of host time per launch); default: plain launch, residency validated once per engine by lstm_persist_supported()
    static const int coop = ab_knob("FC_LSTM_COOP", 0);
    void* kargs[] = {(void*)&a};
#define FC_LP(NS)                                                                                                \
    do {                                                                                                         \
        if (coop) { hipError_t ec = hipLaunchCooperativeKernel((const void*)lstm_persist_kernel<NS>, grid, block, kargs, 0, st); \
                    if (ec != hipSuccess) return ec; }                                                            \
        else hipLaunchKernelGGL((lstm_persist_kernel<NS>), grid, block, 0, st, a);                                 \
    } while (0)
    if (H == 1024) {
        for (int tb = 0; tb < tiles; ++tb) { a.tile_base = tb; FC_LP(16); }
    } else if (H == 512 && groups == tiles) FC_LP(8);
    else return hipErrorInvalidValue;
#undef FC_LP
    return hipGetLastError();
}

// can the persistent kernel be used? (every workgroup must be co-resident: one per CU)
// The grid barrier needs all H/4 workgroups resident at once.  Checked against the runtime's own occupancy answer for the
// instantiation that would run (not just the CU count): blocks per CU x CUs >= grid, with the one-block margin the
// microarchitecture guide asks for near an SGPR edge (the kernel needs exactly ONE block per CU on a 256-CU part, and
// two fit by registers, so the margin is met by construction).
bool lstm_persist_supported(int B, int H, int L, int device) {
    if (L != 2 || (H != 1024 && H != 512) || B > 32) return false;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return false;
    const int groups = lstm_persist_groups(B, H);
    int per_cu = 0;
    hipError_t e = hipErrorInvalidValue;
    if (H == 1024) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lstm_persist_kernel<16>, 256, 0);
    else if (H == 512) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lstm_persist_kernel<8>, 256, 0);
    if (e != hipSuccess || per_cu < 1) return false;
    return (long long)per_cu * prop.multiProcessorCount >= H / 4 * groups && prop.multiProcessorCount >= H / 4 * groups;
}

}  // namespace fc
