// Slot session (fc_slots_*): the staging pass in front of every causal conv of a push whose rows start, continue, end and idle
// independently, and the per-row start of an utterance.  See slots_kernels.h for the contract.
// LDS-free streaming kernels, vector stores only, no atomics: every element has exactly one writer.
#include "slots_kernels.h"
#include "device_common.h"

namespace fc {

namespace {

struct StageArgs {
    const float *s0, *s1, *div, *carry_in;
    float *carry_out, *buf;
    const int *lens, *flags;
    int ldiv, lmul;
    int C, T, Tp, k, pt, stride, transposed, elu;
    float alpha;
};

constexpr int kStageSeg = 2048;      // staged columns per workgroup row

// One workgroup = one (slot, channel quad, column segment), one wave per channel row; a lane takes four staged columns at a time: where all
// four are the row's own columns they move as one 16-byte load and one 16-byte store (dword-aligned vector accesses), the context, the
// padding and the row's end as single dwords.  The first segment's workgroup also writes the row's new carry.
__global__ __launch_bounds__(256) void slots_stage_kernel(const StageArgs p) {
    const int lane = threadIdx.x & 63, c = 4 * blockIdx.x + (threadIdx.x >> 6), b = blockIdx.y;
    if (c >= p.C) return;
    const int pt = p.pt, len = p.lens[b], fl = p.flags[b];
    const int n = len > 0 ? min(ragged_cols(len, p.ldiv, p.lmul, 0), p.T) : 0;      // host-checked: never beyond T
    const bool start = (fl & kSlotStart) != 0;
    int extra = (n > 0 && !p.transposed && (fl & kSlotFinal)) ? ragged_extra(n, p.k, pt, p.stride) : 0;
    if (extra > p.Tp - pt - n) extra = p.Tp - pt - n;                               // host-checked: it fits
    const size_t row = (size_t)b * p.C + c;
    const float* x0 = p.s0 + row * p.T;
    const float* x1 = p.s1 ? p.s1 + row * p.T : nullptr;
    const float* cin = p.carry_in + row * pt;
    float* cout = p.carry_out + row * pt;
    float* out = p.buf + row * p.Tp;
    const float dv = p.div ? p.div[b] : 1.f;
    auto act = [&](float v, float w) __attribute__((always_inline)) {
        if (p.div) v = v / dv;
        if (x1) v = v + w;
        if (p.elu) v = elu_f(v, p.alpha);
        return v;
    };
    auto chunk_at = [&](int t) __attribute__((always_inline)) { return act(x0[t], x1 ? x1[t] : 0.f); };
    // column q of [left context | row]; q < pt + n
    auto left_at = [&](int q) __attribute__((always_inline)) {
        if (!start) return cin[q];
        const int src = pt - q;                               // reflection about the row's column 0; a row shorter than that reads as zero-extended
        return (!p.transposed && src < n) ? chunk_at(src) : 0.f;
    };
    auto concat_at = [&](int q) __attribute__((always_inline)) { return q < pt ? left_at(q) : chunk_at(q - pt); };
    const int end = pt + n, last = end - 1;
    auto col = [&](int q) __attribute__((always_inline)) {    // staged column q
        if (n == 0 || q >= end + extra) return 0.f;
        if (q < end) return concat_at(q);
        const int src = 2 * last - q;                         // the FINAL row's extra_padding: reflection about its last column
        return src >= 0 ? concat_at(src) : 0.f;
    };
    const int q_end = min(p.Tp, (int)(blockIdx.z + 1) * kStageSeg);
    for (int q0 = blockIdx.z * kStageSeg + 4 * lane; q0 < q_end; q0 += 256) {
        if (q0 >= pt && q0 + 3 < end && q0 + 3 < q_end) {
            const int t = q0 - pt;
            const f32x4 a = *(const f32x4u*)(x0 + t);
            const f32x4 w = x1 ? (f32x4)(*(const f32x4u*)(x1 + t)) : a;
            f32x4 y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = act(a[j], w[j]);
            *(f32x4u*)(out + q0) = y;
        } else {
            for (int j = 0; j < 4 && q0 + j < q_end; ++j) out[q0 + j] = col(q0 + j);
        }
    }
    if (blockIdx.z == 0)
        for (int j = lane; j < pt; j += 64) cout[j] = n == 0 ? cin[j] : concat_at(n + j);
}

// one workgroup per slot; a row that does not start is left alone
__global__ __launch_bounds__(256) void slots_start_kernel(const int* __restrict__ flags, int S, float* __restrict__ lstm, int L, int H,
                                                          const float* __restrict__ scale_in, float* __restrict__ scale_out) {
    const int b = blockIdx.x;
    if (!(flags[b] & kSlotStart)) return;
    if (lstm)
        for (int i = threadIdx.x; i < 3 * L * H; i += 256) lstm[((size_t)(i / H) * S + b) * H + i % H] = 0.f;      // h [L][2][S][H] | c [L][S][H]
    if (scale_out && threadIdx.x == 0) scale_out[b] = scale_in ? scale_in[b] : 1.f;
}

// The slot record (slots_kernels.h states it).  One workgroup = one chunk of kSlotRecChunk record floats of one segment of one named
// slot; a lane takes four record floats at a time, in groups that begin where the RECORD is 16-byte aligned.  A group that lies whole
// inside one row (and, for a cache plane, inside the frames in use) moves as one 16-byte load and one 16-byte store: aligned on the
// record side by construction, and on the state side aligned where the state is 16-byte aligned too, else a dword-aligned vector
// access (row offsets such as b * cin * pt are generally not multiples of four floats).  The head in front of the first aligned
// group, the tail, the groups across a row's end and the zero columns move as single floats.  Every float has one writer.
template <bool IMPORT>
__global__ __launch_bounds__(256) void slot_record_kernel(float* __restrict__ state, const SlotSeg* __restrict__ segs, const SlotRef* __restrict__ refs,
                                                          float* __restrict__ records, size_t pitch) {
    const SlotSeg sg = segs[blockIdx.y];
    const SlotRef rf = refs[blockIdx.z];
    const int dec = sg.side == 1;
    const bool live = sg.side < 0 || (rf.bits & (dec ? kSlotRecDecLive : kSlotRecEncLive));
    if (IMPORT && !live) return;                                   // a side that is not Running: the destination keeps what it has
    const int frames = dec ? rf.dec_frames : rf.enc_frames;
    const int fr_e = (rf.enc_frames + 15) & ~15, fr_d = (rf.dec_frames + 15) & ~15;      // seq_cache_pitch of either side
    const bool plane = sg.len == 0;
    const int row = plane ? (dec ? fr_d : fr_e) : sg.len;          // record floats per row
    const int used = plane ? frames : sg.len;                      // of which the state holds this many
    const long long total = (long long)sg.rows * row;
    const long long j_lo = (long long)blockIdx.x * kSlotRecChunk;
    if (j_lo >= total) return;
    const long long j_hi = min(total, j_lo + kSlotRecChunk);
    float* rec = records + (size_t)blockIdx.z * pitch + sg.rec_fixed + (long long)sg.enc_cols * fr_e + (long long)sg.dec_cols * fr_d;
    const int par = (rf.bits >> dec) & 1;
    float* st = state + sg.st_off + par * sg.half + (long long)rf.slot * sg.slot_stride;
    const int st_pitch = plane ? sg.st_pitch : sg.len;
    const int head = (int)((4 - (((uintptr_t)rec >> 2) & 3)) & 3);  // record floats in front of its first 16-byte boundary
    auto one = [&](long long j) __attribute__((always_inline)) {
        const int r = (int)(j / row), f = (int)(j - (long long)r * row);
        if (IMPORT) {
            if (f < used) st[(long long)r * st_pitch + f] = rec[j];
        } else {
            rec[j] = (live && f < used) ? st[(long long)r * st_pitch + f] : 0.f;
        }
    };
    // groups: g = 0 is the head [0, head), group g >= 1 holds [head + 4 (g - 1), head + 4 g); the chunk's groups are those that BEGIN in it
    for (long long g = j_lo / 4 + threadIdx.x; ; g += 256) {
        const long long a = g == 0 ? 0 : head + 4 * (g - 1), b = min(total, head + 4 * g);
        if (a >= j_hi || a >= total) break;
        if (a < j_lo) continue;                                    // begins in the chunk in front: its workgroup moves it
        const int r = (int)(a / row), f = (int)(a - (long long)r * row);
        if (b - a == 4 && f + 3 < row && (IMPORT ? f + 3 < used : (live && f + 3 < used))) {
            float* s = st + (long long)r * st_pitch + f;
            float* d = rec + a;
            const bool aligned = (((uintptr_t)s) & 15) == 0;
            if (IMPORT) {
                const f32x4 v = *(const f32x4*)d;
                if (aligned) *(f32x4*)s = v; else *(f32x4u*)s = v;
            } else {
                const f32x4 v = aligned ? *(const f32x4*)s : (f32x4)(*(const f32x4u*)s);
                *(f32x4*)d = v;
            }
        } else {
            for (long long j = a; j < b; ++j) one(j);
        }
    }
}

}  // namespace

hipError_t launch_slot_record(bool import, float* state, const SlotSeg* segs, int n_segs, const SlotRef* refs, int n, float* records, size_t pitch,
                              long long max_floats, hipStream_t st) {
    if (!state || !segs || !refs || !records || n_segs <= 0 || n_segs > 65535 || n <= 0 || n > 65535 || max_floats <= 0) return hipErrorInvalidValue;
    if ((uintptr_t)records & 3) return hipErrorInvalidValue;
    // One grid for all segments, so x is sized by the longest one: beside a full cache plane (some 190 chunks) every short segment --
    // scale, carry, h, c -- starts workgroups that read their segment's length and return at once, and the zeros of a side that is not
    // Running go out as single floats.  Both are left as they are: the empty workgroups cost no memory traffic, the zeros are a few KB,
    // and the large records, the only ones whose time is not the launch's, move at HBM rate (profiles/slot_record.txt).
    const dim3 grid((unsigned)((max_floats + kSlotRecChunk - 1) / kSlotRecChunk), n_segs, n);      // a group is moved by the chunk it begins in
    if (import) hipLaunchKernelGGL(slot_record_kernel<true>, grid, dim3(256), 0, st, state, segs, refs, records, pitch);
    else hipLaunchKernelGGL(slot_record_kernel<false>, grid, dim3(256), 0, st, state, segs, refs, records, pitch);
    return hipGetLastError();
}

hipError_t launch_slots_stage(const SlotsStage& s, hipStream_t st) {
    if (s.S <= 0 || s.S > 65535 || s.C <= 0 || s.T <= 0 || s.pt < 0 || s.stride < 1 || !s.len.lens || !s.flags || s.len.add != 0) return hipErrorInvalidValue;
    if (s.s0.aff || s.s1.aff || s.s1.div || s.s0.ld || s.s1.ld || (s.pt > 0 && (!s.carry_in || !s.carry_out))) return hipErrorInvalidValue;
    if (s.transposed ? (s.pt != 1 || s.Tp < 1 + s.T) : s.Tp < s.pt + s.T + ragged_extra(s.T, s.k, s.pt, s.stride)) return hipErrorInvalidValue;
    StageArgs a;
    a.s0 = s.s0.ptr; a.s1 = s.s1.ptr; a.div = s.s0.div; a.carry_in = s.carry_in; a.carry_out = s.carry_out; a.buf = s.buf;
    a.lens = s.len.lens; a.flags = s.flags; a.ldiv = s.len.div; a.lmul = s.len.mul;
    a.C = s.C; a.T = s.T; a.Tp = s.Tp; a.k = s.k; a.pt = s.pt; a.stride = s.stride; a.transposed = s.transposed; a.elu = s.elu; a.alpha = s.alpha;
    hipLaunchKernelGGL(slots_stage_kernel, dim3((s.C + 3) / 4, s.S, (s.Tp + kStageSeg - 1) / kStageSeg), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_slots_start(const int* flags, int S, float* lstm, int L, int H, const float* scale_in, float* scale_out, hipStream_t st) {
    if (!flags || S <= 0 || (lstm && (L < 1 || H < 1))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(slots_start_kernel, dim3(S), dim3(256), 0, st, flags, S, lstm, L, H, scale_in, scale_out);
    return hipGetLastError();
}

}  // namespace fc
