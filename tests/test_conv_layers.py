"""Every 1-D conv layer of the time-domain codec in every call form the drivers use, against a float64 CPU reference.

Each layer runs through `Engine.layer_forward(prefix, x0, elu, aff0=, div=, x1=, aff1=)` (fc_layer_forward_src), which hands the sources
to the drivers' own run_conv exactly as run_encoder / run_resblocks / run_decoder build them, so the kernel that runs is the one the
product picks for that layer, form and shape; the thin residual heads run through `Engine.resblock_forward(..., aff0=, x1=, aff1=)`
(fc_resblock_forward_src -> run_resblocks).  The reference is oracle/torch_oracle.py's sconv1d / sconvtr1d with the weights, the inputs,
the affines and the divisor cast to double, and the divide, the affine, the sum and the ELU applied in double before the conv.

Call forms (n = a pending GroupNorm affine on GroupNorm nets; the weight_norm nets take the same forms without affines):
  encoder first conv   raw audio / div[b] (audio_normalize), mono and stereo
  shortcut, block.1    x0 n (block j = 0) or x0 n + x1 n (j > 0); block.1 adds ELU
  block.3              x0 n, ELU
  encoder down conv    x0 n + x1 n, ELU
  encoder last conv    after the LSTM: x0 + x1 n (res_seq skip) and x0 alone, ELU; no sequence model: x0 n, ELU
  decoder first conv   x0 plain
  decoder convtr       stage 0: x0 (+ x1 n: the LSTM skip), or x0 n without a sequence model; later stages x0 n + x1 n; ELU
  decoder last conv    x0 n + x1 n, ELU (the few-output kernels)
  residual heads       the whole block on x0 n (j = 0) or x0 n + x1 n (j > 0): reshead_kernel<C, k, DUAL> for C = 32 / 64

Bars: max and RMS of |gpu - f64| at most ABS_K / RMS_K x torch float32's own error on the same inputs, above a floor of ABS_FLOOR /
RMS_FLOOR (x max(1, RMS of the reference) on the un-normalised weight_norm outputs), and never above the absolute bars of the older
per-layer tests (5e-5, 2e-4 where the GroupNorm covers < 4096 elements).  A GroupNorm over fewer than TINY_GN elements (the 1- and
2-channel last conv at T <= 3) amplifies rounding by up to 1 / sqrt(eps): there only the absolute bar holds.  Measured on an MI355X over
the ~5 600 cases of this file: worst max |gpu - f64| 1.6e-5 (encoder down conv, two sources; torch float32 4.6e-6), 2.6e-5 on a
2-element GroupNorm; above 2e-6 at most 10.9 x torch float32's max error (decoder first conv, K = 3584: the MFMA chunks sum in
order, torch's CPU kernel in blocks); RMS above 3e-7 at most 6.2 x torch's.

Reached (WANT, asserted): all four tile shapes, prologue modes 0 - 5, quad row staging NU 1 / 2 / 11 / 12, quad element staging NU 2 /
3 / 4, MODE 5 with NU 2 - 5, the round-4 layout (QK = false: 2-channel chunks -- the first convs of 1 / 2 audio channels and the
two-source k = 16, stride-8 down convs), all 12 reshead_kernel<C, k, DUAL>, and the dual few-output kernels (rows and streaming form,
k = 3 / 5 / 7, one output channel).

Compiled but reached by no net or form of this file (169 of the 220 conv_mfma_kernel instantiations; listed, not removed):
  * round-4 layout (QK = false), every tile: MODE 0 NU 9 / 11 / 16 / 18, MODE 1 / 2 NU 9 / 18, MODE 3 NU 5 / 9, MODE 4 NU 5; also
    MODE 0 / 1 NU 5 and MODE 2 NU 5 outside 32 x 256, MODE 4 NU 9 on 32 x 128.  A chunk takes this layout only at CC = 2, and CC stays
    2 only for Cin <= 2 (first convs, NU 5) or where a 4-channel slab does not fit the staging registers (k = 16 strided layers).
  * quad element staging NU 5 (all modes <= 2), and NU 2 - 4 where a tile shape's layers stage other slab widths (e.g. 128 x 128 MODE
    0 NU 3 / 4, 32 x 128 every NU).  NU = ceil((CC / 4) * slabW / 256): the nets' strided layers with one source take <= 3.
  * quad row staging: 32 x 128 is reached at MODE 0 only (the 32 x 128 tile is the bottleneck tiling for small_n layers of M <= 256,
    i.e. enc last / dec first, which take one plain or affine source); NU 11 needs CC / 4 * BN / 4 <= 64 (CC = 4 on 256-column tiles).
  * MODE 5 NU 1 and 6 on every tile, and NU 2 - 5 on 32 x 256 / 64 x 256: materialised inputs only arise on layers with >= 3 M tiles
    (M > 256 on 128-row tiles) or force_plain layers.
  * NU 13 / 14 (FC_ROW_CW) and the round-4 row staging (FC_AB_KNOBS) are compiled into tuning builds only.
  * conv_fewout_* with two or more output channels in the two-source form: the stereo nets' last conv (2 outputs) was not observed to
    dispatch to the few-output kernels in this file's runs.
"""
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LAYER_ABS_TOL = 5e-5          # the absolute bars of tests/test_gpu_parity.py's per-layer tests
SMALL_GN_TOL = 2e-4
ABS_FLOOR = 4e-6
ABS_K = 12.0
RMS_FLOOR = 6e-7
RMS_K = 8.0
TINY_GN = 64                  # GroupNorm over fewer elements: 1 / std amplifies any rounding difference; the absolute bar only
WIDE = 512                    # input channels from which T is capped (the float64 CPU reference)
WIDE_T = 129


# ---- the nets ----------------------------------------------------------------------------------------------------------------------
def _synthetic(nf, ratios, *, res_k=3, dil_base=2, n_res=1, compress=2, last_k=7, norm="time_group_norm", causal=False, seq="lstm",
               seq_layers=2, stereo=False, audio_normalize=True, dimension=32):
    from funcodec_amd.config import recipe_config
    cfg = recipe_config("tiny")
    hop = int(np.prod(ratios))
    for side in ("encoder_conf", "decoder_conf"):
        c = dict(cfg[side], ratios=list(ratios), n_filters=nf, residual_kernel_size=res_k, dilation_base=dil_base, n_residual_layers=n_res,
                 compress=compress, last_kernel_size=last_k, norm=norm, causal=causal, seq_model=seq, seq_layer_num=seq_layers)
        if norm != "time_group_norm":
            c.pop("norm_params", None)
        cfg[side] = c
    cfg["encoder_conf"]["dimension"] = dimension
    cfg["model_conf"] = dict(cfg["model_conf"], odim=dimension, audio_normalize=audio_normalize)
    cfg["quantizer_conf"] = dict(cfg["quantizer_conf"], encoder_hop_length=hop)
    if stereo:
        cfg["input_size"] = 2
        cfg["decoder_conf"]["channels"] = 2
    return cfg


# nets that are not named recipes (what the recipes do not reach): chunk tails (Cin % CC != 0: 12, 24, 48, 96 channels), strides 2, 3,
# 5, 8, dilation bases 1, 2, 3 with residual kernels 3, 5, 7, compress 1 / 2 / 4, last kernels 3 / 5 / 7 with 1 and 2 output channels,
# the reshead_kernel widths and taps, causal weight_norm stereo
CONFIGS = {
    "nf12st": lambda: _synthetic(12, (2, 3), res_k=5, dil_base=3, n_res=2, compress=1, last_k=3, seq_layers=1, stereo=True),
    "nf24c4": lambda: _synthetic(24, (5, 8), res_k=7, dil_base=2, n_res=3, compress=4, last_k=5, seq="none", audio_normalize=False),
    "wnc16st": lambda: _synthetic(16, (4, 2), res_k=3, dil_base=2, n_res=2, compress=2, last_k=7, norm="weight_norm", causal=True, stereo=True),
    "rh32k5": lambda: _synthetic(32, (2, 4), res_k=5, dil_base=2, n_res=2, compress=2, last_k=5, seq="none"),
    "rh32k7": lambda: _synthetic(32, (3, 8), res_k=7, dil_base=1, n_res=2, compress=2, last_k=3, seq_layers=1),
}

NETS = {
    # name: (seed, (T of the B = 1 case, T of the B = 3 case))
    "tiny": (7, (1, 1025)),
    "ds320": (0, (2, 257)),
    "ds640": (1, (3, 129)),
    "ds320wn": (2, (5, 256)),
    "ss320": (3, (1, 127)),
    "ss320nc": (4, (2, 255)),
    "tinyst": (5, (3, 1023)),
    "tinyss": (6, (7, 1024)),
    "nf12st": (8, (1, 257)),
    "nf24c4": (9, (2, 1025)),
    "wnc16st": (10, (3, 255)),
    "rh32k5": (11, (2, 129)),
    "rh32k7": (12, (5, 1023)),
}


@functools.lru_cache(maxsize=None)
def _parts(net):
    """(engine model, oracle) of a named recipe or of a CONFIGS net."""
    seed = NETS[net][0]
    if net not in CONFIGS:
        from helpers import engine_for, oracle_for
        return engine_for(net, seed), oracle_for(net, seed)
    cfg = CONFIGS[net]()
    from torch_oracle import Oracle
    from funcodec_amd.config import arch_from_config
    from funcodec_amd.model import EncodecMI355X
    from funcodec_amd.synth import make_state_dict
    arch = arch_from_config(cfg)
    sd = {k: torch.from_numpy(v) for k, v in make_state_dict(arch, seed).items()}
    m = EncodecMI355X(arch, "cuda:0")
    m.load_state_dict(sd)
    return m, Oracle(cfg, sd)


def layer_table(arch):
    """Every 1-D conv of the nets in execution order (plan.encoder_plan / decoder_plan, the oracle's encoder / decoder order), with the
    residual block index j and the decoder stage of a convtr."""
    from funcodec_amd.plan import decoder_plan, encoder_plan
    out = []
    for side, plan in (("enc", encoder_plan(arch)), ("dec", decoder_plan(arch))):
        j, stage = 0, -1
        for op in plan:
            if op.kind not in ("conv", "convtr"):
                continue
            if op.role in ("down", "up", "first"):
                j = 0
            if op.role == "up":
                stage += 1
            out.append(dict(op=op, side=side, j=j, stage=stage))
            if op.role == "block3":
                j += 1
    return out


def call_forms(L, arch):
    """(two sources?, affine on x0?, affine on x1?, ELU, divisor?) forms the drivers use for layer L."""
    op, side = L["op"], L["side"]
    n = arch.norm == "time_group_norm"
    seq = arch.lstm_layers > 0
    skip = seq and arch.lstm_skip
    r = op.role
    if r == "first":
        return [(False, False, False, False, side == "enc" and arch.audio_normalize)]
    if r in ("shortcut", "block1"):
        return [(L["j"] > 0, n, n and L["j"] > 0, r == "block1", False)]
    if r == "block3":
        return [(False, n, False, True, False)]
    if r == "down":
        return [(True, n, n, True, False)]
    if r == "up" and L["stage"] == 0:
        if not seq:
            return [(False, n, False, True, False)]
        return ([(True, False, n, True, False)] if skip else []) + [(False, False, False, True, False)]
    if r == "up":
        return [(True, n, n, True, False)]
    if side == "enc":                                   # encoder last conv
        if not seq:
            return [(False, n, False, True, False)]
        return ([(True, False, n, True, False)] if skip else []) + [(False, False, False, True, False)]
    return [(True, n, n, True, False)]                  # decoder last conv


def _affine(gen, B, C):
    """Per-(b, c) (scale, shift): scale in [0.5, 2], shift ~ N(0, 1) -- never the identity, which hides a swapped pair or a wrong channel."""
    return torch.stack([0.5 + 1.5 * torch.rand(B, C, generator=gen, dtype=torch.float64),
                        torch.randn(B, C, generator=gen, dtype=torch.float64)], -1).float()


def _prologue(x0, a0, div, x1, a1, elu, alpha, dt):
    def app(x, a):
        x = x.to(dt)
        return x if a is None else x * a[..., 0, None].to(dt) + a[..., 1, None].to(dt)
    v = x0.to(dt)
    if div is not None:
        v = v / div.to(dt)[:, None, None]
    v = app(v, a0)
    if x1 is not None:
        v = v + app(x1, a1)
    return F.elu(v, alpha) if elu else v


def _conv(orc, op, v, dt):
    import torch_oracle as TO
    w, b, g, be = (None if t is None else t.to(dt) for t in orc._p(op.key))
    if op.kind == "convtr":
        return TO.sconvtr1d(v, w, b, g, be, op.stride, orc.eps, orc.causal)
    return TO.sconv1d(v, w, b, g, be, op.stride, orc.eps, orc.causal, op.dilation)


def reference(orc, op, srcs, elu, dt):
    return _conv(orc, op, _prologue(*srcs, elu, orc.alpha, dt), dt)


def max_pad(op, T, causal):
    """The larger reflect pad of the layer at input length T (pad1d zero-extends inputs of T <= this before reflecting)."""
    import torch_oracle as TO
    if op.kind == "convtr":
        return 0
    pt = (op.k - 1) * op.dilation - (op.stride - 1)
    extra = TO.get_extra_padding_for_conv1d(T, op.k, op.stride, pt)
    return pt + extra if causal else max(pt - pt // 2, pt // 2 + extra)


WORST = {}


def _bars(got, ref64, ref32, normed, count, tag):
    d = (got.double() - ref64).abs()
    d32 = (ref32.double() - ref64).abs()
    e, e32 = float(d.max()), float(d32.max())
    r, r32 = float(d.pow(2).mean().sqrt()), float(d32.pow(2).mean().sqrt())
    scale = 1.0 if normed else max(1.0, float(ref64.pow(2).mean().sqrt()))
    old = (SMALL_GN_TOL if count < 4096 else LAYER_ABS_TOL) if normed else LAYER_ABS_TOL * scale
    assert e <= old, f"{tag}: max |gpu - f64| {e:.3e} above the absolute bar {old:.1e}"
    if not (normed and count < TINY_GN):
        assert e <= max(ABS_FLOOR * scale, ABS_K * e32), f"{tag}: max |gpu - f64| {e:.3e}, torch float32 {e32:.3e}"
        assert r <= max(RMS_FLOOR * scale, RMS_K * r32), f"{tag}: rms |gpu - f64| {r:.3e}, torch float32 {r32:.3e}"
    return e, e32, r, r32, scale


def _record(form_key, e, e32, r, r32, scale):
    w = WORST.setdefault(form_key, dict(max_gpu=0.0, max_t32=0.0, rms_gpu=0.0, rms_t32=0.0, max_ratio_above_floor=0.0, n=0))
    w["n"] += 1
    w["max_gpu"] = max(w["max_gpu"], e / scale)
    w["max_t32"] = max(w["max_t32"], e32 / scale)
    w["rms_gpu"] = max(w["rms_gpu"], r / scale)
    w["rms_t32"] = max(w["rms_t32"], r32 / scale)
    if e > 0.5 * ABS_FLOOR * scale:
        w["max_ratio_above_floor"] = max(w["max_ratio_above_floor"], e / max(e32, 1e-30))


def _form_name(L, form):
    dual, na0, _, elu, div = form
    return f"{L['side']}.{L['op'].role}" + (".div" if div else "") + (".2src" if dual else "") + (".aff" if na0 else "")


def run_case(m, orc, L, form, B, T, gen, tag="", invariants=False):
    """One layer call on the engine, in float64 and in float32 on the CPU; asserts shape and the bars.  With invariants: the same call
    again returns the same bits, and row 1 of a B >= 2 call equals a B = 1 call on that row bit for bit."""
    op = L["op"]
    dual, na0, na1, elu, use_div = form
    if orc.norm == "time_group_norm" and op.kind == "conv" and op.cout == 1 and T == 1:
        T = 2                                           # a GroupNorm of one element is undefined (the reference raises)
    x0 = torch.randn(B, op.cin, T, generator=gen)
    x1 = torch.randn(B, op.cin, T, generator=gen) if dual else None
    a0 = _affine(gen, B, op.cin) if na0 else None
    a1 = _affine(gen, B, op.cin) if (dual and na1) else None
    div = (0.05 + 2.0 * torch.rand(B, generator=gen, dtype=torch.float64)).float() if use_div else None
    cu = lambda t: None if t is None else t.cuda()
    call = lambda sl: m.engine.layer_forward(op.key, cu(x0[sl]), elu, aff0=cu(None if a0 is None else a0[sl]), div=cu(None if div is None else div[sl]),
                                             x1=cu(None if x1 is None else x1[sl]), aff1=cu(None if a1 is None else a1[sl]))
    got = call(slice(None)).cpu()
    srcs = (x0, a0, div, x1, a1)
    ref = reference(orc, op, srcs, elu, torch.float64)
    ref32 = reference(orc, op, srcs, elu, torch.float32)
    assert got.shape == ref.shape, (tag, op.key, got.shape, ref.shape)
    normed = orc.norm == "time_group_norm"
    count = ref[0].numel() if op.kind == "conv" else op.cout * (T + 1) * op.stride
    res = _bars(got, ref, ref32, normed, count, f"{tag} {op.key} form {form} B={B} T={T}")
    _record(_form_name(L, form), *res)
    if invariants:
        assert torch.equal(call(slice(None)).cpu(), got), (tag, op.key, "two identical calls differ")
        if B >= 2:
            assert torch.equal(call(slice(1, 2)).cpu()[0], got[1]), (tag, op.key, form, B, T, "row 1 of the batch differs from a B = 1 call")
    return res[0]


def _resblock_ref(orc, prefix, dil, srcs, dt):
    from funcodec_amd.plan import ConvOp
    x = _prologue(*srcs, False, orc.alpha, dt)
    y = _conv(orc, ConvOp("conv", prefix + ".block.1.conv", 0, 0, 0, 1, dilation=dil), F.elu(x, orc.alpha), dt)
    y = _conv(orc, ConvOp("conv", prefix + ".block.3.conv", 0, 0, 0, 1), F.elu(y, orc.alpha), dt)
    return _conv(orc, ConvOp("conv", prefix + ".shortcut.conv", 0, 0, 0, 1), x, dt) + y


def run_block(m, orc, L, B, T, gen, tag=""):
    """The whole residual block whose block.1 is L, on x0 n (j = 0) or x0 n + x1 n (j > 0), through the resblock hook."""
    op = L["op"]
    prefix = op.key[: -len(".block.1.conv")]
    n = orc.norm == "time_group_norm"
    dual = L["j"] > 0
    x0 = torch.randn(B, op.cin, T, generator=gen)
    x1 = torch.randn(B, op.cin, T, generator=gen) if dual else None
    a0 = _affine(gen, B, op.cin) if n else None
    a1 = _affine(gen, B, op.cin) if (dual and n) else None
    cu = lambda t: None if t is None else t.cuda()
    got = m.engine.resblock_forward(prefix, x0.cuda(), aff0=cu(a0), x1=cu(x1), aff1=cu(a1)).cpu()
    srcs = (x0, a0, None, x1, a1)
    ref = _resblock_ref(orc, prefix, op.dilation, srcs, torch.float64)
    ref32 = _resblock_ref(orc, prefix, op.dilation, srcs, torch.float32)
    assert got.shape == ref.shape
    # the sum of two GroupNorm'd branches: the older fused-head test's bar (twice the per-layer one)
    e, e32, r, r32, s = _bars(got, ref, ref32, n, 2 * op.cin * T if n else 1 << 30, f"{tag} block {prefix} two={dual} B={B} T={T}")
    _record(f"{L['side']}.resblock" + (".2src" if dual else ""), e, e32, r, r32, s)
    return e


def _long_T(L, T):
    op = L["op"]
    if op.cin >= WIDE:
        T = min(T, WIDE_T)
    if op.stride > 1 and op.kind == "conv" and T % op.stride == 0:
        T += 1                                          # a length the stride does not divide (and odd before the stride-2 layers)
    return T


@pytest.mark.parametrize("net", list(NETS))
def test_every_1d_layer_and_call_form_against_float64(net):
    """Every 1-D layer of the net in every call form, B = 1 at a short T (1, 2, 3, 5, 7: at or under most layers' pads) and B = 3 at a
    length around the 128 / 256 / 1024-column tiles; the thin residual blocks whole.  B = 3 calls also check that a repeated call returns
    the same bits and that row 1 equals a B = 1 call on it."""
    t0 = time.time()
    seed, (t_short, t_long) = NETS[net]
    m, orc = _parts(net)
    gen = torch.Generator().manual_seed(seed)
    for L in layer_table(m.arch):
        for form in call_forms(L, m.arch):
            run_case(m, orc, L, form, 1, t_short if L["op"].stride == 1 else t_short | 1, gen, net)
            run_case(m, orc, L, form, 3, _long_T(L, t_long), gen, net, invariants=True)
        if L["op"].role == "block1":
            run_block(m, orc, L, 1, t_short, gen, net)
            run_block(m, orc, L, 3, _long_T(L, t_long), gen, net)
    m.engine.check_status()
    from conftest import record_report
    record_report("layer1d_" + net, seconds=round(time.time() - t0, 1))


EDGE_NETS = ("tiny", "ds320", "ss320", "nf12st", "wnc16st")


@pytest.mark.parametrize("T", [1, 2, 3, 6, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025])
def test_1d_layer_edge_lengths(T):
    """Lengths at or under the reflect pads (T <= pad with a pending affine and ELU: pad1d zero-extends the ACTIVATED input, so the
    extension reads 0, not ELU(shift)), and around the 128 / 256 / 1024-column tiles; every layer and form of a GroupNorm net, a wide
    one, a causal weight_norm one and two synthetic ones.  T capped at 129 on layers of >= 512 input channels."""
    for net in EDGE_NETS:
        m, orc = _parts(net)
        gen = torch.Generator().manual_seed(1000 + T)
        for L in layer_table(m.arch):
            if L["op"].cin >= WIDE and T > WIDE_T:
                continue
            for form in call_forms(L, m.arch):
                run_case(m, orc, L, form, 1, T, gen, f"{net} T={T}")
            if L["op"].role == "block1" and T <= 257:
                run_block(m, orc, L, 2, T, gen, f"{net} T={T}")
        m.engine.check_status()


def test_1d_layer_at_its_own_pad_and_wide_batches():
    """Each layer at T = its own larger reflect pad and pad + 1 (the last zero-extended length and the first that is not), with the
    pending affine and the ELU of its call form; B = 16 at T = 33; the last decoder conv with >= 8192 output samples (the streaming
    conv_cout1_kernel as well as the rows form)."""
    hit = 0
    for net in ("tiny", "ds320", "ss320", "ss320nc", "nf24c4", "rh32k7", "wnc16st"):
        m, orc = _parts(net)
        gen = torch.Generator().manual_seed(77)
        for L in layer_table(m.arch):
            op = L["op"]
            pads = sorted({p for p in (max_pad(op, 1, orc.causal), max_pad(op, 2, orc.causal), max_pad(op, 3, orc.causal)) if p >= 1})
            for form in call_forms(L, m.arch):
                for T in sorted({t for p in pads for t in (p, p + 1)}):
                    if T <= max_pad(op, T, orc.causal) and (form[1] or form[2]) and form[3]:
                        hit += 1
                    run_case(m, orc, L, form, 2, T, gen, f"{net} pad")
                if net in ("tiny", "ds320"):
                    run_case(m, orc, L, form, 16, 33 if op.cin < WIDE else 9, gen, f"{net} B=16")
                if L["side"] == "dec" and op.role == "last":
                    for T in (8191, 8200, 12345):
                        run_case(m, orc, L, form, 2, T, gen, f"{net} long last conv", invariants=True)
        m.engine.check_status()
    assert hit >= 20, hit


def test_1d_layers_random_shape_sweep():
    """Seeded sweep over (net, layer, call form, B, T) of the nets above (PCG64 seed 2026, 80 draws)."""
    rng = np.random.Generator(np.random.PCG64(2026))
    lengths = [1, 2, 3, 4, 5, 7, 17, 63, 64, 65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2049]
    names = list(NETS)
    for draw in range(80):
        net = names[int(rng.integers(len(names)))]
        m, orc = _parts(net)
        tab = layer_table(m.arch)
        L = tab[int(rng.integers(len(tab)))]
        forms = call_forms(L, m.arch)
        form = forms[int(rng.integers(len(forms)))]
        T = lengths[int(rng.integers(len(lengths)))]
        if L["op"].cin >= WIDE:
            T = min(T, 65)
        B = int(rng.integers(1, 5))
        gen = torch.Generator().manual_seed(draw)
        run_case(m, orc, L, form, B, T, gen, f"draw {draw} {net}")


def _reach_classes():
    """The union of kernel classes the engine launches (fc_engine_profile) while every layer and call form of every net runs at T = 7
    (B = 1) and the last decoder conv at 8200 samples."""
    seen = set()
    for net in NETS:
        m, orc = _parts(net)
        gen = torch.Generator().manual_seed(5)
        m.engine.set_profiling(True)
        try:
            for L in layer_table(m.arch):
                for form in call_forms(L, m.arch):
                    run_case(m, orc, L, form, 1, 7, gen, f"reach {net}")
                    if L["side"] == "dec" and L["op"].role == "last":
                        run_case(m, orc, L, form, 1, 8200, gen, f"reach {net}")
                if L["op"].role == "block1":
                    run_block(m, orc, L, 1, 7, gen, f"reach {net}")
                prof = m.engine.read_profile()
                names = {p["kernel"] for p in prof if p["launches"] > 0}
                assert len(names) < 47, f"{net}: the profile's class table is full"
                seen |= names
        finally:
            m.engine.set_profiling(False)
        m.engine.check_status()
    return seen


def _mfma(BM, BN, WM, WN, forms):
    return {f"conv_mfma_kernel<{BM}, {BN}, {WM}, {WN}, {m}, {nu}, {str(row).lower()}, {str(qk).lower()}>" for m, nu, row, qk in forms}


# (MODE, NU, ROW, QK) per tile shape, as an MI355X run of this file launched them
WANT = (
    _mfma(128, 128, 2, 2, [
        (0, 1, True, True), (0, 2, False, True), (1, 1, True, True), (2, 1, True, True), (2, 12, True, True), (3, 1, True, True),
        (4, 12, True, True), (4, 3, False, True), (4, 9, False, False), (5, 2, False, True), (5, 3, False, True),
        (5, 4, False, True), (5, 5, False, True)])
    |     _mfma(64, 256, 1, 4, [
        (0, 1, True, True), (1, 1, True, True), (2, 1, True, True), (2, 2, True, True), (2, 4, False, True), (3, 1, True, True),
        (4, 1, True, True), (4, 12, True, True), (4, 3, False, True), (4, 9, False, False)])
    |     _mfma(32, 256, 1, 4, [
        (0, 1, True, True), (0, 12, True, True), (0, 2, True, True), (0, 5, False, False), (1, 1, True, True),
        (1, 12, True, True), (1, 2, True, True), (1, 4, False, True), (1, 5, False, False), (2, 1, True, True),
        (2, 11, True, True), (2, 12, True, True), (2, 2, False, True), (2, 2, True, True), (2, 3, False, True),
        (2, 4, False, True), (3, 1, True, True), (3, 12, True, True), (3, 2, False, True), (4, 1, True, True),
        (4, 12, True, True), (4, 3, False, True), (4, 9, False, False)])
    |     _mfma(32, 128, 1, 4, [
        (0, 1, True, True), (0, 2, True, True), (5, 3, False, True), (5, 4, False, True), (5, 5, False, True)])
    | {f"reshead_kernel<{c}, {k}, {d}>" for c in (32, 64) for k in (3, 5, 7) for d in ("false", "true")}
    | {f"{n}<{k}, true, 1>" for n in ("conv_fewout_rows_kernel", "conv_cout1_kernel") for k in (3, 5, 7)}
)


def test_conv_instantiations_are_reached():
    """Reachability from the dispatch itself: every family of conv_mfma_kernel, reshead_kernel and the few-output kernels."""
    seen = _reach_classes()
    from conftest import record_report
    record_report("layer1d_classes", seen=sorted(seen), worst_per_form=WORST)
    assert WANT <= seen, sorted(WANT - seen)
    tiles = {k.split(", ")[0][len("conv_mfma_kernel<"):] + "x" + k.split(", ")[1] for k in seen if k.startswith("conv_mfma_kernel<")}
    modes = {int(k.split(", ")[4]) for k in seen if k.startswith("conv_mfma_kernel<")}
    assert tiles == {"128x128", "64x256", "32x256", "32x128"} and modes == set(range(6)), (tiles, modes)
