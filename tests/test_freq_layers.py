"""Per-layer parity of the STFT-domain codec (FreqCodec, model_type 1) against a float64 CPU reference.

Every 2-D layer runs through `Engine.layer2d_forward` (fc_layer2d_forward), which copies the inputs into the engine's frequency-major
layout with reflected halo rows and then calls the same run_conv2d / run_convtr2d as the encode and decode drivers, so the kernel that
runs is the one the product picks for that layer and shape.  The reference is oracle/freq_oracle.py's sconv2d / sconvtr2d with the state
dict, the inputs and the affines cast to double, and the affine, the sum and the ELU applied in double before the conv.

Call forms (run_encoder_2d / run_resblocks2d / run_decoder_2d):
  first conv      raw x0, no affine, no ELU                       out_halo = engine halo
  shortcut        x0 (block j = 0) or x0 + x1 (j > 0), normed     out_halo = engine halo
  block.1         the same sources, ELU                           out_halo = 0
  block.3         one normed source, ELU                          out_halo = engine halo
  encoder down    x0 + x1 normed, ELU                             halo, 0 at the last stage
  decoder convtr  x0 (+ x1: the LSTM skip at stage 0, else shortcut + block), ELU, halo
  last conv       x0 + x1 normed, ELU                             out_halo = 0
The weight_norm nets take the same forms without affines.

Kernel branches, as run_conv2d / run_convtr2d / launch_gconv2d / launch_gconvtr2d dispatch them:
  * gconv2d_kernel (pack_conv2d sets w_group when groups > 1 and gconv2d_ok(cpg, opg, kf, kt, st)).  With conv_group_ratio 1 the nets
    give (cpg, opg) = (2, 2) for 1 x 1 shortcuts, (2, 4) for 1 x 1 block.3 convs, (4, 2) for 3 x 3 block.1 convs, (2, 4) for the 8 x 2
    strided convs (tinyfreqgr1, freqmpgr1) and the 8 x 4 time-stride-2 convs (tinyfreq640gr1).  Other (cpg, opg) x shape pairs are not
    produced by the group-ratio formulas.  Two sources (DUAL): the shortcut (2, 2) and block.1 (4, 2) of block j = 1 in the nets with two
    residual blocks (tinyfreqgr1res2, tinyfreqgr1wncres2); block.3 always has one source.  The two-source strided layers are materialised
    by combine2d first (FC_GCONV_MAT: kf >= 4 and two sources) and then run the single-source kernel.  The hook refuses a second source for
    a layer the plan gives one (its staging is sized for one).
  * its gather instantiation (NEEDMASK): T <= the time pad (T = 1 symmetric, T <= 2 causal), for one and two sources of the 3 x 3 layers.
    The 1 x 1 layers have no time pad and their sources always lie in the workspace, so they only take the unmasked form.
  * FO = 2 rows per lane (3 x 3 layers) with odd Fo (F = 257 on the tiny nets, F = 65 on freqfuzz54).  Fo = 1 (the 3 x 3 layers of
    tinyfreqgr1f1 at F = 1) dispatches FO = 1 (gconv2d_fo: at most Fo rows per lane), behind the F <= pad materialisation.
  * halo written by the kernel (Fo > halo) and by halo_rows (Fo <= halo: F = 1 with halo 3, F = 1, 4 with halo 4).
  * the dual-source strided layers materialised first (FC_GCONV_MAT: kf >= 4 and two sources).
  * with statistics (GroupNorm) and without (weight_norm).
  * gconvtr2d_kernel<1> / <2> (time ratio 1 / 2), channel splits cs = 1, 2, 4 (B = 96, 48, <= 32 at Fin = 64), fr = 1 (tinyfreqgr1f1);
    the last stage with last_out_padding; causal time trims.
  * the dense implicit-GEMM path (freqmp, tinyfreq, freqmpgr8, freqfuzz10 / freqfuzz16 with frequency ratio 8 = 16-row kernels): the 7 x 7
    first conv over 3 channels, the few-output last conv (3 channels; 2 for tinyfreqang), layers with >= 3 M tiles (materialisation),
    the block-diagonal grouped GEMM of grouped layers the direct kernels do not take (freqmpgr8, freqfuzz16), and the per-phase
    transposed GEMMs with their store_lo / store_hi windows.
  * the F <= pad case: the f1 nets (frequency ratio 1) run 3 x 3 and 2 x 2 layers on F = 1 rows, where pad2d zero-extends; dense
    (tinyfreqf1, tinyfreqf1wn) and grouped (tinyfreqgr1f1).

Halo rows: every returned halo row a next layer with pad p <= out_halo reads is checked bit-identical to the interior row it mirrors.  Where
Fo <= p the next layer reads no halo row: run_conv2d rebuilds such an input with pad2d's zero-extended rows (the F <= pad tests check that).

Tolerances (the 1-D bars, tests/test_gpu_parity.py): max abs error <= 5e-5 on GroupNorm'd outputs, 2e-4 where the GroupNorm runs over
fewer than 4096 elements; weight_norm outputs <= 5e-5 x max(1, RMS of the reference).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LAYER_ABS_TOL = 5e-5
SMALL_GN_TOL = 2e-4


# ---- the nets and their 2-D layers -----------------------------------------------------------------------------------------------
def _res2(name):
    """A recipe with n_residual_layers 2 (dilation_base 1): shortcut and block.1 of block j = 1 take two summed sources."""
    from funcodec_amd.config import freq_recipe_config
    cfg = freq_recipe_config(name)
    for side in ("encoder_conf", "decoder_conf"):
        cfg[side] = dict(cfg[side], n_residual_layers=2, dilation_base=1)
    return cfg


def _fuzz_hop24():
    from funcodec_amd.config import fuzz_freq_recipe_config
    cfg = fuzz_freq_recipe_config(16)                      # n_fft 64, frequency ratios 8, 4, grouped
    cfg["model_conf"]["domain_conf"] = dict(cfg["model_conf"]["domain_conf"], hop_length=24)
    tot = 24
    for _, t in cfg["encoder_conf"]["ratios"]:
        tot *= t
    cfg["quantizer_conf"]["encoder_hop_length"] = tot
    return cfg


# nets that are not named recipes: config builders
CONFIGS = {
    "tinyfreqgr1res2": lambda: _res2("tinyfreqgr1"),
    "tinyfreqgr1wncres2": lambda: _res2("tinyfreqgr1wnc"),
    "fuzz64hop24": _fuzz_hop24,
}


def _freq_parts(cfg_name, seed):
    """(engine, oracle) of a named recipe or of a CONFIGS net."""
    if cfg_name not in CONFIGS:
        from helpers import freq_engine_for, freq_oracle_for
        return freq_engine_for(cfg_name, seed), freq_oracle_for(cfg_name, seed)
    return _config_parts(cfg_name, seed)


@functools.lru_cache(maxsize=2)
def _config_parts(cfg_name, seed):
    cfg = CONFIGS[cfg_name]()
    from freq_oracle import FreqOracle
    from funcodec_amd.config import arch_from_config
    from funcodec_amd.model import EncodecMI355X
    from funcodec_amd.synth import make_freq_state_dict
    sd = {k: torch.from_numpy(v) for k, v in make_freq_state_dict(cfg, seed).items()}
    m = EncodecMI355X(arch_from_config(cfg), "cuda:0")
    m.load_state_dict(sd)
    return m, FreqOracle(cfg, sd)


def layer_table(orc):
    """Every 2-D layer of the oracle's nets in execution order: dict(prefix, kind, F (input rows), C, stride, dil, stage, last, j),
    walking the Sequential indices as FreqOracle.encoder2d / decoder2d do."""
    out = []
    Fq = orc.n_fft // 2 + 1
    nf, n = orc.n_filters, len(orc.ratios2d)
    out.append(dict(prefix="encoder.model.0.conv", kind="first", F=Fq, C=orc.in_ch, stride=(1, 1), dil=(1, 1)))
    idx, c = 1, nf
    for s, (fr, tr) in enumerate(reversed(orc.ratios2d)):
        for j in range(orc.n_res):
            p = f"encoder.model.{idx}"
            out.append(dict(prefix=p + ".shortcut.conv", kind="shortcut", F=Fq, C=c, stride=(1, 1), dil=(1, 1), j=j))
            out.append(dict(prefix=p + ".block.1.conv", kind="block1", F=Fq, C=c, stride=(1, 1), dil=(1, orc.dil_base ** j), j=j))
            out.append(dict(prefix=p + ".block.3.conv", kind="block3", F=Fq, C=c // orc.compress, stride=(1, 1), dil=(1, 1), j=j))
            idx += 1
        idx += 1
        out.append(dict(prefix=f"encoder.model.{idx}.conv", kind="down", F=Fq, C=c, stride=(fr, tr), dil=(1, 1), last=s == n - 1))
        Fq = (Fq + fr - 2 * fr) // fr + 1
        c *= 2
        idx += 1
    idx = 1 + (1 if orc.lstm_layers > 0 else 0) + 1
    Fq = 1
    for s, (fr, tr) in enumerate(orc.ratios2d):
        idx += 1
        last = s == n - 1
        out.append(dict(prefix=f"decoder.model.{idx}.convtr", kind="up", F=Fq, C=c, stride=(fr, tr), dil=(1, 1), stage=s, last=last))
        f_r = fr // 2
        f_l = fr - f_r
        if last:
            f_r = max(f_r - 1, 0)
        Fq = (Fq + 1) * fr - f_l - f_r
        c //= 2
        idx += 1
        for j in range(orc.n_res):
            p = f"decoder.model.{idx}"
            out.append(dict(prefix=p + ".shortcut.conv", kind="shortcut", F=Fq, C=c, stride=(1, 1), dil=(1, 1), j=j))
            out.append(dict(prefix=p + ".block.1.conv", kind="block1", F=Fq, C=c, stride=(1, 1), dil=(1, orc.dil_base ** j), j=j))
            out.append(dict(prefix=p + ".block.3.conv", kind="block3", F=Fq, C=c // orc.compress, stride=(1, 1), dil=(1, 1), j=j))
            idx += 1
    idx += 1
    out.append(dict(prefix=f"decoder.model.{idx}.conv", kind="last", F=Fq, C=nf, stride=(1, 1), dil=(1, 1)))
    return out


def call_forms(L, normed, lstm_skip):
    """The (two sources?, affine on x0?, affine on x1?, ELU, out_halo is the engine halo?) forms the drivers use for layer L."""
    k = L["kind"]
    if k == "first":
        return [(False, False, False, False, True)]
    if k in ("shortcut", "block1"):
        elu, halo = k == "block1", k == "shortcut"
        return [(True, normed, normed, elu, halo)] if L["j"] > 0 else [(False, normed, False, elu, halo)]
    if k == "block3":
        return [(False, normed, False, True, True)]
    if k == "down":
        return [(True, normed, normed, True, not L["last"])]
    if k == "up":
        if L["stage"] == 0:
            return [(True, False, normed, True, True)] if lstm_skip else [(False, False, False, True, True)]
        return [(True, normed, normed, True, True)]
    return [(True, normed, normed, True, False)]          # last conv


def _skip(m):
    return m.arch.lstm_layers > 0 and bool(m.arch.lstm_skip)


def _affine(gen, B, C):
    return torch.stack([0.5 + torch.rand(B, C, generator=gen, dtype=torch.float64),
                        0.5 * torch.randn(B, C, generator=gen, dtype=torch.float64)], -1).float()


def reference(orc, L, x0, a0, x1, a1, elu):
    """float64 CPU restatement of the layer on act(a0(x0) + a1(x1))."""
    def app(x, a):
        x = x.double()
        return x if a is None else x * a[..., 0, None, None].double() + a[..., 1, None, None].double()
    v = app(x0, a0)
    if x1 is not None:
        v = v + app(x1, a1)
    if elu:
        v = F.elu(v, alpha=float(getattr(orc, "alpha", 1.0)))
    w, b, g, be = (None if t is None else t.double() for t in orc._p(L["prefix"]))
    from freq_oracle import sconv2d, sconvtr2d
    if L["kind"] == "up":
        op = orc.last_out_padding if L["last"] else ((0, 0), (0, 0))
        return sconvtr2d(v, w, b, g, be, L["stride"], orc.eps, op, orc.causal)
    return sconv2d(v, w, b, g, be, L["stride"], orc.eps, L["dil"], orc.causal)


def run_case(m, orc, L, form, B, T, gen, halo, tag=""):
    """One layer call on the engine and in float64; asserts shape, accuracy and the halo rows.  Returns the max abs error."""
    dual, na0, na1, elu, with_halo = form
    C, Fq = L["C"], L["F"]
    x0 = torch.randn(B, C, Fq, T, generator=gen)
    x1 = torch.randn(B, C, Fq, T, generator=gen) if dual else None
    a0 = _affine(gen, B, C) if na0 else None
    a1 = _affine(gen, B, C) if (dual and na1) else None
    oh = halo if with_halo else 0
    got = m.engine.layer2d_forward(L["prefix"], x0.cuda(), None if a0 is None else a0.cuda(), None if x1 is None else x1.cuda(),
                                   None if a1 is None else a1.cuda(), apply_elu=elu, out_halo=oh).cpu()
    ref = reference(orc, L, x0, a0, x1, a1, elu)
    Fo = ref.shape[2]
    assert got.shape == (ref.shape[0], ref.shape[1], Fo + 2 * oh, ref.shape[3]), (tag, L["prefix"], got.shape, ref.shape)
    inner = got[:, :, oh:oh + Fo]
    err = float((inner.double() - ref).abs().max())
    if orc.norm == "time_group_norm":
        # the GroupNorm's element count: the (untrimmed, for a transposed conv) output of one utterance
        count = ref[0].numel()
        if L["kind"] == "up":
            fr, tr = L["stride"]
            count = ref.shape[1] * (L["F"] + 1) * fr * (T + 1) * tr
        tol = SMALL_GN_TOL if count < 4096 else LAYER_ABS_TOL
    else:
        tol = LAYER_ABS_TOL * max(1.0, float(ref.pow(2).mean().sqrt()))
    assert err <= tol, (tag, L["prefix"], form, B, Fq, T, err, tol)
    # halo rows: every row a next layer with pad p <= out_halo reads is the interior row it mirrors, bit for bit.  With Fo <= p the
    # next layer does not read them (run_conv2d materialises its activated input with pad2d's zero-extended rows instead)
    for i in range(1, oh + 1):
        if i < Fo:
            assert torch.equal(got[:, :, oh - i], got[:, :, oh + i]), (tag, L["prefix"], "top halo row", i)
            assert torch.equal(got[:, :, oh + Fo - 1 + i], got[:, :, oh + Fo - 1 - i]), (tag, L["prefix"], "bottom halo row", i)
    return err


NETS = {
    # name: (seed, T values per layer of width <= 16 / wider layers)
    "tinyfreq": (7, (5, 203)),
    "tinyfreqgr1": (8, (7, 1025)),
    "tinyfreq640gr1": (9, (2, 1024)),
    "tinyfreqang": (10, (3, 64)),
    "tinyfreqwn": (11, (1, 130)),
    "tinyfreqwnc": (12, (2, 99)),
    "tinyfreqgr1wnc": (13, (1, 1023)),
    "tinyfreqf1": (14, (3, 77)),
    "tinyfreqf1wn": (15, (2, 33)),
    "freqmpgr1": (16, (3, 40)),
    "freqmp": (17, (2, 9)),
    "freqmpgr8": (18, (5, 12)),
    "freqfuzz10": (10, (1, 301)),
    "freqfuzz16": (16, (2, 257)),
    "freqfuzz54": (54, (3, 130)),
    "tinyfreqgr1f1": (19, (1, 300)),
    "tinyfreqgr1res2": (20, (1, 1025)),
    "tinyfreqgr1wncres2": (21, (2, 1023)),
}


@pytest.mark.parametrize("net", list(NETS))
def test_every_2d_layer_and_call_form_against_float64(net):
    """Every 2-D layer of the net in every call form the drivers use, at its own frequency rows, B in {1, 3}, a short T and a longer one
    (the longer one only where channels x rows are small: largest reference tensor ~ 3 x 16 x 257 x 1025 doubles on the tiny nets, 3 x 64 x
    257 x 40 on freqmpgr1, 3 x 512 x 5 x 9 on freqmp)."""
    seed, (t_short, t_long) = NETS[net]
    m, orc = _freq_parts(net, seed)
    halo = m.engine.freq_halo()
    gen = torch.Generator().manual_seed(seed)
    worst = {}
    normed = orc.norm == "time_group_norm"
    for L in layer_table(orc):
        for form in call_forms(L, normed, _skip(m)):
            for B, T in ((1, t_short), (3, t_long if L["C"] * L["F"] <= 16 * 257 else t_short)):
                if L["stride"][1] == 2 and T > 1 and L["kind"] == "down":
                    T = T | 1 if B == 1 else T & ~1 or 2        # odd and even T before the time-stride-2 layers
                err = run_case(m, orc, L, form, B, T, gen, halo, net)
                key = L["kind"]
                worst[key] = max(worst.get(key, 0.0), err)
    m.engine.check_status()
    from conftest import record_report
    record_report("layer2d_" + net, **{k: float(f"{v:.3g}") for k, v in worst.items()})


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7, 1023, 1024, 1025, 2049])
def test_2d_layer_edge_lengths(T):
    """Lengths shorter than the time pad (the gather instantiation), not a multiple of 4, and around the 1024-column tiles of the direct
    kernels: one net with grouped direct kernels, one dense, one causal weight_norm.  Largest reference tensor 1 x 16 x 257 x 2049 doubles."""
    for net in ("tinyfreqgr1", "tinyfreq", "tinyfreqgr1wnc"):
        seed = NETS[net][0]
        m, orc = _freq_parts(net, seed)
        halo = m.engine.freq_halo()
        gen = torch.Generator().manual_seed(1000 + T)
        normed = orc.norm == "time_group_norm"
        for L in layer_table(orc):
            if T > 256 and L["C"] * L["F"] > 16 * 257:
                continue
            for form in call_forms(L, normed, _skip(m)):
                run_case(m, orc, L, form, 1, T, gen, halo, f"{net} T={T}")


def test_direct_kernel_instantiations_are_reached():
    """Reachability from the dispatch itself: the engine's per-launch kernel classes (fc_engine_profile) while every layer and call form of
    the grouped nets runs.  gconv2d_kernel<CPG, OPG, KF, KT, ST, DUAL>: the 1 x 1 and 3 x 3 layers with one and two sources, the strided
    8 x 2 / 8 x 4 layers with one (their two-source calls are materialised first, so no two-source strided class may appear)."""
    want = {"gconv2d_kernel<2, 2, 1, 1, 1, false>", "gconv2d_kernel<2, 2, 1, 1, 1, true>", "gconv2d_kernel<4, 2, 3, 3, 1, false>",
            "gconv2d_kernel<4, 2, 3, 3, 1, true>", "gconv2d_kernel<2, 4, 1, 1, 1, false>", "gconv2d_kernel<2, 4, 8, 2, 1, false>",
            "gconv2d_kernel<2, 4, 8, 4, 2, false>", "gconvtr2d_kernel<1>", "gconvtr2d_kernel<2>"}
    seen = set()
    for net in ("tinyfreqgr1res2", "tinyfreq640gr1"):
        m, orc = _freq_parts(net, NETS[net][0])
        halo = m.engine.freq_halo()
        gen = torch.Generator().manual_seed(5)
        normed = orc.norm == "time_group_norm"
        m.engine.set_profiling(True)
        try:
            for L in layer_table(orc):
                for form in call_forms(L, normed, _skip(m)):
                    for T in (1, 7):
                        run_case(m, orc, L, form, 1, T, gen, halo, f"reach {net}")
            seen |= {p["kernel"] for p in m.engine.read_profile() if p["launches"] > 0}
        finally:
            m.engine.set_profiling(False)
    assert want <= seen, sorted(want - seen)
    assert not any(k.startswith("gconv2d_kernel<") and (", 8, 2, 1, true>" in k or ", 8, 4, 2, true>" in k) for k in seen), sorted(seen)


def _gconvtr_cs(Fin, T, B, fr, tr, cout):
    """The output-channel split launch_gconvtr2d (freq_kernels.hip) picks: doubled while <= fr, <= cout and nx (Fin + 1) B cs < 6144."""
    nx, cs = -(-(T + 1) * tr // 1024), 1
    while cs * 2 <= fr and cs * 2 <= cout and nx * (Fin + 1) * B * cs < 6144:
        cs *= 2
    return cs


def test_2d_layer_grid_z_extent_and_channel_split():
    """B = 32 at F = 257 (B x ceil(Fo / FO) workgroup rows on the grid's z axis) for the stage-0 layers of a grouped net and the last
    decoder stage, and the last decoder convtr (Fin = 64) at B = 96, 48, 1: channel splits cs = 1, 2, 4.  Largest reference tensor
    96 x 8 x 257 x 3 doubles."""
    m, orc = _freq_parts("tinyfreqgr1", 8)
    halo = m.engine.freq_halo()
    gen = torch.Generator().manual_seed(32)
    normed = orc.norm == "time_group_norm"
    tab = layer_table(orc)
    up = tab[-5]
    assert up["kind"] == "up" and up["F"] == 64
    for L in tab[:4] + tab[-4:]:
        for form in call_forms(L, normed, True):
            run_case(m, orc, L, form, 32, 3, gen, halo, "z-extent")
    fr, tr = up["stride"]
    splits = set()
    for B in (96, 48, 1):
        splits.add(_gconvtr_cs(up["F"], 3, B, fr, tr, up["C"] // 2))
        for form in call_forms(up, normed, True):
            run_case(m, orc, up, form, B, 3, gen, halo, f"channel split B={B}")
    assert splits == {1, 2, 4}


def test_2d_layers_random_shape_sweep():
    """Seeded sweep over (net, layer, call form, B, T) of the nets above (PCG64 seed 2025, 60 draws)."""
    rng = np.random.Generator(np.random.PCG64(2025))
    lengths = [1, 2, 3, 5, 7, 17, 63, 64, 65, 127, 255, 511, 1023, 1024, 1025]
    names = list(NETS)
    for draw in range(60):
        net = names[int(rng.integers(len(names)))]
        m, orc = _freq_parts(net, NETS[net][0])
        halo = m.engine.freq_halo()
        tab = layer_table(orc)
        L = tab[int(rng.integers(len(tab)))]
        forms = call_forms(L, orc.norm == "time_group_norm", _skip(m))
        form = forms[int(rng.integers(len(forms)))]
        T = lengths[int(rng.integers(len(lengths)))]
        if L["C"] * L["F"] > 16 * 257:
            T = min(T, 17)                                    # keep the float64 reference cheap on the wide layers
        B = int(rng.integers(1, 4))
        gen = torch.Generator().manual_seed(draw)
        run_case(m, orc, L, form, B, T, gen, halo, f"draw {draw} {net}")


@pytest.mark.parametrize("net,seed", [("tinyfreqf1", 21), ("tinyfreqf1wn", 22), ("tinyfreqgr1f1", 23)])
def test_frequency_ratio_1_layers_at_F_1(net, seed):
    """F = 1 inputs of 3 x 3 and 2 x 2 layers: pad2d zero-extends the ACTIVATED input before reflecting (conv.py:100-119), so the halo rows
    read as 0, not as the activation of a raw zero row (ELU(shift), ELU(shift0 + shift1))."""
    m, orc = _freq_parts(net, seed)
    halo = m.engine.freq_halo()
    gen = torch.Generator().manual_seed(seed)
    normed = orc.norm == "time_group_norm"
    hit = 0
    for L in layer_table(orc):
        if L["F"] != 1 or L["kind"] == "up":
            continue
        for form in call_forms(L, normed, _skip(m)):
            for T in (1, 6, 301):
                run_case(m, orc, L, form, 2, T, gen, halo, net)
                hit += 1
    assert hit >= 8


@pytest.mark.parametrize("net,seed,B,T", [("tinyfreqf1", 31, 2, 2900), ("tinyfreqf1wn", 32, 1, 1777), ("tinyfreqgr1f1", 33, 1, 2222)])
def test_frequency_ratio_1_net_against_oracle(net, seed, B, T):
    """End to end like test_freq_codec_against_oracle_fresh_inputs, on the nets whose bottleneck runs at F = 1."""
    from helpers import audio, index_report, rms
    m, orc = _freq_parts(net, seed)
    wav = audio(B, T, 5000 + T, "tones")
    o = orc.inference(wav, bit_width=None, use_scale=True)
    ret = m.inference(wav.cuda().unsqueeze(1), bit_width=None, use_scale=True)
    m.engine.check_status()
    assert ret["recon_speech"].shape == o["recon_speech"].shape
    enc_err = rms(m.engine.encode(wav.cuda(), 1, want_enc_out=True)["enc_out"], o["encoder_out"])
    assert enc_err < 1e-4 * max(1.0, float(o["encoder_out"].double().pow(2).mean().sqrt())), enc_err
    rep = index_report(ret["code_indices"][0], o["code_indices"][0])
    if rep["frames_bad"]:
        from test_gpu_parity import _assert_flips_are_near_ties
        _assert_flips_are_near_ties(orc.embed, o["encoder_out"], o["code_indices"][0], ret["code_indices"][0], max_frames=1)
        return
    ref_rms = float(o["recon_speech"].double().pow(2).mean().sqrt())
    assert rms(ret["recon_speech"], o["recon_speech"]) < 1e-3 * ref_rms


@pytest.mark.parametrize("net,T", [("tinyfreq", 257), ("tinyfreq", 1001), ("freqmp", 4801), ("fuzz64hop24", 33), ("fuzz64hop24", 999)])
def test_stft_features_mag_phase_against_float64_stft(net, T):
    """The engine's mag_phase feature tensor (log-magnitude, phase re, phase im; codec_freq.py:366-379) against torch.stft in float64:
    T = n_fft / 2 + 1 (the shortest accepted), odd T, a hop (24) that does not divide n_fft (64)."""
    from freq_oracle import spectrogram
    from helpers import audio
    m, orc = _freq_parts(net, NETS[net][0] if net in NETS else 16)
    assert T >= orc.n_fft // 2 + 1
    B = 2
    wav = audio(B, T, 6000 + T, "tones")
    x = wav.double()
    if orc.audio_normalize:
        x = x / (1e-8 + x.pow(2).mean(dim=1, keepdim=True).sqrt())
    xc = spectrogram(x, orc.n_fft, orc.stft_hop)
    mag = xc.abs()
    ref_log = torch.log(torch.clamp(mag, min=1e-6))
    ph = xc / torch.clamp(mag, min=1e-6)
    cap = torch.zeros((B, 3, orc.n_fft // 2 + 1, 1 + T // orc.stft_hop), dtype=torch.float32, device="cuda")
    m.engine.debug_freq_features(cap, 1)
    m.engine.encode(wav.cuda(), 1)
    torch.cuda.synchronize()
    got = cap.cpu().double()
    top = float(mag.max())
    assert float((got[:, 0].exp() - ref_log.exp()).abs().max()) < 2e-5 * top
    for c, part in ((1, ph.real), (2, ph.imag)):
        assert float(((got[:, c] - part).abs() * mag).max()) < 2e-5 * top, c


def test_layer_forward_refuses_2d_layers_and_wrong_channel_counts():
    """fc_layer_forward runs 1-D layers only: a 2-D prefix is refused on the host before any launch (it used to be run as a conv over
    kf x C channels, reading kf times the input); Engine.layer_forward checks the input's channel count."""
    import ctypes as C
    from helpers import engine_for
    from funcodec_amd.engine import EngineError
    m, _ = _freq_parts("tinyfreq", 7)
    x = torch.zeros(1, 4, 16, device="cuda")
    with pytest.raises(EngineError, match="2-D layer of the STFT-domain codec: use layer2d_forward"):
        m.engine.layer_forward("encoder.model.1.block.1.conv", x)
    eng = m.engine
    y = torch.zeros(1, 64, 16, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    rc = eng.lib.fc_layer_forward(eng._h, b"encoder.model.1.block.1.conv", C.c_void_p(x.data_ptr()), 1, 16, 0, C.c_void_p(y.data_ptr()),
                                  C.c_void_p(ws.data_ptr()), ws.numel(), eng._stream())
    assert rc != 0 and "use fc_layer2d_forward" in eng.lib.fc_last_error().decode()
    with pytest.raises(EngineError, match="1-D layer: use fc_layer_forward"):
        eng.layer2d_forward("encoder.model.16.conv", torch.zeros(1, 64, 1, 4, device="cuda"))
    with pytest.raises(EngineError, match="expected input"):
        eng.layer2d_forward("encoder.model.1.block.1.conv", torch.zeros(1, 5, 257, 4, device="cuda"))
    t = engine_for("tiny", 7)
    with pytest.raises(EngineError, match="expected input"):
        t.engine.layer_forward("encoder.model.1.block.1.conv", torch.zeros(1, 5, 16, device="cuda"))
