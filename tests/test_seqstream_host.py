"""Host side of streaming a causal transformer net through a key / value cache (fc_seqstream_*, ``open_stream(..., max_frames=N)``):
the entry points, the refusals, the size of the state, and the chunked attention rule itself in float64."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from funcodec_amd import _lib
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.plan import encoder_plan
from funcodec_amd.stream import conv_layers, min_first, stream_refusal
from funcodec_amd.synth import make_state_dict
from test_seq_transformer_gpu import _ln, transformer_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQSTREAM_CALLS = {"fc_seqstream_state_bytes", "fc_seqstream_create", "fc_seqstream_forward"}
SCHEDULE = [7, 1, 1, 1, 6, 1, 15, 16, 17, 1, 33, 32]          # 131 frames; reaches positions 16, 17, 32, 48 and 65
LONG_SCHEDULE = [500, 500, 24, 1, 1, 1]


def causal_tinytf(C=None):
    """recipe tinytf made causal the way tests/test_seq_transformer_gpu.py::_block_engine does; C: the bottleneck width (4 n_filters)"""
    cfg = recipe_config("tinytf")
    for k in ("encoder_conf", "decoder_conf"):
        if C is not None:
            cfg[k]["n_filters"] = C // 4
        cfg[k].update(norm="weight_norm", causal=True)
        cfg[k].pop("norm_params", None)
    return cfg


def test_seqstream_calls_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    declared = {n for n in re.findall(r"\b(fc_seqstream_[a-z_0-9]+)\s*\(", hdr)}
    bound = {n for n in _lib.SYMBOLS if n.startswith("fc_seqstream_")}
    assert declared == bound == SEQSTREAM_CALLS
    lib = ctypes.CDLL(_lib.lib_path())
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in SEQSTREAM_CALLS:
        assert hasattr(lib, name), name
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, flat).group(1)
        assert len([p for p in params.split(",") if p.strip()]) == len(_lib.SYMBOLS[name][1]), name
    assert _lib.FC_ABI_VERSION == 7 and "#define FC_ABI_VERSION 7 " in hdr and _lib.load().fc_abi_version() == 7


def test_max_frames_opens_a_causal_transformer_net_and_nothing_else():
    tfc = arch_from_config(recipe_config("ss320tfc"))
    assert stream_refusal(tfc, max_frames=64) is None
    assert "seq_model: transformer" in stream_refusal(tfc)
    ss = arch_from_config(recipe_config("ss320"))
    for arch, key in [(arch_from_config(recipe_config("ds320")), "causal"),
                      (dataclasses.replace(ss, model_type="freq_codec"), "freq_codec"),
                      (dataclasses.replace(tfc, segment_dur=0.5), "model_conf.segment_dur"),
                      (dataclasses.replace(tfc, q0_ds_ratio=2), "quantizer_conf.q0_ds_ratio"),
                      (ss, "max_frames")]:
        assert key in stream_refusal(arch, max_frames=64), key
    samples, frames = min_first(tfc)
    need = max(samples // 320, frames)
    assert need > 1 and stream_refusal(tfc, max_frames=need) is None
    assert "max_frames" in stream_refusal(tfc, max_frames=need - 1)


def _r64(n):
    return (n + 63) // 64 * 64


def _expected_state_bytes(arch, B, F):
    """the documented layout (include/funcodec_amd.h): [scale B] [per conv with a left context a carry pair [2][B][cin][pt]],
    each rounded up to 64 floats; then, at a multiple of 64 floats, per side and per block K [B][C][F16] and V [B][C][F16]"""
    prefix = _r64(B) + sum(_r64(2 * B * L["cin"] * L["carry"]) for L in conv_layers(arch) if L["carry"] > 0)
    f16 = (F + 15) // 16 * 16
    return prefix * 4, (_r64(prefix) + 2 * arch.lstm_layers * 2 * B * arch.bottleneck_channels * f16) * 4


def test_state_size_is_the_documented_formula_and_the_prefix_is_unchanged():
    from funcodec_amd.engine import CodecEngine
    tiny = CodecEngine(arch_from_config(recipe_config("tiny")))
    assert tiny.lib.fc_seqstream_state_bytes(tiny._h, 2, 37) == 0
    plain = CodecEngine(arch_from_config(recipe_config("tinywn")))          # causal, but its bottleneck is an LSTM
    assert plain.lib.fc_seqstream_state_bytes(plain._h, 2, 37) == 0
    for cfg in (causal_tinytf(), recipe_config("ss320tfc")):
        arch = arch_from_config(cfg)
        eng = CodecEngine(arch)
        bare = CodecEngine(dataclasses.replace(arch, lstm_layers=0))       # the same convs without a sequence model: fc_stream_create's layout
        assert eng.lib.fc_stream_state_bytes(eng._h, 1) == 0                  # without the bound it goes on refusing
        for B in (1, 3):
            for F in (7, 37, 1500):
                prefix, total = _expected_state_bytes(arch, B, F)
                assert bare.lib.fc_stream_state_bytes(bare._h, B) == prefix, (B, F)
                assert eng.lib.fc_seqstream_state_bytes(eng._h, B, F) == total, (B, F)
        assert eng.lib.fc_seqstream_state_bytes(eng._h, 1, 0) == 0 and eng.lib.fc_seqstream_state_bytes(eng._h, 0, 7) == 0


def transformer_chunked_f64(x, sd, prefix, blocks, pushes, heads=4):
    """The rule of a session, restated: per block a K and a V cache; a push of n frames at position pos appends its K and V at
    [pos, pos + n) and its query i attends over keys 0 .. pos + i; LayerNorm, the Linears and the feed-forward run per frame on the
    chunk.  x [B, C, T] float64 -> after_norm(blocks(x)) [B, C, T] without the skip."""
    sd = {k: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith(prefix + ".")}
    B, C, T = x.shape
    dk = C // heads
    lin = lambda h, k: h @ sd[k + ".weight"].T + sd[k + ".bias"]
    kc = [torch.full((B, heads, T, dk), float("nan"), dtype=torch.float64) for _ in range(blocks)]     # never read before written
    vc = [torch.full((B, heads, T, dk), float("nan"), dtype=torch.float64) for _ in range(blocks)]
    out, pos = [], 0
    for n in pushes:
        xs = x[:, :, pos:pos + n].double().permute(0, 2, 1)
        for l in range(blocks):
            p = f"{prefix}.encoders.{l}"
            h = _ln(xs, sd, p + ".norm1")
            q, k, v = (lin(h, f"{p}.self_attn.linear_{w}").view(B, n, heads, dk).transpose(1, 2) for w in "qkv")
            kc[l][:, :, pos:pos + n], vc[l][:, :, pos:pos + n] = k, v
            ctx = torch.empty(B, heads, n, dk, dtype=torch.float64)
            for i in range(n):
                s = q[:, :, i:i + 1] @ kc[l][:, :, :pos + i + 1].transpose(-2, -1) / np.sqrt(dk)
                ctx[:, :, i:i + 1] = torch.softmax(s, -1) @ vc[l][:, :, :pos + i + 1]
            xs = xs + lin(ctx.transpose(1, 2).reshape(B, n, C), f"{p}.self_attn.linear_out")
            h = _ln(xs, sd, p + ".norm2")
            xs = xs + lin(torch.relu(lin(h, f"{p}.feed_forward.w_1")), f"{p}.feed_forward.w_2")
        out.append(_ln(xs, sd, prefix + ".after_norm").permute(0, 2, 1))
        pos += n
    assert pos == T
    return torch.cat(out, -1)


@pytest.mark.parametrize("pushes", [SCHEDULE, LONG_SCHEDULE, [131], [1] * 40], ids=["schedule", "long", "single", "frames1"])
def test_the_chunked_rule_equals_the_whole_sequence_in_float64(pushes):
    arch = arch_from_config(causal_tinytf(64))
    sd = make_state_dict(arch, 164)
    prefix = [op.key for op in encoder_plan(arch) if op.kind == "transformer"][0]
    T = sum(pushes)
    x = torch.randn(2, 64, T, generator=torch.Generator().manual_seed(T), dtype=torch.float64)
    whole = transformer_f64(x, sd, prefix, arch.lstm_layers, True, False)
    got = transformer_chunked_f64(x, sd, prefix, arch.lstm_layers, pushes)
    err = float((got - whole).abs().max())
    assert err < 1e-12, err                     # float64 rounding only: the values are O(1) after after_norm
