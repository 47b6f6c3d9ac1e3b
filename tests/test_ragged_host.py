"""Length-aware (ragged) batches, host side: the new C entry points and their ctypes bindings, the refusals, and the per-row padding
rules of the staging pass restated in Python and checked in float64 torch against the reference's layers on every row alone
(oracle/torch_oracle.py sconv1d / sconvtr1d).  No GPU."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

from funcodec_amd import _lib
from funcodec_amd.config import arch_from_config, freq_recipe_config, recipe_config
from funcodec_amd.engine import ragged_refusal
from funcodec_amd.plan import decoder_plan, encoder_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from torch_oracle import sconv1d, sconvtr1d  # noqa: E402

RAGGED = ["fc_ragged_workspace_bytes", "fc_encode_ragged", "fc_decode_emb_ragged", "fc_decode_codes_ragged", "fc_encode_decode_ragged"]


def test_ragged_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.lib_path())
    for name in RAGGED:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/funcodec_amd.h"
        n_params = len([p for p in m.group(1).split(",") if p.strip()])
        assert name in _lib.SYMBOLS, name
        assert len(_lib.SYMBOLS[name][1]) == n_params, (name, n_params, len(_lib.SYMBOLS[name][1]))
        assert hasattr(lib, name), f"{name} not exported"
        assert not name.startswith("fc_stream_")
    assert _lib.FC_ABI_VERSION == 7 and _lib.load().fc_abi_version() == 7
    # the signatures are those of the offline siblings plus the lengths
    for rag, off in [("fc_encode_ragged", "fc_encode"), ("fc_decode_emb_ragged", "fc_decode_emb"), ("fc_decode_codes_ragged", "fc_decode_codes"),
                     ("fc_encode_decode_ragged", "fc_encode_decode"), ("fc_ragged_workspace_bytes", "fc_engine_workspace_bytes")]:
        extra = 0 if rag == "fc_ragged_workspace_bytes" else 1
        assert len(_lib.SYMBOLS[rag][1]) == len(_lib.SYMBOLS[off][1]) + extra, rag
        assert _lib.SYMBOLS[rag][0] == _lib.SYMBOLS[off][0]


def test_host_calls_take_the_length_keywords():
    import inspect
    from funcodec_amd.bin.codec_inference import Speech2Token, get_parser
    from funcodec_amd.model import EncodecMI355X
    for fn, kw in [(EncodecMI355X.inference, "speech_lengths"), (EncodecMI355X.inference_encoding, "speech_lengths"),
                   (EncodecMI355X.inference_decoding, "token_lengths"), (EncodecMI355X.inference_decoding_emb, "token_lengths"),
                   (Speech2Token.__call__, "speech_lengths")]:
        p = inspect.signature(getattr(fn, "__wrapped__", fn)).parameters
        assert kw in p and p[kw].default is None, (fn, kw)
    args = get_parser().parse_args(["--length_aware", "true"])
    assert args.length_aware is True and get_parser().parse_args([]).length_aware is False


def test_ragged_refusal_names_the_key():
    for name in ["ds320", "ds640", "ds320wn", "ss320", "ss320nc", "tiny", "tinywn", "tinyst", "ds320cd64"]:
        assert ragged_refusal(arch_from_config(recipe_config(name))) is None, name
    assert "freq_codec" in ragged_refusal(arch_from_config(freq_recipe_config("freqmp")))
    assert "seq_model: transformer" in ragged_refusal(arch_from_config(recipe_config("ds320tf")))
    assert "quantizer_conf.q0_ds_ratio" in ragged_refusal(arch_from_config(recipe_config("ds320q0")))
    assert "model_conf.segment_dur" in ragged_refusal(arch_from_config(recipe_config("ds320seg")))


# ---- the staging rules, restated (ragged_kernels.h: ragged_cols / ragged_extra; ragged_kernels.hip: ragged_stage_kernel) ----------
def _extra(n, k, pt, stride):
    num = n - k + pt
    nfr = -(-num // stride) if num >= 0 else -((-num) // stride)
    return nfr * stride + (k - pt) - n


def _stage_conv(x, lens, k, stride, dil, causal):
    """x [B, C, Tin] with garbage behind lens[b] -> [B, C, Tp]: [left padding | the row | right padding incl. its own extra | zeros]."""
    B, C, Tin = x.shape
    pt = (k - 1) * dil - (stride - 1)
    Tp = pt + Tin + _extra(Tin, k, pt, stride)
    buf = torch.zeros(B, C, Tp, dtype=x.dtype)
    for b, n in enumerate(lens):
        padL = pt if causal else pt - pt // 2
        padR = (0 if causal else pt // 2) + _extra(n, k, pt, stride)
        Leff = n if n > max(padL, padR) else max(padL, padR) + 1
        for q in range(padL + n + padR):
            rel = q - padL
            src = abs(rel)
            if src >= Leff:
                src = 2 * (Leff - 1) - src
            if 0 <= src < n:
                buf[b, :, q] = x[b, :, src]
    return buf


def _layers(name):
    a = arch_from_config(recipe_config(name))
    return a, [op for op in encoder_plan(a) + decoder_plan(a) if op.kind in ("conv", "convtr")]


@pytest.mark.parametrize("name", ["tiny", "tinywn", "ds320", "ss320"])
def test_staged_rows_equal_every_row_alone_in_float64(name):
    a, ops = _layers(name)
    norm = a.norm == "time_group_norm"
    causal = bool(a.causal)
    g = torch.Generator().manual_seed(5)
    seen = set()
    for op in ops:
        sig = (op.kind, op.k, op.stride, op.dilation)
        if sig in seen:              # the rules depend on (kind, k, stride, dilation, causal) alone, not on the channel counts
            continue
        seen.add(sig)
        k, s, d = op.k, op.stride, op.dilation
        pt = (k - 1) * d - (s - 1) if op.kind == "conv" else k - s
        Tmax = 53
        lens = sorted({1, 2, max(pt, 1), pt + 1, max(s - 1, 1), s + 1, 37, Tmax})
        cin, cout = 3, 2
        x = torch.randn(len(lens), cin, Tmax, dtype=torch.float64, generator=g)
        for b, n in enumerate(lens):
            x[b, :, n:] = float("nan")                      # what lies behind a row's end must never be read
        gamma = torch.randn(cout, dtype=torch.float64, generator=g) if norm else None
        beta = torch.randn(cout, dtype=torch.float64, generator=g) if norm else None
        bias = torch.randn(cout, dtype=torch.float64, generator=g)
        if op.kind == "conv":
            w = torch.randn(cout, cin, k, dtype=torch.float64, generator=g)
            y = F.conv1d(_stage_conv(x, lens, k, s, d, causal), w, bias, stride=s, dilation=d)      # plain, unpadded, common width
            for b, n in enumerate(lens):
                nout = -(-n // s)                           # the per-layer row-length rule: ceil at every stride
                yb = y[b:b + 1, :, :nout]
                if norm:                                    # statistics over the row's valid columns only
                    yb = F.group_norm(yb, 1, gamma, beta, a.gn_eps)
                ref = sconv1d(x[b:b + 1, :, :n], w, bias, gamma, beta, s, a.gn_eps, causal, d)
                assert ref.shape == yb.shape, (op.key, n, ref.shape, yb.shape)
                assert float((ref - yb).abs().max()) < 1e-12, (op.key, n)
        else:
            w = torch.randn(cin, cout, k, dtype=torch.float64, generator=g)
            buf = torch.zeros(len(lens), cin, Tmax + 2, dtype=torch.float64)      # [0 | the row | zeros]
            for b, n in enumerate(lens):
                buf[b, :, 1:1 + n] = x[b, :, :n]
            y = F.conv_transpose1d(buf, w, bias, stride=s)[..., s:]               # staged column j = x column j - 1
            pr = pt if causal else pt // 2
            pl = pt - pr
            for b, n in enumerate(lens):
                full = y[b:b + 1, :, :(n + 1) * s]                                # the row's UNTRIMMED output
                if norm:
                    full = F.group_norm(full, 1, gamma, beta, a.gn_eps)
                yb = full[..., pl:(n + 1) * s - pr]
                ref = sconvtr1d(x[b:b + 1, :, :n], w, bias, gamma, beta, s, a.gn_eps, causal)
                assert ref.shape == yb.shape == (1, cout, n * s), (op.key, n)
                assert float((ref - yb).abs().max()) < 1e-12, (op.key, n)
    assert len(seen) >= 3


def test_row_lengths_follow_the_ceil_at_every_stride():
    """fc_engine_frames's rule per row: nested ceilings over the encoder strides collapse to one ceiling over the hop."""
    a = arch_from_config(recipe_config("ds320"))
    hop = math.prod(a.ratios)
    for n in [1, 2, hop - 1, hop, hop + 1, 4321, 9999, 16000]:
        t = n
        for r in reversed(a.ratios):
            t = -(-t // r)
        assert t == -(-n // hop)
