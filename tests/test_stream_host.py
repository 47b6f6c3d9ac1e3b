"""CPU tests of the streaming session: its C-ABI surface, what it refuses, and the per-layer geometry of a push (carry widths, staged and
output columns) restated in Python and checked against float64 torch on every conv of the causal recipes."""
import ctypes
import dataclasses
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from funcodec_amd import _lib
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.engine import EngineError
from funcodec_amd.stream import CodecStream, chunk_geometry, conv_layers, extra_padding, min_first, stream_refusal
from torch_oracle import get_extra_padding_for_conv1d, sconv1d, sconvtr1d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_CALLS = {"fc_stream_state_bytes", "fc_stream_create", "fc_stream_destroy", "fc_stream_min_first", "fc_stream_workspace_bytes",
                "fc_stream_reset", "fc_stream_encode", "fc_stream_decode_codes", "fc_stream_decode_emb", "fc_stream_lstm_forward"}


def test_stream_calls_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    declared = {n for n in re.findall(r"\b(fc_stream_[a-z_0-9]+)\s*\(", hdr)}
    bound = {n for n in _lib.SYMBOLS if n.startswith("fc_stream_")}
    assert declared == bound == STREAM_CALLS
    lib = ctypes.CDLL(_lib.lib_path())
    for name in STREAM_CALLS:
        assert hasattr(lib, name), name
    # one C parameter per ctypes argument
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in STREAM_CALLS:
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, flat).group(1)
        assert len([p for p in params.split(",") if p.strip()]) == len(_lib.SYMBOLS[name][1]), name
    assert _lib.FC_ABI_VERSION == 7 and "#define FC_ABI_VERSION 7 " in hdr and _lib.load().fc_abi_version() == 7


@pytest.mark.parametrize("name, change, key", [
    ("ds320", {}, "causal"),
    ("ss320tfc", {}, "seq_model: transformer"),
    ("ss320", {"model_type": "freq_codec"}, "freq_codec"),
    ("ss320", {"segment_dur": 0.5}, "model_conf.segment_dur"),
    ("ss320", {"q0_ds_ratio": 2}, "quantizer_conf.q0_ds_ratio"),
])
def test_codec_stream_refuses_what_is_out_of_scope_and_names_the_key(name, change, key):
    arch = dataclasses.replace(arch_from_config(recipe_config(name)), **change)
    assert key in stream_refusal(arch)
    with pytest.raises(EngineError, match=re.escape(key)):
        CodecStream(types.SimpleNamespace(arch=arch, engine=None), 1)      # refused before any engine call


@pytest.mark.parametrize("name", ["ss320", "ds320wn", "tinywn", "tinystwn", "tinyss"])
def test_causal_recipes_are_streamable(name):
    assert stream_refusal(arch_from_config(recipe_config(name))) is None


def test_a_stream_of_a_non_causal_engine_is_refused_by_the_library_too():
    from funcodec_amd.engine import CodecEngine
    eng = CodecEngine(arch_from_config(recipe_config("tiny")))
    assert eng.lib.fc_stream_state_bytes(eng._h, 2) == 0


def test_extra_padding_restated_in_integers():
    for k, s, d in [(7, 1, 1), (3, 1, 9), (4, 2, 1), (10, 5, 1), (16, 8, 1)]:
        pt = (k - 1) * d - (s - 1)
        for n in range(1, 200):
            assert extra_padding(n, k, s, pt) == get_extra_padding_for_conv1d(n, k, s, pt)


def _chunkings(n_first, cpf):
    """column counts of the pushes at one layer: a first push of n_first frames, then 1 frame per push / a mixed pattern, each with a
    whole last push and with ragged ones (1 column, one short of a frame, one more than a frame)"""
    out = []
    for frames in ([n_first] + [1] * 6, [n_first + 2, 3, 1, 5, 1], [n_first]):
        cols = [f * cpf for f in frames]
        out.append(cols)
        for tail in sorted({1, max(1, cpf - 1), cpf + 1}):
            out.append(cols + [tail])
    return out


@pytest.mark.parametrize("name", ["tinywn", "tinyss", "ss320"])
def test_chunked_layers_equal_the_whole_signal_in_float64(name):
    """Every conv and transposed conv of the net: the reference's causal layer on the whole signal (torch_oracle.sconv1d / sconvtr1d in
    float64) against the same torch conv WITHOUT padding over [carry | chunk | extra] pieces as the session stages them.  Channel counts are
    capped at 4 x 3 (the geometry does not depend on them).  Bound: float64 rounding of sums of <= 64 products of O(1) values, 1e-12."""
    arch = arch_from_config(recipe_config(name))
    enc_first, dec_first = min_first(arch)
    hop = arch.hop_length
    assert enc_first % hop == 0
    gen = torch.Generator().manual_seed(11)
    checked = 0
    for L in conv_layers(arch):
        cin, cout, k, s, d, pt, cpf = min(L["cin"], 4), min(L["cout"], 3), L["k"], L["stride"], L["dil"], L["carry"], L["cols_per_frame"]
        tr = L["kind"] == "convtr"
        assert pt == (1 if tr else (k - 1) * d - (s - 1))
        n_first = enc_first // hop if L["side"] == "encoder" else dec_first
        assert tr or n_first * cpf >= pt + 1, "the first push must hold the reflected left padding"
        w = torch.randn((cin, cout, k) if tr else (cout, cin, k), generator=gen, dtype=torch.float64)
        b = torch.randn(cout, generator=gen, dtype=torch.float64)
        for cols in _chunkings(n_first, cpf):
            if tr and cols[-1] % cpf:
                continue                                     # the decoder sees whole frames only
            x = torch.randn(2, cin, sum(cols), generator=gen, dtype=torch.float64)
            want = sconvtr1d(x, w, b, None, None, s, 0.0, True) if tr else sconv1d(x, w, b, None, None, s, 0.0, True, d)
            got, carry, pos = [], None, 0
            for i, tc in enumerate(cols):
                final = i == len(cols) - 1
                c = x[..., pos:pos + tc]
                pos += tc
                if carry is None:                            # first push: zeros (convtr) / the offline call's reflection
                    carry = torch.zeros(2, cin, 1, dtype=torch.float64) if tr else c[..., 1:pt + 1].flip(-1)
                buf = torch.cat([carry, c], -1)
                carry = buf[..., buf.shape[-1] - pt:]
                if tr:
                    y = F.conv_transpose1d(buf, w, b, stride=s)[..., s:s + tc * s]
                else:
                    extra = extra_padding(tc, k, s, pt) if final else 0
                    if extra:
                        buf = F.pad(buf, (0, extra), "reflect")
                    y = F.conv1d(buf, w, b, stride=s, dilation=d)
                tp, tout = chunk_geometry(L, tc, final)
                assert (buf.shape[-1], y.shape[-1]) == (tp, tout), (L, tc, final)
                if not final and not tr:
                    assert tout * s == tc
                got.append(y)
            got = torch.cat(got, -1)
            assert got.shape == want.shape, (L, cols)
            assert float((got - want).abs().max()) < 1e-12, (L, cols)
            checked += 1
    assert checked >= 10 * len(conv_layers(arch))
