"""Host side of slot sessions of a causal transformer net (fc_seqslots_*, ``open_slots(..., max_frames=N)``): the entry points, the
size of the state, the refusals that need no device, and what "per slot" means, in float64."""
import ctypes
import os
import re
import types

import pytest
import torch

from funcodec_amd import _lib
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.engine import EngineError
from funcodec_amd.plan import encoder_plan
from funcodec_amd.stream import StreamSlots, min_first
from funcodec_amd.synth import make_state_dict
from test_seq_transformer_gpu import transformer_f64
from test_seqstream_host import causal_tinytf, transformer_chunked_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQSLOTS_CALLS = {"fc_seqslots_state_bytes", "fc_seqslots_create", "fc_seqslots_forward"}
SEQSLOTS_ARGS = {name: _lib.SYMBOLS[name][1] for name in sorted(SEQSLOTS_CALLS)}      # everything below is about these calls: no binding, no module

# frames per round and slot; a negative count marks START.  Row counts 1, 15, 16, 17 and 33; positions that cross 16, 32 and 48; pushes
# that mix split rows (<= 16 frames), unsplit rows and idle rows; a row at position 0 beside one with several units; rows far narrower
# than the push; slot 2 restarted over a stale cache in round 7.  Slot 2's first utterance ends at exactly 50 frames.
ROUNDS = [
    (-7, 0, -17, 0),
    (1, -9, 1, 0),
    (1, 0, 16, -33),
    (8, 1, 0, 1),
    (0, 6, 15, 1),
    (16, 1, 1, 0),
    (1, 17, 0, 30),
    (1, 1, -7, 1),
]
ROUNDS_MAX_FRAMES = 66          # slot 3 ends at exactly 66 frames: the bound, and no multiple of 16


def utterances(rounds=ROUNDS):
    """per slot the list of its utterances, each the list of its pushes' frame counts"""
    out = [[] for _ in rounds[0]]
    for row in rounds:
        for slot, n in enumerate(row):
            if n < 0:
                out[slot].append([-n])
            elif n > 0:
                out[slot][-1].append(n)
    return out


def test_the_table_has_the_properties_the_kernel_can_go_wrong_at():
    counts = {abs(n) for row in ROUNDS for n in row}
    assert {1, 15, 16, 17, 33} <= counts
    utts = utterances()
    ends = [sum(u) for per in utts for u in per]
    assert max(ends) == ROUNDS_MAX_FRAMES and ROUNDS_MAX_FRAMES % 16 != 0
    for edge in (16, 32, 48):          # a push that begins below the edge and ends above it
        assert any(sum(u[:i]) < edge < sum(u[:i + 1]) for per in utts for u in per for i in range(len(u))), edge
    assert len(utts[2]) == 2 and sum(utts[2][0]) > sum(utts[2][1])         # the restart runs over a longer utterance's stale cache
    assert any(0 in row and any(0 < abs(n) <= 16 for n in row) and any(abs(n) > 16 for n in row) for row in ROUNDS)
    assert any(0 < abs(n) and 4 * abs(n) < max(abs(m) for m in row) for row in ROUNDS for n in row)


def test_seqslots_calls_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    declared = {n for n in re.findall(r"\b(fc_seqslots_[a-z_0-9]+)\s*\(", hdr)}
    bound = {n for n in _lib.SYMBOLS if n.startswith("fc_seqslots_")}
    assert declared == bound == SEQSLOTS_CALLS
    lib = ctypes.CDLL(_lib.lib_path())
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in SEQSLOTS_CALLS:
        assert hasattr(lib, name), name
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, flat).group(1)
        assert len([p for p in params.split(",") if p.strip()]) == len(SEQSLOTS_ARGS[name]), name
    assert _lib.FC_ABI_VERSION == 7 and "#define FC_ABI_VERSION 7 " in hdr and _lib.load().fc_abi_version() == 7


def test_state_size_is_the_lock_step_sessions():
    from funcodec_amd.engine import CodecEngine
    tiny = CodecEngine(arch_from_config(recipe_config("tiny")))              # not causal
    assert tiny.lib.fc_seqslots_state_bytes(tiny._h, 2, 37) == 0
    plain = CodecEngine(arch_from_config(recipe_config("tinywn")))          # causal, but its bottleneck is an LSTM
    assert plain.lib.fc_seqslots_state_bytes(plain._h, 2, 37) == 0
    for cfg in (causal_tinytf(), recipe_config("ss320tfc")):
        eng = CodecEngine(arch_from_config(cfg))
        assert eng.lib.fc_slots_state_bytes(eng._h, 1) == 0                  # without the bound it goes on refusing
        for S in (1, 3):
            for F in (7, 37, 1500):
                want = eng.lib.fc_seqstream_state_bytes(eng._h, S, F)
                assert want > 0 and eng.lib.fc_seqslots_state_bytes(eng._h, S, F) == want, (S, F)
        for S, F in ((1, 0), (0, 7), (-1, 7), (1, -3)):
            assert eng.lib.fc_seqslots_state_bytes(eng._h, S, F) == 0, (S, F)


def test_refusals_that_need_no_engine_call():
    ss = types.SimpleNamespace(arch=arch_from_config(recipe_config("ss320")))
    with pytest.raises(EngineError, match="max_frames"):
        StreamSlots(ss, 4, max_frames=64)
    tfc = arch_from_config(recipe_config("ss320tfc"))
    samples, frames = min_first(tfc)
    need = max(samples // 320, frames)
    assert need > 1
    with pytest.raises(EngineError, match="max_frames"):
        StreamSlots(types.SimpleNamespace(arch=tfc), 4, max_frames=need - 1)
    with pytest.raises(EngineError, match="seq_model: transformer"):          # without the bound: as before
        StreamSlots(types.SimpleNamespace(arch=tfc), 4)


def test_per_slot_means_the_chunked_rule_on_the_slots_own_pushes_in_float64():
    arch = arch_from_config(causal_tinytf(64))
    sd = make_state_dict(arch, 164)
    prefix = [op.key for op in encoder_plan(arch) if op.kind == "transformer"][0]
    for slot, per in enumerate(utterances()):
        for k, pushes in enumerate(per):
            T = sum(pushes)
            x = torch.randn(1, 64, T, generator=torch.Generator().manual_seed(100 * slot + k), dtype=torch.float64)
            whole = transformer_f64(x, sd, prefix, arch.lstm_layers, True, False)
            got = transformer_chunked_f64(x, sd, prefix, arch.lstm_layers, pushes)
            err = float((got - whole).abs().max())
            assert err < 1e-12, (slot, k, err)
