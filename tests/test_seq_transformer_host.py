"""Host side of the transformer bottleneck (encoder_conf / decoder_conf ``seq_model: transformer``): config parsing, refusals, the
checkpoint contract against the real reference's key list, the synthetic checkpoints of every other configuration left unchanged, and the
C ABI entry point.  No GPU needed."""
import hashlib
import json
import os
import re

import pytest

from funcodec_amd import _lib
from funcodec_amd import config
from funcodec_amd.config import arch_from_config, recipe_config
from funcodec_amd.plan import expected_tensors
from funcodec_amd.synth import make_freq_state_dict, make_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# name -> (blocks, C, causal, model_type)
NEW = {
    "tinytf": (2, 64, False, "encodec"),
    "ds320tf": (2, 512, False, "encodec"),
    "ds640tf": (2, 1024, False, "encodec"),
    "ss320tfc": (2, 512, True, "encodec"),
    "ds320tfseg": (2, 512, False, "encodec"),
    "freqmptf": (2, 512, False, "freq_codec"),
}
KEYS = {"tinytf": "tinytf", "ds320tf": "ds320tf", "ds640tf": "ds640tf", "ss320tfc": "ss320tfc", "freqmptf": "freqmptf"}


def _state(name, seed=0):
    cfg = recipe_config(name)
    arch = arch_from_config(cfg)
    return arch, (make_freq_state_dict(cfg, seed) if arch.model_type == "freq_codec" else make_state_dict(arch, seed))


@pytest.mark.parametrize("name", sorted(NEW))
def test_new_recipes_parse(name):
    blocks, c, causal, mt = NEW[name]
    a = arch_from_config(recipe_config(name))
    assert a.seq_model == "transformer" and a.lstm_layers == blocks and a.lstm_skip
    assert a.bottleneck_channels == c and c // 4 in (16, 32, 64, 128, 256)
    assert a.causal == causal and a.model_type == mt
    if name == "ds320tfseg":
        assert a.segment_length == 8000


@pytest.mark.parametrize("name", sorted(KEYS))
def test_checkpoint_contract_matches_the_reference(name):
    """plan.expected_tensors and the synthetic checkpoint both equal the key / shape list of the reference's own state_dict
    (tests/golden/state_dict_keys_<cfg>.json, written by tools/make_golden_seqtf.py from the real reference)."""
    ref = {k: tuple(s) for k, s in json.load(open(os.path.join(GOLD, f"state_dict_keys_{KEYS[name]}.json")))}
    arch, sd = _state(name)
    assert expected_tensors(arch) == ref
    hot = {k: tuple(v.shape) for k, v in sd.items() if k.startswith(("encoder.", "decoder.")) or k == "quantizer.rq.model.embed"}
    assert hot == ref
    tf = [k for k in ref if ".encoders." in k or ".after_norm." in k]
    assert len(tf) == 2 * (2 * 16 + 2)           # encoder + decoder, 2 blocks of 16 tensors + after_norm
    assert ref[[k for k in tf if k.endswith("feed_forward.w_1.weight")][0]] == (config.SEQ_FF, arch.bottleneck_channels)


def _cfg_with(base, **conf):
    cfg = recipe_config(base)
    for k in ("encoder_conf", "decoder_conf"):
        cfg[k].update(conf)
    return cfg


def test_refusals_are_by_name():
    with pytest.raises(NotImplementedError, match="transformer"):
        arch_from_config(_cfg_with("tiny", seq_model="transformer"))                    # C = 32: head size 8 is not built
    with pytest.raises(NotImplementedError, match="transformer"):
        arch_from_config(_cfg_with("ds640", seq_model="transformer", n_filters=64))     # C = 2048
    cfg = recipe_config("ds320tf")
    cfg["decoder_conf"]["seq_model"] = "lstm"
    with pytest.raises(NotImplementedError, match="seq_model"):
        arch_from_config(cfg)
    with pytest.raises(NotImplementedError, match="seq_layer_num"):
        arch_from_config(_cfg_with("ds320", seq_model="transformer", seq_layer_num=0))
    cfg = recipe_config("freqmptf")
    cfg["encoder_conf"]["n_filters"] = cfg["decoder_conf"]["n_filters"] = 8              # 2-D nets: C = 128 is built, C = 32 is not
    assert arch_from_config(cfg).bottleneck_channels == 128
    cfg["encoder_conf"]["n_filters"] = cfg["decoder_conf"]["n_filters"] = 2
    with pytest.raises(NotImplementedError, match="transformer"):
        arch_from_config(cfg)


def _digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode()); h.update(str(sd[k].dtype).encode()); h.update(str(sd[k].shape).encode()); h.update(sd[k].tobytes())
    return h.hexdigest()


# recorded from the parent commit (before the transformer existed): the committed goldens of these configs depend on their weights
PARENT_DIGESTS = {
    "tiny": "95b0cce7a3bdc97a9abcfb6781dc7e449a81cb96d3bb326760091d9d640b0c23",
    "ds320": "71be93fa8f2018564d53fcdf1d0c43ec897b5a95dcc8c8aff7bd1f90db0a103b",
    "ss320": "d37422f1e7dd828c75c60495966f6fe52a841d6544cb69a15023e6fdbac1aa23",
    "freqmp": "a828c4bb689f10bb1e5e82bdb4ba64ccb49c1de8dab3923a8f17d7a4d2c2f087",
    "freqmpgr1rel": "6d13afb274b2e2c27107ba4c571953d02209dbcbee3bdd1b07f758e749925a66",
}


@pytest.mark.parametrize("name", sorted(PARENT_DIGESTS))
def test_existing_synthetic_checkpoints_are_unchanged(name):
    arch, sd = _state(name)
    assert arch.seq_model == "lstm"
    assert _digest(sd) == PARENT_DIGESTS[name]


def test_fc_seq_forward_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "funcodec_amd.h")).read()
    assert re.search(r"int fc_seq_forward\(fc_engine\* e, const char\* prefix, const float\* x, int B, int T,\s*float\* y, void\* workspace, "
                     r"size_t workspace_bytes, void\* stream\);", hdr)
    assert "fc_seq_forward" in _lib.SYMBOLS
    assert [f[0] for f in _lib.FcArch._fields_][-3:] == ["seq_model", "seq_heads", "seq_ff"] and _lib.FC_ABI_VERSION == 7
    lib = _lib.load()                         # binds every symbol of SYMBOLS: an unexported one raises
    assert lib.fc_seq_forward is not None and lib.fc_abi_version() == 7
