"""TEST INFRASTRUCTURE ONLY.  Generates the text-to-music LauraTTS fixtures (recipe egs/jamendo/text2music_laura, config
``lauramusic``: d_model 1024, 16 heads, feed-forward 4096, T5-base input width 768) by running the REAL reference on CPU in the build
container, the way oracle/make_golden_laura.py does for the speech recipe (whose ``run_case`` pins oracle/laura_oracle.py against the
reference bit for bit while it writes):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_laura_music.py [CASE ...]

writes tests/golden/laura_music_b2.npz, laura_music_cont_b2.npz, laura_e2e_music_freqmp640.npz, state_dict_keys_lauramusic.json and
MANIFEST_laura_music.json.  Weights (about 330 M parameters) are never stored: funcodec_amd.synth re-creates them from seeds.

The e2e case runs the reference Text2Audio.__call__ in continual mode with funcodec_amd.synth.synthetic_text_embedder in place of the
T5 encoder (build_text_emb_model patched).  Its codec is the FreqCodec ds640 recipe (``freqmp640``): a STAND-IN.  The released music
model pairs with the FreqCodec "universal-general nq32ds640", whose config.yaml is not in the reference tree.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_shim  # noqa: E402
from make_golden_laura import GOLD, build_reference_model, run_case  # noqa: E402  (installs ref_shim)

from funcodec_amd.config import recipe_config  # noqa: E402
from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config  # noqa: E402
from funcodec_amd.synth import (make_freq_state_dict, make_laura_state_dict, synthetic_audio,  # noqa: E402
                                synthetic_text_embedder, write_checkpoint)

MANIFEST = os.path.join(GOLD, "MANIFEST_laura_music.json")
# name, config, weight seed, text seed, text lengths, max_length, continual lengths (make_golden_laura.run_case)
CASES = [
    ("laura_music_b2", "lauramusic", 10, 40, [19, 11], 10, None),
    ("laura_music_cont_b2", "lauramusic", 11, 41, [14, 23], 9, [10, 6]),
]
# name, laura config, laura seed, embedder seed, codec config, codec seed, text, prompt text, prompt samples, max_length
E2E_CASES = [
    ("laura_e2e_music_freqmp640", "lauramusic", 12, 5, "freqmp640", 0,
     "an upbeat acoustic folk song with bright guitar and hand claps", "calm piano", 9600, 10),
]


def run_e2e(name, lcfg_name, lseed, eseed, ccfg_name, cseed, text, prompt_text, prompt_samples, max_length):
    """The REAL Text2Audio.__call__ (bin/text2audio_inference.py:137-198), continual mode, greedy, stand-in text embedder."""
    from funcodec.bin.text2audio_inference import Text2Audio
    from make_golden import reference_config
    ref_shim.install_torchaudio_transforms()      # FreqCodec's Spectrogram / InverseSpectrogram (torchaudio is a stub here)
    lcfg = laura_recipe_config(lcfg_name)
    spec = laura_spec_from_config(lcfg)
    lsd = make_laura_state_dict(lcfg, lseed)
    ccfg = recipe_config(ccfg_name)
    csd = make_freq_state_dict(ccfg, cseed)
    lsd["quantizer_codebook.embed"] = csd["quantizer.rq.model.embed"][: spec.num_quantizers].copy()
    prompt_audio = synthetic_audio(1, prompt_samples, lseed + 600, "tones")
    embedder = synthetic_text_embedder(lcfg, eseed)
    real_build = Text2Audio.build_text_emb_model
    Text2Audio.build_text_emb_model = lambda self, path: embedder
    try:
        with tempfile.TemporaryDirectory() as tmp:
            lcfg_path, lpth_path = write_checkpoint(os.path.join(tmp, "laura"), lcfg, lsd)
            ccfg_path, cpth_path = write_checkpoint(os.path.join(tmp, "codec"), reference_config(ccfg), csd)
            t2a = Text2Audio(config_file=lcfg_path, model_file=lpth_path, device="cpu", text_emb_model="t5-base", beam_size=1,
                             sampling=False, continual=True, codec_config_file=ccfg_path, codec_model_file=cpth_path,
                             tokenize_to_phone=False, exclude_prompt=True)
            real_decode = t2a.model.decode_codec
            t2a.model.decode_codec = lambda *a, **k: real_decode(*a, **{**k, "max_length": max_length})
            with torch.no_grad():
                ret, decoded = t2a(text, prompt_text, prompt_audio)
    finally:
        Text2Audio.build_text_emb_model = real_build
    arrays = dict(gen=ret["gen"].numpy(), gen_only_lm=ret["gen_only_lm"].numpy(), decoded_codec=decoded[0].numpy().astype(np.int16))
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **arrays)
    meta = dict(laura_config=lcfg_name, laura_seed=lseed, embedder_seed=eseed, codec_config=ccfg_name, codec_seed=cseed, text=text,
                prompt_text=prompt_text, prompt_samples=prompt_samples, prompt_audio_seed=lseed + 600, max_length=max_length,
                decoded_frames=int(decoded.shape[1]), gen_samples=int(ret["gen"].shape[-1]),
                codec_note="stand-in: the released universal nq32ds640 FreqCodec config is not in the reference tree")
    print(name, {k: v for k, v in meta.items() if k not in ("text", "prompt_text", "codec_note")}, flush=True)
    return meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*")
    only = set(ap.parse_args().cases) or None
    torch.manual_seed(0)
    manifest = json.load(open(MANIFEST)) if os.path.exists(MANIFEST) else {"cases": {}, "e2e": {}}
    manifest.update(torch=torch.__version__, threads=torch.get_num_threads())

    def save():
        with open(MANIFEST, "wt") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)

    if only is None or "keys" in only:
        cfg = laura_recipe_config("lauramusic")
        model = build_reference_model(cfg, make_laura_state_dict(cfg, 0))
        with open(os.path.join(GOLD, "state_dict_keys_lauramusic.json"), "wt") as f:
            json.dump({k: list(v.shape) for k, v in model.state_dict().items()}, f, indent=0, sort_keys=True)
        del model
    for c in CASES:
        if only is None or c[0] in only:
            manifest["cases"][c[0]] = run_case(*c)
            save()
    for c in E2E_CASES:
        if only is None or c[0] in only:
            manifest["e2e"][c[0]] = run_e2e(*c)
            save()


if __name__ == "__main__":
    main()
