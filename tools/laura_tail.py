"""Time the two ends of ``Text2Audio.generate_many`` around the decoding session -- the codec encode of the prompt recordings, the fine
predictor and the codec decoder -- per phase, with one codec call per utterance (the default) and as length-aware batches
(``length_aware=True``), on the synthetic checkpoints of the ``laura`` and ``lauramusic`` recipes (the method of
``tools/laura_start_from.py``: warm-up, then synchronised repetitions, the two forms alternating in one process; median and min .. max).

Phases of one call: prompt encode (``_prompt_codecs``), text encode (``_encode_texts``), LM (the session: the call minus the other
phases), and the tail (``_synthesise``): fine predictor (``cal_codec_emb_batch``), ``gen_only_lm`` decode (``run_mod="decode"``), ``gen``
decode (``run_mod="decode_emb"``), and what is left of the tail (host: padding, packing, cutting the rows).  Every phase is timed between
two synchronisations, in both forms alike.

Workloads: (A) 16 requests x 4 samples at max_length 100 through 16 slots, keep="all" and keep="best" (README's figures; no prompt
recordings); (B) 64 requests with recordings of 1 - 5 s whose max_length is spread over 50 .. 750 (set per request as its text is
encoded, just before its slot starts), 16 slots.

Condition (exit status): the tail of (A) is faster with length_aware and the two forms' min .. max do not overlap, wherever the codec
has length-aware calls; a codec that refuses them (``engine.ragged_refusal``) is reported with its refusal and timed in the default
form alone.

    python tools/laura_tail.py [--out profiles/laura_tail.txt] [--reps 24] [--models laura,lauramusic]
    python tools/laura_tail.py --default-only          # totals of the default form alone (no length_aware keyword: runs on older trees)
"""
import argparse
import datetime
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from funcodec_amd.laura_config import laura_recipe_config, laura_spec_from_config   # noqa: E402
from funcodec_amd.synth import make_laura_state_dict                                # noqa: E402

CODEC = {"laura": "ds640", "lauramusic": "freqmp640"}          # the codecs the end-to-end fixtures pair the recipes with
PHASES = ["prompt encode", "text encode", "LM", "fine predictor", "gen decode", "gen_only_lm decode", "tail, rest", "tail", "call"]
TAIL = ["fine predictor", "gen decode", "gen_only_lm decode"]


class Clock:
    """seconds per phase of the call that is running, each between two synchronisations"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.t = {}
        self.calls = {}

    def time(self, name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0
        self.calls[name] = self.calls.get(name, 0) + 1
        return out

    def phases(self):
        t = dict(self.t)
        for k in PHASES:
            t.setdefault(k, 0.0)
        t["tail, rest"] = t["tail"] - sum(t[k] for k in TAIL)
        t["LM"] = t["call"] - t["prompt encode"] - t["text encode"] - t["tail"]
        return t


class TimedCodec:
    """the Speech2Token of a Text2Audio with its two decode modes on the clock (the encode calls are inside "prompt encode")"""

    def __init__(self, inner, clock):
        self.inner, self.clock, self.model = inner, clock, inner.model

    def __call__(self, speech, *a, **k):
        name = {"decode": "gen_only_lm decode", "decode_emb": "gen decode"}.get(k.get("run_mod"))
        if name is None:
            return self.inner(speech, *a, **k)
        return self.clock.time(name, lambda: self.inner(speech, *a, **k))


def build(name, max_positions):
    """(Text2Audio of the recipe's synthetic checkpoints with its phases on a clock, the clock)"""
    from funcodec_amd.bin.text2audio_inference import Text2Audio
    from funcodec_amd.config import arch_from_config, recipe_config
    from funcodec_amd.synth import make_freq_state_dict, make_state_dict, synthetic_text_embedder, write_checkpoint
    cfg = laura_recipe_config(name)
    spec = laura_spec_from_config(cfg)
    ccfg = recipe_config(CODEC[name])
    csd = make_freq_state_dict(ccfg, 0) if CODEC[name].startswith("freq") else make_state_dict(arch_from_config(ccfg), 0)
    lsd = make_laura_state_dict(cfg, 0)
    lsd["quantizer_codebook.embed"] = csd["quantizer.rq.model.embed"][: spec.num_quantizers].copy()
    tmp = tempfile.mkdtemp(prefix="laura_tail_")
    try:
        lc, lp = write_checkpoint(os.path.join(tmp, "laura"), cfg, lsd)
        del lsd
        cc, cp = write_checkpoint(os.path.join(tmp, "codec"), ccfg, csd)
        t2a = Text2Audio(config_file=lc, model_file=lp, device="cuda", text_emb_model=synthetic_text_embedder(cfg, 5), beam_size=1,
                         sampling=True, continual=True, codec_config_file=cc, codec_model_file=cp, tokenize_to_phone=False,
                         exclude_prompt=True, max_length=100, max_positions=max_positions)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    clock = Clock()
    t2a.max_length_of = {}                  # text -> max_length of that request (workload B)
    prompt_codecs, encode_texts, synthesise, codec_emb = t2a._prompt_codecs, t2a._encode_texts, t2a._synthesise, t2a.model.cal_codec_emb_batch

    def texts_on_the_clock(texts):
        if len(texts) == 1 and texts[0] in t2a.max_length_of:          # generate_many encodes a request alone, just before its slot starts
            t2a.max_length = t2a.max_length_of[texts[0]]
        return clock.time("text encode", lambda: encode_texts(texts))
    t2a._prompt_codecs = lambda *a, **k: clock.time("prompt encode", lambda: prompt_codecs(*a, **k))
    t2a._encode_texts = texts_on_the_clock
    t2a._synthesise = lambda *a, **k: clock.time("tail", lambda: synthesise(*a, **k))
    t2a.model.cal_codec_emb_batch = lambda *a, **k: clock.time("fine predictor", lambda: codec_emb(*a, **k))
    t2a.codec_model = TimedCodec(t2a.codec_model, clock)
    return t2a, clock


def workload_a(keep):
    n, N = 16, 4
    texts = [" ".join(f"w{i}x{k}" for k in range(16 + (5 * i) % 11)) for i in range(n)]
    seeds = [[1000 + N * i + k for k in range(N)] for i in range(n)]
    return dict(texts=texts, slots=16, seeds=seeds, samples=N, keep=keep), {}


def workload_b(t2a):
    from funcodec_amd.synth import synthetic_audio
    n = 64
    rate = t2a.codec_model.model.quantizer.sampling_rate
    texts = [" ".join(f"v{i}x{k}" for k in range(12 + (5 * i) % 11)) for i in range(n)]
    ptexts = [" ".join(f"p{i}x{k}" for k in range(4)) for i in range(n)]
    audios = [synthetic_audio(1, int(rate * (1 + 4 * ((29 * i) % n) / (n - 1))), 700 + i, "tones") for i in range(n)]
    limits = {" ".join([p, t]): 50 + (700 * ((37 * i) % n)) // (n - 1) for i, (p, t) in enumerate(zip(ptexts, texts))}
    return dict(texts=texts, prompt_texts=ptexts, prompt_audios=audios, slots=16, seeds=[2000 + i for i in range(n)]), limits


def flat(codecs):
    return [c for row in codecs for c in (row if isinstance(row, list) else [row])]


def measure(t2a, clock, kw, limits, forms, reps, say, title):
    """reps calls per form, the forms alternating; {form: {phase: [seconds]}}"""
    def call(form):
        clock.reset()
        t2a.max_length_of, t2a.max_length = limits, 100
        more = dict(length_aware=True) if form == "length_aware" else {}
        return clock.time("call", lambda: t2a.generate_many(**kw, **more))
    got = {f: call(f) for f in forms}                          # warm-up, and the same tokens in both forms
    calls = {f: None for f in forms}
    ref = flat(got[forms[0]][1])
    for f in forms[1:]:
        new = flat(got[f][1])
        assert len(new) == len(ref) and all(torch.equal(a, b) for a, b in zip(new, ref)), "the forms disagree on the tokens"
    frames = sorted(int(r["gen"].shape[-1]) // t2a.codec_model.model.engine.hop_length for r in flat(got[forms[0]][0]))
    del got
    t = {f: {k: [] for k in PHASES} for f in forms}
    for r in range(reps + 1):                                  # one more warm-up round
        for f in forms:
            call(f)
            calls[f] = dict(clock.calls)
            if r:
                for k, v in clock.phases().items():
                    t[f][k].append(v)
    say(f"  {title}: {len(frames)} utterances reach the tail, frames decoded min {frames[0]} / median {frames[len(frames) // 2]} / max {frames[-1]}; "
        f"{reps} repetitions per form, forms alternating")
    for f in forms:
        c = calls[f]
        say(f"      {f:12s} codec calls: gen {c.get('gen decode', 0)}, gen_only_lm {c.get('gen_only_lm decode', 0)}; fine predictor calls "
            f"{c.get('fine predictor', 0)}")
    ms = lambda v: f"{statistics.median(v) * 1e3:8.2f} ({min(v) * 1e3:7.2f} .. {max(v) * 1e3:7.2f})"          # noqa: E731
    say(f"      {'phase, ms: median (min .. max)':32s} {'default':>30s}" + (f" {'length_aware':>30s}   l.a. / default" if len(forms) > 1 else ""))
    for k in PHASES:
        line = f"      {k:32s} {ms(t[forms[0]][k]):>30s}"
        if len(forms) > 1:
            a, b = statistics.median(t[forms[0]][k]), statistics.median(t[forms[1]][k])
            line += f" {ms(t[forms[1]][k]):>30s}   " + (f"{b / a:6.3f}" if a > 1e-5 else "     -")
        say(line)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--models", default="laura,lauramusic")
    ap.add_argument("--default-only", action="store_true")
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", "laura_tail_default.txt" if args.default_only else "laura_tail.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/laura_tail.py{' --default-only' if args.default_only else ''}  {datetime.date.today().isoformat()}  "
        f"{torch.cuda.get_device_name(0)}  torch {torch.__version__}")
    ok = True
    for name in args.models.split(","):
        t2a, clock = build(name, 1024)                        # one session size for both workloads: (B) needs up to 903 positions
        forms = ["default"]
        say(f"{name} + {CODEC[name]}, max_positions 1024")
        if not args.default_only:
            from funcodec_amd.engine import ragged_refusal
            why = ragged_refusal(t2a.codec_model.model.arch)
            if why:
                say(f"  length_aware=True is refused ({why}): the default form alone")
            else:
                forms.append("length_aware")
        for which in ("A", "B"):
            if which == "A":
                for keep in ("all", "best"):
                    kw, limits = workload_a(keep)
                    t = measure(t2a, clock, kw, limits, forms, args.reps, say, f"(A) 16 requests x 4 samples, max_length 100, keep=\"{keep}\"")
                    if len(forms) > 1:
                        d, la = t["default"]["tail"], t["length_aware"]["tail"]
                        met = max(la) < min(d)
                        ok = ok and met
                        say(f"      tail: length_aware / default = {statistics.median(la) / statistics.median(d):.3f}; faster, min .. max apart: "
                            f"{'met' if met else 'MISSED'}")
            else:
                kw, limits = workload_b(t2a)
                measure(t2a, clock, kw, limits, forms, args.reps, say, "(B) 64 requests, max_length 50 .. 750, recordings of 1 - 5 s")
        del t2a, clock
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
