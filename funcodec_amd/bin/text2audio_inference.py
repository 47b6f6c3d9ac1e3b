"""``Text2Audio`` -- same constructor keywords, call signature and return value as the reference's
funcodec/bin/text2audio_inference.py:30-198 (LauraTTS zero-shot generation), running on the MI355X engines:

    from funcodec_amd.bin.text2audio_inference import Text2Audio
    t2a = Text2Audio(config_file="config.yaml", model_file="model.pth", device="cuda", text_emb_model=None, beam_size=1,
                     sampling=25, continual=True, codec_config_file="codec/config.yaml", codec_model_file="codec/model.pth")
    ret_val, decoded_codec = t2a(text, prompt_text, prompt_audio)          # ret_val = {"gen": wav, "gen_only_lm": wav}

plus ``generate_batch`` (up to 16 prompts per engine call: the reference is batch-1 with one host round trip per token) and
``generate_many`` (any number of prompts through a decoding session whose slots are refilled as utterances end).
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from pathlib import Path
from typing import Any, List, Optional, Sequence, Union

import numpy as np
import torch

from ..laura import LauraGenMI355X
from ..laura_config import laura_spec_from_config
from .codec_inference import Speech2Token


def build_model_from_file(config_file, model_file, device="cuda", max_positions: int = 2048):
    """Counterpart of Text2AudioGenTask.build_model_from_file (funcodec/tasks/abs_task.py:1895-1947)."""
    import yaml
    with open(config_file, "rt", encoding="utf-8") as f:
        args = yaml.safe_load(f)
    spec = laura_spec_from_config(args)
    model = LauraGenMI355X(spec, device=device, max_positions=max_positions)
    if model_file is not None:
        model.load_state_dict(torch.load(model_file, map_location="cpu"))
    return model, argparse.Namespace(**args)


class Text2Audio:
    """Text2Audio class (drop-in for funcodec.bin.text2audio_inference.Text2Audio)."""

    def __init__(
            self,
            config_file: Union[Path, str] = None,
            model_file: Union[Path, str] = None,
            device: str = "cuda",
            dtype: str = "float32",
            **kwargs
    ):
        if dtype != "float32":
            raise NotImplementedError("the MI355X LauraTTS engine computes in float32 (the reference's default)")
        if device == "cpu":
            raise RuntimeError("funcodec_amd.Text2Audio runs on MI355X only; use the reference for device='cpu'")
        model, model_args = build_model_from_file(config_file, model_file, device, kwargs.get("max_positions", 2048))
        self.model = model
        self.model_args = model_args
        self.device = device
        self.dtype = dtype
        text_emb_model = kwargs.get("text_emb_model")
        self.beam_size = kwargs.get("beam_size", 1)
        self.sampling = kwargs.get("sampling", True)
        self.continual = kwargs.get("continual", True)
        self.tokenize_to_phone = kwargs.get("tokenize_to_phone", False)
        self.exclude_prompt = kwargs.get("exclude_prompt", True)
        self.max_length = kwargs.get("max_length", 30 * 25)          # bin/text2audio_inference.py:168
        if self.tokenize_to_phone:
            raise NotImplementedError("tokenize_to_phone needs the g2p_en package (third party, not in this image); pass phoneme strings")
        if not self.model.vocab_size:
            # embedding-input checkpoints: the reference runs a T5 encoder from `transformers` (:115-135), a third-party model
            # outside this engine; any callable text -> (embeddings [1, L, input_size], lengths [1]) is accepted in its place
            if callable(text_emb_model):
                self.text_emb_model = text_emb_model
            elif text_emb_model:
                self.text_emb_model = self.build_text_emb_model(text_emb_model)
            else:
                raise ValueError("an embedding-input LauraTTS checkpoint needs text_emb_model (a T5 path or a callable)")
        else:
            self.text_emb_model = self.tokenize_text
        codec_kwargs = dict(config_file=kwargs["codec_config_file"], model_file=kwargs["codec_model_file"], device=device)
        self.codec_model = Speech2Token.from_pretrained(model_tag=None, **codec_kwargs)

    # -- text side (bin/text2audio_inference.py:99-135) ------------------------------------------------------------------------
    def token_ids(self, text: str) -> List[int]:
        """tokenize_text (:99-110): whitespace split, tokens missing from the list are dropped."""
        toks = self.model.token_list
        index = getattr(self, "_tok_index", None)
        if index is None:
            index = self._tok_index = {}
            for i, t in enumerate(toks):
                index.setdefault(t, i)              # list.index semantics: first occurrence
        return [index[one] for one in text.strip().split(" ") if one in index]

    def tokenize_text(self, text: str):
        ids = self.token_ids(text)
        logging.info(" ".join(str(x) for x in ids))
        token_idx = torch.tensor(ids, dtype=torch.int64, device=self.model.device)
        text_emb = self.model.token_embedding(token_idx)          # ids: the lookup happens inside the engine (fc_laura_encode)
        return text_emb.unsqueeze(0), torch.tensor([len(ids)], dtype=torch.int64, device=self.model.device)

    def build_text_emb_model(self, model_path: str):
        emb_type = "enc"
        if ":" in model_path:
            model_path, emb_type = model_path.rsplit(":", maxsplit=1)
        from transformers import T5Model, T5Tokenizer
        tokenizer = T5Tokenizer.from_pretrained(model_path)
        model = T5Model.from_pretrained(model_path).to(self.model.device)

        def _forward(text: str):
            inputs = tokenizer(text, return_tensors="pt")
            inputs = {k: v.to(self.model.device) for k, v in inputs.items()}
            with torch.no_grad():
                if emb_type == "enc":
                    outputs = model.encoder(inputs["input_ids"]).last_hidden_state
                else:
                    outputs = model.shared(inputs["input_ids"])
            return outputs, inputs["attention_mask"].sum(dim=1)

        return _forward

    # -- one utterance, exactly the reference's flow (:137-198) ----------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, text: str, prompt_text: str = None, prompt_audio: np.ndarray = None):
        ret, codecs = self.generate_batch([text], None if prompt_text is None else [prompt_text],
                                          None if prompt_audio is None else [prompt_audio])
        return ret[0], codecs[0]

    # -- the parts generate_batch and generate_many share ---------------------------------------------------------------------------
    def _refuse_length_aware(self, who: str):
        """length_aware=True with a codec that has no length-aware calls raises here, before any engine call: nothing falls back."""
        from ..engine import EngineError, ragged_refusal
        why = ragged_refusal(self.codec_model.model.arch)
        if why:
            raise EngineError(f"{who}(length_aware=True): {why}")

    def _prompt_codecs(self, prompt_audios, length_aware: bool = False):
        """First predict_nq code groups of every prompt recording: [T, nq] each (one codec call each: no padding inside an utterance).
        length_aware: the recordings in arrival order, 16 per codec call, zero-padded to the longest of the call and coded by their own
        lengths (speech_lengths: every row as if it were alone)."""
        per = []
        if length_aware:
            frames = self.codec_model.model.engine.frames
            wavs = [torch.as_tensor(a, dtype=torch.float32) for a in prompt_audios]
            for i, a in enumerate(wavs):
                if a.dim() < 2 or a.shape[0] != 1 or tuple(a.shape[1:-1]) != tuple(wavs[0].shape[1:-1]):
                    raise ValueError(f"prompt recording {i}: one utterance [1, T] (or [1, C, T]) each, got {tuple(a.shape)}")
            for g in (wavs[i: i + 16] for i in range(0, len(wavs), 16)):
                ns = [int(a.shape[-1]) for a in g]
                speech = torch.zeros((len(g),) + tuple(g[0].shape[1:-1]) + (max(ns),), dtype=torch.float32)
                for b, a in enumerate(g):
                    speech[b, ..., : ns[b]] = a[0]
                codes = self.codec_model(speech, run_mod="encode", speech_lengths=torch.tensor(ns, dtype=torch.int64))[0][0]     # [n_q, B, Tf]
                per += [codes[:, b, : frames(ns[b])].transpose(0, 1)[:, : self.model.predict_nq] for b in range(len(g))]
            return per
        for a in prompt_audios:
            a = torch.as_tensor(a, dtype=torch.float32)
            codec = self.codec_model(a, run_mod="encode")[0][0].squeeze(1).transpose(0, 1)      # [T, n_q]
            per.append(codec[:, : self.model.predict_nq])
        return per

    def _encode_texts(self, texts):
        """0. text embeddings, 1. text encoder: (text_outs [n, L, D], lengths)."""
        m, n = self.model, len(texts)
        embs, lens = [], []
        for t in texts:
            e, l = self.text_emb_model(t)
            embs.append(e[0])
            lens.append(int(l.reshape(-1)[0]))
        L = max(lens)
        if embs[0].is_floating_point():
            text_in = torch.zeros((n, L, embs[0].shape[-1]), dtype=torch.float32, device=m.device)
        else:
            text_in = torch.full((n, L), -1, dtype=torch.int64, device=m.device)
        for i, e in enumerate(embs):
            text_in[i, : lens[i]] = e[: lens[i]].to(m.device)
        text_outs, _ = m.encode(text_in, torch.tensor(lens))
        return text_outs, lens

    def _synthesise(self, text_outs, lens, tokens, out_lens, excl, length_aware: bool = False):
        """3. dense embeddings of all codec groups, then the codec decoder, for one batch of finished utterances.
        length_aware: two codec calls for the batch instead of two per utterance -- row j's frames [excl[j] or 0, out_lens[j]) packed to
        the front of a padded batch (laura.pack_windows) and decoded by their own count (speech_lengths: every row as if it were alone)."""
        emb = self.model.cal_codec_emb_batch(text_outs, lens, tokens, out_lens)
        if length_aware:
            return self._decode_length_aware(emb, tokens, out_lens, excl)
        rets, codecs = [], []
        for i in range(len(lens)):
            dec = tokens[i: i + 1, : out_lens[i]]
            lo = excl[i]
            _, _, gen_only_lm, _ = self.codec_model(dec[:, lo:], bit_width=None, run_mod="decode")
            _, _, gen, _ = self.codec_model(emb[i: i + 1, : out_lens[i]][:, lo:], run_mod="decode_emb")
            rets.append(dict(gen=gen, gen_only_lm=gen_only_lm))
            codecs.append(dec)
        return rets, codecs

    def _decode_length_aware(self, emb, tokens, out_lens, excl):
        from ..laura import pack_windows
        n = len(out_lens)
        lo = [int(e or 0) for e in excl]
        k = [int(out_lens[j]) - lo[j] for j in range(n)]
        live = [j for j in range(n) if k[j] > 0]
        rets = [None] * n
        if live:
            rows = slice(None) if len(live) == n else live
            lo_l, hi_l = [lo[j] for j in live], [int(out_lens[j]) for j in live]
            ks = torch.tensor([k[j] for j in live], dtype=torch.int64)
            _, _, only_lm, _ = self.codec_model(pack_windows(tokens[rows], lo_l, hi_l), bit_width=None, run_mod="decode", speech_lengths=ks)
            _, _, gen, _ = self.codec_model(pack_windows(emb[rows], lo_l, hi_l), run_mod="decode_emb", speech_lengths=ks)
            samples = self.codec_model.model.engine.decoded_samples
            for r, j in enumerate(live):
                ns = samples(k[j])
                rets[j] = dict(gen=gen[r: r + 1, :, : ns].clone(), gen_only_lm=only_lm[r: r + 1, :, : ns].clone())
        for j in range(n):
            if rets[j] is None:       # no frame behind the prompt: the row is in no batch and gets what the one-utterance calls give it
                dec = tokens[j: j + 1, : out_lens[j]]
                _, _, only_lm, _ = self.codec_model(dec[:, excl[j]:], bit_width=None, run_mod="decode")
                _, _, gen, _ = self.codec_model(emb[j: j + 1, : out_lens[j]][:, excl[j]:], run_mod="decode_emb")
                rets[j] = dict(gen=gen, gen_only_lm=only_lm)
        return rets, [tokens[j: j + 1, : out_lens[j]] for j in range(n)]

    # -- up to 16 prompts per engine call -----------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate_batch(self, texts: Sequence[str], prompt_texts: Optional[Sequence[str]] = None,
                       prompt_audios: Optional[Sequence[np.ndarray]] = None, seed: Optional[int] = None, length_aware: bool = False):
        """Returns (list of {"gen": wav [1, 1, T], "gen_only_lm": wav}, list of decoded_codec [1, T, predict_nq]) like calling the
        reference once per utterance; utterances of one call share the engine passes.
        length_aware = True also shares the codec calls (one encode for the prompts, two decodes for the batch; see generate_many)."""
        m, nq = self.model, self.model.predict_nq
        n = len(texts)
        if length_aware:
            self._refuse_length_aware("generate_batch")
        continual_mode = self.continual and prompt_texts is not None and prompt_audios is not None
        cont, cont_lens = None, None
        if continual_mode:
            texts = [" ".join([p, t]).strip() for p, t in zip(prompt_texts, texts)]
            per = self._prompt_codecs(prompt_audios, length_aware)
            cont_lens = [int(c.shape[0]) for c in per]
            cont = torch.zeros((n, max(cont_lens), nq), dtype=torch.int64, device=m.device)
            for i, c in enumerate(per):
                cont[i, : c.shape[0]] = c
        text_outs, lens = self._encode_texts(texts)
        # 2. first codec groups, autoregressively
        tokens, out_lens = m.decode_codec_batch(text_outs, lens, self.max_length, self.sampling, cont, cont_lens, seed)
        excl = [(cl if self.exclude_prompt else 0) for cl in (cont_lens or [0] * n)] if continual_mode else [None] * n
        return self._synthesise(text_outs, lens, tokens, out_lens, excl, length_aware)

    # -- any number of prompts through a decoding session ---------------------------------------------------------------------------
    @torch.no_grad()
    def generate_many(self, texts: Sequence[str], prompt_texts: Optional[Sequence[str]] = None,
                      prompt_audios: Optional[Sequence[np.ndarray]] = None, slots: int = 16, seeds: Optional[Sequence[int]] = None,
                      step_n: Optional[int] = None, samples: int = 1, retries: int = 0, keep: str = "all", rules=None, prefill: int = 0,
                      length_aware: bool = False, queue: bool = False, elastic: bool = False):
        """Any number of prompts through a decoding session of `slots` slots kept full in arrival order (laura.drive_slots): a prompt
        starts as soon as a slot ends, nobody waits for the longest utterance of a batch.  Returns what generate_batch returns, in
        request order; per request the tokens are what a session of `slots` slots gives that prompt alone with its seed.  slots = 17 ..
        64 opens a wide session (LauraEngine.open_decode(wide=True)): more rows per decoding step, the same calls.

        samples = N > 1 draws N candidates per request (consecutive entries in arrival order; seeds [n][N], or drawn per candidate)
        and returns one list of N per request in both return values.  A candidate whose request has another candidate running in
        some slot is started from that slot (DecodeSlots.start_from: a copy of the prefix instead of a prefix pass); the two ways
        give the same bits, so every candidate is what its request listed N times as N requests with the same seeds gives, and
        which way a candidate started is purely a matter of cost.

        retries = R > 0 gives a candidate that reaches max_length without <eos> up to R second tries (laura.drive_retries): its slot
        is rewound in place to the first half of its tokens (DecodeSlots.rewind, keep = n_gen // 2: no prefix pass, no copy) and
        goes on with seed laura.retry_seed(seed, attempt); the last attempt is kept.  retries = 0 is the call without it.

        keep = "best" keeps one candidate per request: the session scores every step on the device (open_decode(score=True): the
        log-probability the LM gave its own picks), laura.pick_best ranks a request's N candidates -- <eos>-ended above run-aways,
        then the higher mean log-probability per step, ties to the lower index; with retries, a candidate's last attempt by the score
        of its whole final path -- and only the winners reach the fine predictor and the codec decoder.  Returns (rets, codecs,
        choice): rets[i], codecs[i] in the shape of samples = 1, choice[i] = (k, mean) of the candidate kept.  The candidates are,
        token for token, those of keep = "all" (the default: today's call, a session without scores) with the same seeds.

        rules = a ``laura.SamplingRules`` (temperature, min_length, top_p with an integer ``sampling``, the repeat rule) for every
        candidate: every start, start_from and rewind of the call carries it.  None is the call without rules.

        prefill = P in 1 .. 16 runs the prefix passes ahead of need, P different prompts per pass: a second, holding session of P
        rows (never stepped, no log-probabilities, the main session's max_positions) is filled through DecodeSlots.start_many
        whenever a slot needs a request that is not held -- that request and the next ones in arrival order (laura.prefill states the
        rule) -- and EVERY candidate starts by a device copy from its request's row (DecodeSlots.start_from(source=held)); a row is
        released once all `samples` candidates of its request have started.  Held rows are started greedy with max_length 1; what
        they sample is never used.  Texts are still encoded one request at a time.  A slot started by the copy is, bit for bit, the
        slot its own prefix pass gives, so the results are token for token and sample for sample those of prefill = 0 (the default:
        today's call) with the same seeds, whatever samples, retries, keep and rules; n requests cost ceil(n / P) prefix passes
        instead of n.  ``self.last_prefix_passes`` = {"main", "held"} says how many each session of the last call ran.

        length_aware = True runs the codec around the session as length-aware batches (``speech_lengths``: every row as if it were alone)
        instead of one call per utterance: the prompt recordings 16 per encode call in arrival order; the finished candidates sorted by
        the frames they decode (laura.tail_groups), 16 per fine-predictor call and per pair of decode calls.  Tokens are those of the
        default (False: today's call); waveforms are a length-aware row's, within the 1e-4 RMS bar of such a row against its own call.  A
        codec without length-aware calls (engine.ragged_refusal) raises before anything runs.

        step_n (default 1, with queue 16) is the decoding steps per status read-back (laura.drive_slots).

        queue = True (needs prefill >= 1, retries = 0 -- a rewind is the host's decision) takes the host out of the refill loop: the main
        session is a QUEUED one (open_decode(queue=, source=the holding session)), every candidate is a ticket, and ended slots are
        retired and refilled from the waiting tickets on the device inside the captured step, so step_n = 16 no longer lets an ended slot
        idle.  The host fills held rows in arrival order, submits `samples` tickets per row, refills rows whose tickets are all claimed
        (laura.queue_rows, laura.drive_queue) and collects results as they finish.  A ticket's slot is the slot
        start_from(source=held) gives, bit for bit, so the results are token for token those of queue = False (the default: the call
        as it is) with the same seeds, whatever samples, keep, rules, length_aware and slots.

        elastic = True opens the main session elastic (open_decode(elastic=True)): a decoding step runs the column blocks of 16 rows
        up to the highest running row, and running rows are moved down when that saves a block, so a session opened for the peak
        costs what its load needs.  Tokens and waveforms are those of elastic = False (the default: the call as it is) with the same
        seeds, whatever samples, retries, keep, rules, prefill and length_aware; up to 16 slots there is one block and nothing to
        save.  Refused with queue = True: a queued session claims its slots on the device and the host cannot know the busy rows.
        ``self.last_elastic`` = {"moves", "blocks"} of the last such call: rows moved, and {blocks: steps run at that width}."""
        from ..laura import CandidateRun, tail_groups
        m, nq = self.model, self.model.predict_nq
        n, N, R = len(texts), int(samples), int(retries)
        if N < 1:
            raise ValueError(f"generate_many: samples must be >= 1, got {samples}")
        if R < 0:
            raise ValueError(f"generate_many: retries must be >= 0, got {retries}")
        if keep not in ("all", "best"):
            raise ValueError(f"generate_many: keep must be \"all\" or \"best\", got {keep!r}")
        P = int(prefill)
        if not 0 <= P <= 16:
            raise ValueError(f"generate_many: prefill must be 0 (off) or 1 .. 16 rows, got {prefill}")
        best = keep == "best"
        if queue and P < 1:
            raise ValueError("generate_many: queue=True needs prefill >= 1: tickets name rows of the holding session")
        if queue and R > 0:
            raise ValueError(f"generate_many: queue=True goes with retries = 0, got {retries}: a rewind is decided by the host")
        if queue and elastic:
            raise ValueError("generate_many: elastic=True is refused with queue=True: a queued session claims its slots on the device, "
                             "the host cannot know the busy rows")
        step_n = (16 if queue else 1) if step_n is None else int(step_n)
        if length_aware:
            self._refuse_length_aware("generate_many")
        continual_mode = self.continual and prompt_texts is not None and prompt_audios is not None
        per = None
        if continual_mode:
            texts = [" ".join([p, t]).strip() for p, t in zip(prompt_texts, texts)]
            per = self._prompt_codecs(prompt_audios, length_aware)
        if seeds is None:
            seeds = [m._next_seed() for _ in range(n * N)]
        elif N == 1:
            seeds = [int(v) for v in seeds]
        else:
            if len(seeds) != n or any(len(row) != N for row in seeds):
                raise ValueError(f"generate_many: seeds must be [{n}][{N}]")
            seeds = [int(v) for row in seeds for v in row]
        if len(seeds) != n * N:
            raise ValueError(f"generate_many: {len(seeds)} seeds for {n} requests")

        def encode(i):
            text_outs, lens = self._encode_texts([texts[i]])
            return text_outs[0, : lens[0]], lens[0]

        run = CandidateRun(n, N, seeds, rules, encode, per)
        try:
            run.open(m, slots, P, queue, score=best, elastic=elastic)
            taken, choice = run.drive(self.max_length, self.sampling, R, step_n)
        finally:
            counts = run.close()
            if counts:
                self.last_prefix_passes = counts["prefix_passes"]
                if elastic:
                    self.last_elastic = counts["elastic"]
        # taken[j] is a candidate of request j // M: all N of every request, or with keep = "best" the winner only
        M = 1 if best else N
        first = [((int(c.shape[0]) if self.exclude_prompt else 0) if continual_mode else None) for c in (per or [None] * n)]
        ends = [run.encoded(j // M) + (t[0], t[1], first[j // M]) for j, t in enumerate(taken)]   # text_outs, len, tokens, len, first frame kept
        if length_aware:          # neighbours in decoded length share a call: a length-aware call computes over its group's common width
            groups = tail_groups([e[3] - (e[4] or 0) for e in ends], 16)
        else:
            groups = [list(range(i, min(i + 16, len(ends)))) for i in range(0, len(ends), 16)]
        done = [None] * len(ends)
        for g in groups:                                                    # finished utterances, 16 at a time, through the batch forms
            outs, lens, toks, out_lens, excl = (list(col) for col in zip(*(ends[j] for j in g)))
            text_outs = torch.zeros((len(g), max(lens), outs[0].shape[-1]), dtype=torch.float32, device=m.device)
            tokens = torch.zeros((len(g), max(max(out_lens), 1), nq), dtype=torch.int64, device=m.device)
            for b in range(len(g)):
                text_outs[b, : lens[b]] = outs[b]
                tokens[b, : out_lens[b]] = toks[b]
            for j, one in zip(g, zip(*self._synthesise(text_outs, lens, tokens, out_lens, excl, length_aware))):
                done[j] = one
        rets, codecs = [d[0] for d in done], [d[1] for d in done]          # candidate order, however they were grouped
        if best:
            return rets, codecs, choice
        if N == 1:
            return rets, codecs
        return [rets[i * N: (i + 1) * N] for i in range(n)], [codecs[i * N: (i + 1) * N] for i in range(n)]

    @staticmethod
    def from_pretrained(model_tag: Optional[str] = None, **kwargs: Optional[Any]):
        return Text2Audio(**kwargs)


def save_audio(wav: torch.Tensor, path: Union[Path, str], sample_rate: int, rescale: bool = False):
    """bin/text2audio_inference.py:231-239: like the codec CLI's save_audio with an extra 0.6 gain on the rescaled signal."""
    from ..io import save_audio as _save
    limit = 0.99
    w = torch.as_tensor(wav).detach().float().cpu()
    if rescale:
        mx = w.abs().max()
        w = w * min(limit / mx, 1) * 0.6
    _save(w, str(path), sample_rate, False)


def inference_func(output_dir: Optional[str] = None, batch_size: int = 1, dtype: str = "float32", ngpu: int = 1, seed: int = 0,
                   num_workers: int = 0, log_level: Union[int, str] = "INFO", key_file: Optional[str] = None,
                   config_file: Optional[str] = "config.yaml", model_file: Optional[str] = "model.pth", model_tag: Optional[str] = None,
                   allow_variable_data_keys: bool = True, streaming: bool = False, **kwargs):
    """bin/text2audio_inference.py:242-357: build the model once, return a function over `raw_inputs` = (text,) or
    (text, prompt_text, prompt_audio path | array).  The scp-driven streaming iterator of the reference's data layer is outside
    this engine's scope; `raw_inputs` (its modelscope pipeline form) is supported."""
    if ngpu > 1:
        raise NotImplementedError("only single GPU decoding is supported")
    logging.basicConfig(level=log_level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    torch.manual_seed(seed)
    my_model = Text2Audio.from_pretrained(model_tag=model_tag, config_file=config_file, model_file=model_file, device="cuda", dtype=dtype,
                                          **kwargs)

    def _forward(data_path_and_name_and_type=None, raw_inputs=None, output_dir_v2: Optional[str] = None, param_dict: Optional[dict] = None):
        if raw_inputs is None:
            raise NotImplementedError("pass raw_inputs=(text,) or (text, prompt_text, prompt_audio)")
        inputs = [raw_inputs[0]]
        if len(raw_inputs) == 3:
            audio = raw_inputs[2]
            if isinstance(audio, str):
                from ..io import read_wav, resample
                x, sr = read_wav(audio)
                want = my_model.codec_model.model.quantizer.sampling_rate
                if sr != want:
                    x = resample(torch.from_numpy(x)[None], sr, want)[0].numpy()
                audio = x[np.newaxis, :]
            else:
                audio = np.asarray(audio).squeeze()[None, :]
            inputs += [raw_inputs[1], audio]
        ret_val, _ = my_model(*inputs)
        out_path = output_dir_v2 if output_dir_v2 is not None else output_dir
        if out_path is not None:
            os.makedirs(out_path, exist_ok=True)
            for suffix, wave in ret_val.items():
                save_audio(wave[0], os.path.join(out_path, "utt1_" + suffix + ".wav"), rescale=True,
                           sample_rate=my_model.codec_model.model.quantizer.sampling_rate)
            return []
        return [{"key": "utt1", "value": ret_val}]

    return _forward


def inference(output_dir: Optional[str], batch_size: int = 1, dtype: str = "float32", ngpu: int = 1, seed: int = 0, num_workers: int = 0,
              log_level: Union[int, str] = "INFO", data_path_and_name_and_type=None, key_file: Optional[str] = None,
              config_file: Optional[str] = None, model_file: Optional[str] = None, model_tag: Optional[str] = None,
              allow_variable_data_keys: bool = True, streaming: bool = False, **kwargs):
    """bin/text2audio_inference.py:360-397."""
    pipeline = inference_func(output_dir=output_dir, batch_size=batch_size, dtype=dtype, ngpu=ngpu, seed=seed, num_workers=num_workers,
                              log_level=log_level, key_file=key_file, config_file=config_file, model_file=model_file, model_tag=model_tag,
                              allow_variable_data_keys=allow_variable_data_keys, streaming=streaming,
                              **{k: v for k, v in kwargs.items() if k not in ("raw_inputs", "mode", "gpuid_list")})
    return pipeline(data_path_and_name_and_type, raw_inputs=kwargs.get("raw_inputs", None))


def _int_or_float_or_bool(value: str):
    """funcodec/utils/types.py int_or_float_or_bool: "true"/"false" -> bool, "25" -> int, "0.8" -> float (the --sampling argument)."""
    v = value.strip().lower()
    if v in ("true", "false"):
        return v == "true"
    try:
        return int(v)
    except ValueError:
        return float(v)


def get_parser():
    """Same flags as the reference's CLI (bin/text2audio_inference.py:400-536); `python -m funcodec_amd.bin.text2audio_inference ...`
    accepts the command lines of egs/LibriTTS/text2speech_laura/demo.sh (minus --tokenize_to_phone true: pass phoneme strings)."""
    def str2bool(v):
        return str(v).lower() in ("true", "1", "yes")

    p = argparse.ArgumentParser(description="Text to audio generation", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--log_level", type=lambda x: x.upper(), default="INFO", choices=("CRITICAL", "ERROR", "WARNING", "INFO", "DEBUG", "NOTSET"))
    p.add_argument("--output_dir", type=str, required=False)
    p.add_argument("--ngpu", type=int, default=1)
    p.add_argument("--gpuid_list", type=str, default="0")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--dtype", default="float32", choices=["float16", "float32", "float64"])
    p.add_argument("--num_workers", type=int, default=0)
    g = p.add_argument_group("Input data related")
    g.add_argument("--data_path_and_name_and_type", type=str, required=False, action="append")
    g.add_argument("--raw_inputs", type=str, required=False, action="append")
    g.add_argument("--key_file", type=str, default=None)
    g.add_argument("--allow_variable_data_keys", type=str2bool, default=False)
    g = p.add_argument_group("The model configuration related")
    g.add_argument("--mode", type=str, default="inference mode")
    g.add_argument("--config_file", type=str)
    g.add_argument("--model_file", type=str)
    g.add_argument("--model_tag", type=str)
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--beam_size", type=int, default=1)
    g.add_argument("--text_emb_model", type=str, default="./exp/t5-base")
    g.add_argument("--sampling", type=_int_or_float_or_bool, default="true")
    g.add_argument("--codec_config_file", type=str, default=None)
    g.add_argument("--codec_model_file", type=str, default=None)
    g.add_argument("--continual", type=int, default=0)
    g.add_argument("--tokenize_to_phone", type=str2bool, default=False)
    g.add_argument("--exclude_prompt", type=str2bool, default=True)
    return p


def main(cmd=None):
    args = get_parser().parse_args(cmd)
    kwargs = vars(args)
    gpuid = kwargs["gpuid_list"].split(",")[0] or "0"          # one process drives one GPU (bin/text2audio_inference.py:545-556)
    if torch.cuda.is_available():
        torch.cuda.set_device(int(gpuid))
    inference(**kwargs)


if __name__ == "__main__":
    main()
