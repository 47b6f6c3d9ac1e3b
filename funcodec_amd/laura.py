"""Host side of the MI355X LauraTTS engine and the drop-in for the inference surface of the reference's ``LauraGenModel``
(funcodec/models/audio_generation/laura_model.py): ``encode`` (:186-202), ``decode_codec`` (:501-548), ``cal_codec_emb``
(:296-333), ``syn_audio`` (:550-567), plus batch forms of each (the reference generates one utterance at a time, re-scoring the
whole prefix per token; the engine keeps a KV cache, decodes up to 16 prompts per call and samples on the device).

PyTorch is used for device memory, streams and checkpoint I/O only; every arithmetic operation happens inside
libfuncodec_amd.so (HIP, gfx950).  There is no CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import logging
from collections.abc import Mapping
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .engine import EngineError, _on_device, _ptr
from .laura_config import LauraSpec, StackSpec, laura_spec_from_config


def _i32(vals: Sequence[int]):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def _u64(seed: int) -> int:
    return int(seed) & (2 ** 64 - 1)


def sampling_args(sampling: Union[bool, int, float]):
    """LauraGenModel.sampling_ids' `sampling` argument (laura_model.py:466-499) -> (mode, k, p) of fc_laura_decode_codec."""
    if isinstance(sampling, bool):
        return (1, 0, 0.0) if sampling else (0, 0, 0.0)
    if isinstance(sampling, int):
        return 2, int(sampling), 0.0
    if isinstance(sampling, float):
        return 3, 0, float(sampling)
    raise NotImplementedError(f"Not implemented for {type(sampling)} sampling")


class SamplingRules:
    """What shapes a decoding slot's draw beside ``sampling`` and ``seed`` (fc_laura_slots_set_rules states the semantics): the logits
    are divided by `temperature`; <eos> cannot be picked while the slot has generated fewer than `min_length` tokens; `top_p` cuts the
    top-k candidates of an integer ``sampling`` to their nucleus; with `repeat_window` W > 0, a drawn id that already stands at least
    `repeat_count` times among the group's last W generated tokens is drawn again from the whole distribution (drawing modes only).
    The defaults are the neutral rules: the session without rules, bit for bit."""

    __slots__ = ("temperature", "min_length", "top_p", "repeat_window", "repeat_count")

    def __init__(self, temperature: float = 1.0, min_length: int = 0, top_p: Optional[float] = None, repeat_window: int = 0,
                 repeat_count: int = 1):
        t = float(temperature)
        if not (0.0 < t <= float(np.finfo(np.float32).max) and float(np.float32(t)) > 0.0):
            raise ValueError(f"SamplingRules: temperature must be finite and > 0 (in float32), got {temperature!r}")
        for name, v in (("min_length", min_length), ("repeat_window", repeat_window), ("repeat_count", repeat_count)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"SamplingRules: {name} must be an integer, got {v!r}")
        if min_length < 0:
            raise ValueError(f"SamplingRules: min_length must be >= 0, got {min_length}")
        if top_p is not None and not 0.0 < float(np.float32(top_p)) <= 1.0:       # as the library sees it: 0 there means none
            raise ValueError(f"SamplingRules: top_p must lie in (0, 1] (None: no nucleus cut), got {top_p!r}")
        if not 0 <= repeat_window <= 256:
            raise ValueError(f"SamplingRules: repeat_window must lie in 0 .. 256 (0: off), got {repeat_window}")
        if repeat_window > 0 and not 1 <= repeat_count <= repeat_window:
            raise ValueError(f"SamplingRules: repeat_count must lie in 1 .. repeat_window = {repeat_window}, got {repeat_count}")
        if repeat_window == 0 and repeat_count < 1:
            raise ValueError(f"SamplingRules: repeat_count must be >= 1, got {repeat_count}")
        self.temperature, self.min_length = t, int(min_length)
        self.top_p = None if top_p is None else float(top_p)
        self.repeat_window, self.repeat_count = int(repeat_window), int(repeat_count)

    def args(self):
        """(temperature, min_length, top_p, repeat_window, repeat_count) of fc_laura_slots_set_rules; top_p 0 = none"""
        return self.temperature, self.min_length, 0.0 if self.top_p is None else self.top_p, self.repeat_window, self.repeat_count

    def __repr__(self):
        return (f"SamplingRules(temperature={self.temperature}, min_length={self.min_length}, top_p={self.top_p}, "
                f"repeat_window={self.repeat_window}, repeat_count={self.repeat_count})")


class LauraEngine:
    """One engine per (device, checkpoint); calls are serialised by the caller like a torch module's forward."""

    max_batch = 16

    def __init__(self, spec: LauraSpec, device: "torch.device | str | int" = "cuda:0", max_positions: int = 2048):
        self.lib = _lib.load()
        self.spec = spec
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if dev.type != "cuda":
            raise EngineError(f"funcodec_amd runs on MI355X (gfx950) only; device={device!r} has no implementation "
                              "(there is deliberately no CPU fallback)")
        self.device = torch.device("cuda", dev.index if dev.index is not None else 0)
        if int(max_positions) % 4 or not 16 <= int(max_positions) <= 2048:
            raise EngineError(f"max_positions must be a multiple of 4 in [16, 2048], got {max_positions}")
        a = _lib.FcLauraArch()
        a.abi_version = _lib.FC_ABI_VERSION
        a.input_size, a.vocab_size = spec.input_size, spec.vocab_size
        a.codebook_size, a.codebook_dim, a.num_quantizers = spec.codebook_size, spec.codebook_dim, spec.num_quantizers
        a.predict_nq = spec.predict_nq
        a.pos_emb_split = int(spec.pos_emb_type == "split")
        a.bidirectional_inputs = int(spec.bidirectional_inputs)
        a.max_positions = int(max_positions)
        for name in ("text_encoder", "codec_lm", "codec_encoder"):
            s: StackSpec = getattr(spec, name)
            d = getattr(a, name)
            d.idim, d.d_model, d.heads, d.ff, d.layers = s.idim, s.d_model, s.heads, s.ff, s.layers
            d.act = {"relu": 1, "swish": 2}[s.act]
            d.embed_relu = int(s.embed_relu)
            d.norm_style = int(s.norm_names[0] == "norm1")
        self.max_positions = int(max_positions)
        h = C.c_void_p()
        self._check(self.lib.fc_laura_create(C.byref(a), self.device.index, C.byref(h)))
        self._h = h
        self._ws: Optional[torch.Tensor] = None
        self._ws_need: Dict[tuple, int] = {}
        self._side = None

    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(self.lib.fc_last_error().decode("utf-8", "replace"))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.lib.fc_laura_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def expected_tensors(self) -> Dict[str, tuple]:
        out = {}
        name = C.c_char_p()
        dims = (C.c_int64 * 4)()
        for i in range(self.lib.fc_laura_num_weights(self._h)):
            nd = self.lib.fc_laura_weight_info(self._h, i, C.byref(name), dims)
            out[name.value.decode()] = tuple(int(dims[j]) for j in range(nd))
        return out

    @_on_device
    def load_state_dict(self, state: Dict[str, "torch.Tensor | np.ndarray"]) -> None:
        """Tolerant load like the reference's filter_state_dict (funcodec/torch_utils/load_pretrained_model.py:12-43): tensors
        outside the generation path (the model's training-time quantiser, codec_index_shift) are skipped; a MISSING tensor of the
        path is an error."""
        want = self.expected_tensors()
        for key, shape in want.items():
            if key not in state:
                raise EngineError(f"checkpoint is missing tensor {key} {shape}")
            t = torch.as_tensor(state[key]).detach().to("cpu", torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise EngineError(f"shape mismatch for {key}: checkpoint {tuple(t.shape)} vs architecture {shape}")
            dims = (C.c_int64 * 4)(*t.shape)
            self._check(self.lib.fc_laura_set_weight(self._h, key.encode(), C.c_void_p(t.data_ptr()), dims, t.dim()))
        skipped = [k for k in state if k not in want]
        if skipped:
            logging.info("funcodec_amd: skipped %d LauraTTS checkpoint tensors outside the generation path (e.g. %s)", len(skipped), skipped[0])
        self._check(self.lib.fc_laura_finalize(self._h))

    _fallbacks_seen = 0

    @property
    def persistent_step_fallbacks(self) -> int:
        """Calls of this engine whose persistent decoding step timed out and which were re-run on the kernel chain."""
        return int(self.lib.fc_laura_persistent_step_fallbacks(self._h))

    def set_persistent_step(self, on: bool) -> bool:
        """Decoding step as one persistent launch (default) or as the chain of one kernel per Linear / attention; returns whether the
        persistent form is in effect (False also when this model / device cannot run it)."""
        return self.lib.fc_laura_set_persistent_step(self._h, int(bool(on))) == 1

    def _workspace(self, B: int, L: int, Cmax: int, max_length: int) -> torch.Tensor:
        key = (B, L, Cmax, max_length)
        need = self._ws_need.get(key)
        if need is None:
            need = self._ws_need[key] = int(self.lib.fc_laura_workspace_bytes(self._h, B, L, Cmax, max_length))
        return self._grown(need)

    def _grown(self, need: int) -> torch.Tensor:
        """The engine's one scratch buffer, at least `need` bytes of it: it only grows, and the old buffer goes before the new one comes."""
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t, dtype) -> torch.Tensor:
        return torch.as_tensor(t).to(device=self.device, dtype=dtype).contiguous()

    # -- argument validation: the C side takes plain pointers and trusts these shapes ------------------------------------------------
    def _check_batch(self, what: str, B: int, cap: Optional[int] = None, **length_lists) -> None:
        if B < 1 or (cap is not None and B > cap):
            raise EngineError(f"{what}: batch of {B} utterances" + (f", the engine takes 1 .. {cap} per call" if cap else ""))
        for name, vals in length_lists.items():
            if vals is None:
                continue
            if len(vals) != B:
                raise EngineError(f"{what}: {name} has {len(vals)} entries for a batch of {B}")

    def _check_lens(self, what: str, name: str, vals: Sequence[int], upper: int, lower: int = 0) -> List[int]:
        out = [int(v) for v in vals]
        for v in out:
            if v < lower or v > upper:
                raise EngineError(f"{what}: {name} entry {v} outside [{lower}, {upper}]")
        return out

    def _check_text_outs(self, what: str, text_outs: torch.Tensor) -> None:
        if text_outs.dim() != 3 or text_outs.shape[-1] != self.spec.codebook_dim:
            raise EngineError(f"{what}: text_outs must be [B, L, {self.spec.codebook_dim}], got {tuple(text_outs.shape)}")

    # -- LauraGenModel.encode -------------------------------------------------------------------------------------------
    @_on_device
    def encode(self, text, text_lengths: Sequence[int]) -> torch.Tensor:
        """text: float [B, L, input_size] embeddings or int64 [B, L] token ids -> text_outs [B, L, codebook_dim]."""
        text = torch.as_tensor(text)
        ids = not text.is_floating_point()
        text = self._dev(text, torch.int64 if ids else torch.float32)
        if (ids and text.dim() != 2) or (not ids and (text.dim() != 3 or text.shape[-1] != self.spec.input_size)):
            raise EngineError(f"encode: text must be int64 [B, L] token ids or float [B, L, {self.spec.input_size}] embeddings, "
                              f"got {tuple(text.shape)}")
        B, L = text.shape[0], text.shape[1]
        text_lengths = list(text_lengths)
        self._check_batch("encode", B, text_lengths=text_lengths)
        text_lengths = self._check_lens("encode", "text_lengths", text_lengths, L, 1)
        out = torch.empty((B, L, self.spec.codebook_dim), dtype=torch.float32, device=self.device)
        ws = self._workspace(B, L, 0, 1)
        self._check(self.lib.fc_laura_encode(self._h, None if ids else _ptr(text), _ptr(text) if ids else None, _i32(text_lengths), B, L,
                                             _ptr(out), _ptr(ws), ws.numel(), self._stream()))
        return out

    # -- teacher-forced LM scores ---------------------------------------------------------------------------------------
    @_on_device
    def lm_logprobs(self, text_outs: torch.Tensor, text_lengths: Sequence[int], codec: Optional[torch.Tensor] = None,
                    codec_lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """log-softmax of the LM output at every position of [<sos>, text, <task>, codec]: [B, Tseq, vocab]."""
        text_outs = self._dev(text_outs, torch.float32)
        self._check_text_outs("lm_logprobs", text_outs)
        B, L = text_outs.shape[0], text_outs.shape[1]
        text_lengths = list(text_lengths)
        self._check_batch("lm_logprobs", B, text_lengths=text_lengths)
        text_lengths = self._check_lens("lm_logprobs", "text_lengths", text_lengths, L, 1)
        Cmax = 0
        if codec is not None:
            codec = self._dev(codec, torch.int64)
            if codec.dim() != 3 or codec.shape[0] != B or codec.shape[2] != self.spec.predict_nq:
                raise EngineError(f"lm_logprobs: codec must be int64 [{B}, Cmax, {self.spec.predict_nq}], got {tuple(codec.shape)}")
            Cmax = codec.shape[1]
            if codec_lengths is None:
                raise EngineError("lm_logprobs: codec given without codec_lengths")
            self._check_batch("lm_logprobs", B, codec_lengths=list(codec_lengths))
        cl = self._check_lens("lm_logprobs", "codec_lengths", list(codec_lengths), Cmax) if codec is not None else [0] * B
        Tseq = max(int(t) + 2 + int(c) for t, c in zip(text_lengths, cl))
        logp = torch.empty((B, Tseq, self.spec.lm_vocab), dtype=torch.float32, device=self.device)
        ws = self._workspace(B, L, Cmax, 1)
        self._check(self.lib.fc_laura_lm_logprobs(self._h, _ptr(text_outs), _i32(text_lengths), B, L, _ptr(codec),
                                                  _i32(cl) if codec is not None else None, Cmax, _ptr(logp), Tseq, _ptr(ws), ws.numel(),
                                                  self._stream()))
        return logp

    # -- LauraGenModel.decode_codec ----------------------------------------------------------------------------------------
    @_on_device
    def decode_codec(self, text_outs: torch.Tensor, text_lengths: Sequence[int], max_length: int = 30 * 25,
                     sampling: Union[bool, int, float] = True, seed: int = 0, continual: Optional[torch.Tensor] = None,
                     continual_lengths: Optional[Sequence[int]] = None, forced: Optional[torch.Tensor] = None,
                     return_logp: bool = False):
        """Batch form of decode_codec: returns (tokens [B, Cmax + max_length, nq] int64, lengths list[int]) and, with
        return_logp, the per-step log-probabilities [B, max_length, vocab]."""
        text_outs = self._dev(text_outs, torch.float32)
        self._check_text_outs("decode_codec", text_outs)
        B, L = text_outs.shape[0], text_outs.shape[1]
        text_lengths = list(text_lengths)
        self._check_batch("decode_codec", B, cap=self.max_batch, text_lengths=text_lengths)
        text_lengths = self._check_lens("decode_codec", "text_lengths", text_lengths, L, 1)
        if int(max_length) < 1:
            raise EngineError(f"decode_codec: max_length {max_length} < 1")
        nq = self.spec.predict_nq
        Cmax = 0
        if continual is not None:
            continual = self._dev(continual, torch.int64)
            if continual.dim() != 3 or continual.shape[0] != B or continual.shape[2] != nq:
                raise EngineError(f"decode_codec: continual must be int64 [{B}, Cmax, {nq}], got {tuple(continual.shape)}")
            Cmax = continual.shape[1]
            if continual_lengths is None:
                raise EngineError("decode_codec: continual given without continual_lengths")
            continual_lengths = list(continual_lengths)
            self._check_batch("decode_codec", B, continual_lengths=continual_lengths)
            continual_lengths = self._check_lens("decode_codec", "continual_lengths", continual_lengths, Cmax)
        mode, k, p = sampling_args(sampling)
        if forced is not None:
            forced = self._dev(forced, torch.int64)
            if tuple(forced.shape) != (B, int(max_length), nq):
                raise EngineError(f"decode_codec: forced must be int64 [{B}, {int(max_length)}, {nq}], got {tuple(forced.shape)}")
        tokens = torch.zeros((B, Cmax + max_length, nq), dtype=torch.int64, device=self.device)
        logp = torch.zeros((B, max_length, self.spec.lm_vocab), dtype=torch.float32, device=self.device) if return_logp else None
        out_lens = (C.c_int32 * B)()
        ws = self._workspace(B, L, Cmax, max_length)
        # the decoding loop replays a captured HIP graph of one step; the legacy default stream cannot be captured, so a caller on it
        # is moved to a stream of the engine's own (ordered after / before the caller's stream; the call synchronises at its end anyway)
        cur = torch.cuda.current_stream(self.device)
        run = cur
        if cur.cuda_stream == 0:
            if self._side is None:
                self._side = torch.cuda.Stream(self.device)
            run = self._side
            run.wait_stream(cur)
        self._check(self.lib.fc_laura_decode_codec(self._h, _ptr(text_outs), _i32(text_lengths), B, L, _ptr(continual),
                                                   _i32(continual_lengths) if continual is not None else None, Cmax, int(max_length),
                                                   mode, k, p, _u64(seed), _ptr(forced), _ptr(tokens), out_lens, _ptr(logp),
                                                   _ptr(ws), ws.numel(), C.c_void_p(run.cuda_stream)))
        if run is not cur:
            cur.wait_stream(run)
        nfb = int(self.lib.fc_laura_persistent_step_fallbacks(self._h))
        if nfb != self._fallbacks_seen:            # the call succeeded on the kernel chain after a hand-off timeout: said, not hidden
            self._fallbacks_seen = nfb
            import warnings
            warnings.warn("decode_codec: the persistent decoding step timed out at a hand-off (CUs held by another stream / process?); this call "
                          "was re-run on the kernel chain and later calls use it until set_persistent_step(True)", RuntimeWarning)
        lens = [int(v) for v in out_lens]
        return (tokens, lens, logp) if return_logp else (tokens, lens)

    def open_decode(self, slots: int, max_positions: Optional[int] = None, logp: bool = True, score: bool = False,
                    wide: bool = False, queue: Optional[int] = None, source: Optional["DecodeSlots"] = None,
                    elastic: bool = False) -> "DecodeSlots":
        """A decoding session of `slots` slots (1 .. 16, or 1 .. 64 with wide=True): prompts join and leave a running batch.  max_positions (default: the engine's)
        bounds text_len + 2 + prompt tokens + max_length of a slot and sizes the session's state; logp=False leaves out the per-step
        log-probabilities [slots, max_positions, vocab], the largest part of it.  score=True keeps one number per slot and step, the
        log-probability of the step's picks (DecodeSlots.score): [slots, max_positions] floats.  wide=True allows 1 .. 64 slots: the
        step's GEMV runs the rows beyond 16 as further column blocks of 16, each as the 16-row kernel computes it; up to 16 slots it
        is the session without the flag.

        queue=Q with source=a holding session of this engine opens a QUEUED session (``DecodeSlots.submit`` / ``claimed`` /
        ``collect``): tickets name a held row and wait on the device; inside every captured step ended slots retire into a result
        ring of Q entries and free slots claim the oldest tickets, so ``step(n)`` is n steps with the slots full and one read-back.
        It needs logp=False (no log-probability rows per ticket) and composes with score and wide.

        elastic=True opens an ``ElasticSlots``: a step costs the column blocks in use, not the slots opened.  The caller's slot numbers
        are logical; a slot that starts takes the lowest free row, ``step`` first moves running rows down when that saves a column
        block (``compact_plan``, ``DecodeSlots.move``) and the library launches the step over the blocks up to the highest running row.
        Results do not depend on the row, so nothing but the cost changes.  Up to 16 slots there is one block and the flag is inert;
        refused with queue= (the slots are claimed on the device, the host cannot know the busy rows)."""
        if elastic:
            if queue is not None or source is not None:
                raise EngineError("open_decode: elastic=True is refused with queue=: a queued session claims its slots on the device, "
                                  "the host cannot know the busy rows")
            return ElasticSlots(self, slots, max_positions, logp, score, wide)
        if queue is None and source is None:
            return DecodeSlots(self, slots, max_positions, logp, score, wide)
        return DecodeSlots(self, slots, max_positions, logp, score, wide, queue, source)

    # -- LauraGenModel.cal_codec_emb on one-hot probabilities (syn_audio) ---------------------------------------------------
    @_on_device
    def codec_emb(self, text_outs: torch.Tensor, text_lengths: Sequence[int], codec: torch.Tensor, codec_lengths: Sequence[int]) -> torch.Tensor:
        """codec int64 [B, Cmax, >= predict_nq] -> dense codec embeddings [B, Cmax, codebook_dim] (rows past each length zero)."""
        text_outs = self._dev(text_outs, torch.float32)
        codec = self._dev(codec, torch.int64)
        self._check_text_outs("codec_emb", text_outs)
        B, L = text_outs.shape[0], text_outs.shape[1]
        if codec.dim() != 3 or codec.shape[0] != B or codec.shape[2] < self.spec.predict_nq:
            raise EngineError(f"codec_emb: codec must be int64 [{B}, Cmax, >= {self.spec.predict_nq}], got {tuple(codec.shape)}")
        Cmax, cols = codec.shape[1], codec.shape[2]
        text_lengths, codec_lengths = list(text_lengths), list(codec_lengths)
        self._check_batch("codec_emb", B, text_lengths=text_lengths, codec_lengths=codec_lengths)
        text_lengths = self._check_lens("codec_emb", "text_lengths", text_lengths, L, 1)
        codec_lengths = self._check_lens("codec_emb", "codec_lengths", codec_lengths, Cmax)
        emb = torch.empty((B, Cmax, self.spec.codebook_dim), dtype=torch.float32, device=self.device)
        ws = self._workspace(B, L, Cmax, 1)
        self._check(self.lib.fc_laura_codec_emb(self._h, _ptr(text_outs), _i32(text_lengths), B, L, _ptr(codec), cols, _i32(codec_lengths),
                                                Cmax, _ptr(emb), _ptr(ws), ws.numel(), self._stream()))
        return emb

    # -- per-op entry point (tests) -----------------------------------------------------------------------------------------------
    @_on_device
    def linear(self, name: str, x: torch.Tensor, step_form: bool = False, gemv_stage: str = "auto") -> torch.Tensor:
        """One Linear of the model by name, full-sequence form or (``step_form``) the decoding step's GEMV.  ``gemv_stage`` (test
        hook, step form): "auto" as the decoding step runs it, "single" x staged in LDS in one piece, "windowed" in >= 2 windows."""
        x = self._dev(x, torch.float32)
        B, T, cin = x.shape
        want = self.expected_tensors()
        cout = want[name + ".weight"][0] if name + ".weight" in want else 3 * cin
        y = torch.empty((B, T, cout), dtype=torch.float32, device=self.device)
        ws = self._grown(4 * B * (T + 8) * (cin + cout) * 2 + (1 << 20))
        form = {"auto": 1, "single": 2, "windowed": 3}[gemv_stage] if step_form else 0
        self._check(self.lib.fc_laura_linear(self._h, name.encode(), _ptr(x), B, T, form, _ptr(y), _ptr(ws), ws.numel(), self._stream()))
        return y

    STACKS = ("text_encoder", "codec_lm", "codec_encoder")

    @_on_device
    def attention(self, stack: str, layer: int, qkv: torch.Tensor, lengths: Sequence[int], causal: bool = False,
                  bidir: Optional[Sequence[int]] = None) -> torch.Tensor:
        """The full-sequence rel-pos attention of one block on the caller's q / k / v (per-op test entry): qkv [B, T, 3 d] token-major
        with q | k | v along the feature axis -> the attention context [B, T, d] before linear_out.  Keys >= lengths[b] are masked;
        with ``causal``, rows and keys below ``bidir[b]`` see each other.  Nothing is masked on the way in or out: values at
        positions >= lengths[b] reach the kernel (keep them finite), and rows there come back as the kernel left them."""
        if stack not in self.STACKS:
            raise EngineError(f"attention: stack must be one of {self.STACKS}, got {stack!r}")
        d = getattr(self.spec, stack).d_model
        qkv = self._dev(qkv, torch.float32)
        if qkv.dim() != 3 or qkv.shape[-1] != 3 * d:
            raise EngineError(f"attention: qkv must be [B, T, {3 * d}], got {tuple(qkv.shape)}")
        B, T = qkv.shape[0], qkv.shape[1]
        lengths = list(lengths)
        self._check_batch("attention", B, lengths=lengths, bidir=None if bidir is None else list(bidir))
        lengths = self._check_lens("attention", "lengths", lengths, T, 1)
        bd = None if bidir is None else self._check_lens("attention", "bidir", list(bidir), T)
        ctx = torch.empty((B, T, d), dtype=torch.float32, device=self.device)
        ws = self._grown(4 * B * (T + 8) * 4 * d + (1 << 20))
        self._check(self.lib.fc_laura_attention(self._h, self.STACKS.index(stack), int(layer), _ptr(qkv), _i32(lengths),
                                                None if bd is None else _i32(bd), int(bool(causal)), B, T, _ptr(ctx), _ptr(ws), ws.numel(),
                                                self._stream()))
        return ctx

    @_on_device
    def step_block(self, layer: int, x: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: Sequence[int],
                   key_ranges: Optional[int] = None, wide: bool = False):
        """One block of the LM as the kernel chain's decoding step runs it (per-op test entry), on B <= 64 rows: x [B, d], the block's
        caches k_cache [B, d, Tcap] and v_cache [B, Tcap, d] in the engine's layouts, pos [B] the position of each row's new token
        (keys 0 .. pos[b]).  ``key_ranges`` 1 .. 8 key ranges per (row, head), None: the engine's rule; ``wide``: the GEMV
        instantiations over column blocks also at B <= 16.  Returns (new x [B, d], q [B, d], the raw partials
        [B, heads, key_ranges, dk + 2] -- per range the unnormalised context, the running max, the sum of exponentials --, k_cache
        and v_cache after the scatter at pos); the arguments are left unchanged."""
        s = self.spec.codec_lm
        d, H = s.d_model, s.heads
        x = self._dev(x, torch.float32).clone()
        kc = self._dev(k_cache, torch.float32).clone()
        vc = self._dev(v_cache, torch.float32).clone()
        if x.dim() != 2 or x.shape[1] != d or not 1 <= x.shape[0] <= 64:
            raise EngineError(f"step_block: x must be [1 .. 64, {d}], got {tuple(x.shape)}")
        B = x.shape[0]
        if kc.dim() != 3 or tuple(kc.shape[:2]) != (B, d) or tuple(vc.shape) != (B, kc.shape[2], d):
            raise EngineError(f"step_block: caches must be [{B}, {d}, Tcap] and [{B}, Tcap, {d}], got {tuple(kc.shape)} and {tuple(vc.shape)}")
        Tcap = kc.shape[2]
        pos = list(pos)
        self._check_batch("step_block", B, pos=pos)
        pos = self._check_lens("step_block", "pos", pos, min(Tcap, self.max_positions) - 1)
        NS = max(1, min(8, 256 // (B * H))) if key_ranges is None else int(key_ranges)      # None: a decoding step's own split (alloc_step_mem)
        if not 1 <= NS <= 8:
            raise EngineError(f"step_block: key_ranges must be 1 .. 8, got {key_ranges}")
        q = torch.empty((B, d), dtype=torch.float32, device=self.device)
        part = torch.empty((B, H, NS, d // H + 2), dtype=torch.float32, device=self.device)
        rows = 16 * ((B + 15) // 16)
        ws = self._grown(4 * rows * (2 * d + H * 8 * (d // H + 2) + s.ff) + (1 << 20))
        self._check(self.lib.fc_laura_step_block(self._h, int(layer), _ptr(x), _ptr(kc), _ptr(vc), _i32(pos), B, Tcap, NS, int(bool(wide)),
                                                 _ptr(q), _ptr(part), _ptr(ws), ws.numel(), self._stream()))
        return x, q, part, kc, vc

    SAMPLE_ROW_FIELDS = ("mode", "k", "p", "max_steps", "seed", "forced_on", "rng_row", "temperature", "min_length", "top_p",
                         "repeat_window", "repeat_count")

    @_on_device
    def sample(self, logits: torch.Tensor, tokens: torch.Tensor, step: Sequence[int], n_gen: Sequence[int], done: Sequence[int],
               pos: Sequence[int], tok_off: Sequence[int], *, rows: Optional[Sequence[dict]] = None, mode: int = 0, k: int = 0, p: float = 0.0,
               seed: int = 0, max_steps: Optional[int] = None, forced: Optional[torch.Tensor] = None, logp: bool = False, score: bool = False,
               row0: int = 0, nrows: int = 0, n_done: int = 0, fill: float = 0.0) -> dict:
        """The device sampler on the caller's logits and state (per-op test entry, fc_laura_sample): logits [B, V] float32, B <= 64,
        tokens [B, R, nq] int64 (the history the repeat rule reads; generated token g of row b is row tok_off[b] + g), the per-row state
        as integer lists.  Call form (``rows`` None): mode / k / p / seed / max_steps for every row, neutral rules, Philox row word =
        the batch row; ``forced`` is [B, max_steps, nq] and logp / score hold max_steps steps per row.  Table form: ``rows`` holds a
        dict per row with SAMPLE_ROW_FIELDS (missing rule fields are neutral, forced_on 1, rng_row 0); ``forced`` is [B, R, nq] and
        logp / score hold R steps.  ``row0`` / ``nrows``: only those rows (0: all).  The float outputs start filled with ``fill``.
        Returns a dict: tokens, step, n_gen, done, pos (lists), n_done, logp, score (None unless asked for), next_emb [B, D],
        xs [B, d_model]; the arguments are left unchanged."""
        spec = self.spec
        nq, V, D, dm = spec.predict_nq, spec.lm_vocab, spec.codebook_dim, spec.codec_lm.d_model
        logits = self._dev(logits, torch.float32)
        if logits.dim() != 2 or logits.shape[1] != V or not 1 <= logits.shape[0] <= 64:
            raise EngineError(f"sample: logits must be [1 .. 64, {V}], got {tuple(logits.shape)}")
        if not bool(torch.isfinite(logits).all()):
            raise EngineError("sample: logits must be finite")
        B = logits.shape[0]
        tokens = self._dev(tokens, torch.int64).clone()
        if tokens.dim() != 3 or tokens.shape[0] != B or tokens.shape[2] != nq or tokens.shape[1] < 1:
            raise EngineError(f"sample: tokens must be [{B}, R, {nq}], got {tuple(tokens.shape)}")
        R = tokens.shape[1]
        state = {"step": list(step), "n_gen": list(n_gen), "done": list(done), "pos": list(pos), "tok_off": list(tok_off)}
        self._check_batch("sample", B, **state)
        if not (0 <= int(row0) and 0 <= int(nrows) and int(row0) + (int(nrows) or B) <= B):
            raise EngineError(f"sample: row0 = {row0}, nrows = {nrows} outside the {B} rows")
        io = _lib.FcLauraSampleIo()
        if rows is None:
            if max_steps is None:
                raise EngineError("sample: the call form needs max_steps")
            steps = int(max_steps)
            per_row = [int(max_steps)] * B
            io.rows = None
            io.mode, io.k, io.p, io.seed, io.max_steps = int(mode), int(k), float(p), _u64(seed), int(max_steps)
            modes = [int(mode)] * B
        else:
            rows = list(rows)
            if len(rows) != B:
                raise EngineError(f"sample: {len(rows)} table rows for {B} rows")
            steps = R
            table = (_lib.FcLauraSampleRow * B)()
            neutral = dict(k=0, p=0.0, seed=0, forced_on=1, rng_row=0, temperature=1.0, min_length=0, top_p=0.0, repeat_window=0, repeat_count=1)
            for b, r in enumerate(rows):
                extra = set(r) - set(self.SAMPLE_ROW_FIELDS)
                if extra or "mode" not in r or "max_steps" not in r:
                    raise EngineError(f"sample: row {b}: fields must be mode, max_steps and any of {self.SAMPLE_ROW_FIELDS}, got {sorted(r)}")
                full = dict(neutral, **r)
                SamplingRules(full["temperature"], full["min_length"], full["top_p"] or None, full["repeat_window"], full["repeat_count"])
                for name in self.SAMPLE_ROW_FIELDS:
                    v = full[name]
                    setattr(table[b], name, _u64(v) if name == "seed" else float(v) if name in ("p", "temperature", "top_p") else int(v))
            io.rows = table
            per_row = [int(r["max_steps"]) for r in rows]
            modes = [int(r["mode"]) for r in rows]
        if any(m not in (0, 1, 2, 3) for m in modes):
            raise EngineError(f"sample: sampling modes must be 0 .. 3, got {modes}")
        for b in range(B):
            if not 1 <= per_row[b] <= steps:
                raise EngineError(f"sample: row {b}: max_steps {per_row[b]} outside 1 .. {steps}")
            if min(state[n][b] for n in state) < 0:
                raise EngineError(f"sample: row {b}: negative state")
            if state["tok_off"][b] + state["n_gen"][b] > R or state["tok_off"][b] + per_row[b] > R:
                raise EngineError(f"sample: row {b}: tok_off + n_gen and tok_off + max_steps must not exceed the {R} token rows")
        if forced is not None:
            forced = self._dev(forced, torch.int64)
            if tuple(forced.shape) != (B, steps, nq):
                raise EngineError(f"sample: forced must be [{B}, {steps}, {nq}], got {tuple(forced.shape)}")
            if int(forced.min()) < 0 or int(forced.max()) > spec.codebook_size:
                raise EngineError(f"sample: forced ids must lie in 0 .. {spec.codebook_size}")
        new = lambda *shape: torch.full(shape, float(fill), dtype=torch.float32, device=self.device)
        lp = new(B, steps, V) if logp else None
        sc = new(B, steps) if score else None
        nemb, xs = new(B, D), new(B, dm)
        host = {n: _i32(v) for n, v in state.items()}
        nd = _i32([n_done])
        io.logits = _ptr(logits)
        io.step, io.n_gen, io.done, io.pos, io.tok_off, io.n_done = host["step"], host["n_gen"], host["done"], host["pos"], host["tok_off"], nd
        io.tokens, io.forced = _ptr(tokens), None if forced is None else _ptr(forced)
        io.logp, io.score = None if lp is None else _ptr(lp), None if sc is None else _ptr(sc)
        io.next_emb, io.xs = _ptr(nemb), _ptr(xs)
        io.B, io.R, io.row0, io.nrows = B, R, int(row0), int(nrows)
        ws = self._grown(1 << 20)
        self._check(self.lib.fc_laura_sample(self._h, C.byref(io), _ptr(ws), ws.numel(), self._stream()))
        out = {n: list(host[n]) for n in ("step", "n_gen", "done", "pos")}
        out.update(tokens=tokens, n_done=int(nd[0]), logp=lp, score=sc, next_emb=nemb, xs=xs)
        return out


SLOT_STATES ={1: "running", 2: "done", 3: "failed"}       # fc_laura_slots_step's done_out; 0 = free (not reported)


class DecodeSlots:
    """A decoding session (``LauraEngine.open_decode``): S slots (1 .. 16, or 1 .. 64 with ``wide=True``) of ``decode_codec``, each
    holding one utterance at a time.  ``start``
    puts a prompt into a slot while the others are in the middle of theirs, ``step`` advances every running slot by the same number of
    decoding steps, ``take`` returns what an ended slot generated and frees it.  A slot depends on nothing but its own prompt and
    parameters; a session of one slot is ``decode_codec`` on the prompt alone, bit for bit."""

    MAX_SLOTS, MAX_SLOTS_WIDE = 16, 64
    MAX_QUEUE = 65536
    queue: Optional[int] = None             # a session without a queue, unless __init__ says otherwise
    source: Optional["DecodeSlots"] = None

    def __init__(self, engine: "LauraEngine", slots: int, max_positions: Optional[int] = None, logp: bool = True, score: bool = False,
                 wide: bool = False, queue: Optional[int] = None, source: Optional["DecodeSlots"] = None):
        self.engine, self.lib, self.device = engine, engine.lib, engine.device
        self.slots = int(slots)
        self.wide = bool(wide)
        if self.wide and not 1 <= self.slots <= self.MAX_SLOTS_WIDE:
            raise EngineError(f"a wide decoding session has 1 .. {self.MAX_SLOTS_WIDE} slots, got {slots}")
        #: result entries of a queued session (None: a session without a queue) and the holding session its tickets name rows of
        self.queue = None if queue is None else int(queue)
        self.source = source
        if self.queue is None and source is not None:
            raise EngineError("open_decode: source= goes with queue= (start_from(source=...) takes a source per call)")
        if self.queue is not None:
            if logp:
                raise EngineError("open_decode: queue= needs logp=False: log-probability rows are not kept per ticket")
            if not isinstance(source, DecodeSlots):
                raise EngineError(f"open_decode: queue= needs source=, the holding DecodeSlots its tickets name rows of, got {type(source).__name__}")
            if source.engine is not engine:
                raise EngineError("open_decode: queue=: the source session belongs to another engine (other weights: its prefix is not this engine's)")
            if source.queue is not None:
                raise EngineError("open_decode: queue=: the source session is itself queued (it holds no prompts)")
            if not 1 <= self.queue <= self.MAX_QUEUE:
                raise EngineError(f"open_decode: queue must be 1 .. {self.MAX_QUEUE} result entries, got {queue}")
            limit = self.MAX_SLOTS_WIDE if self.wide else self.MAX_SLOTS
            if not 1 <= self.slots <= limit:
                raise EngineError(f"a {'wide ' if self.wide else ''}decoding session has 1 .. {limit} slots, got {slots}")
        self._submitted = self._claimed = self._finished = self._failed = self._collected = 0
        self._ticket_max_length: Dict[int, int] = {}
        self.max_positions = int(engine.max_positions if max_positions is None else max_positions)
        self.with_logp = bool(logp)
        self.with_score = bool(score)
        self._h = None
        self._max_length = [0] * max(self.slots, 0)
        self._status = (C.c_int32 * max(self.slots, 1))()
        self._n_gen = (C.c_int32 * max(self.slots, 1))()
        #: prefix passes this session has run: one per ``start``, one per ``start_many`` whatever its n, none for start_from / fork
        self.prefix_passes = 0
        self._open()

    @_on_device
    def _open(self):
        eng = self.engine
        if self.queue is not None:
            nbytes = int(self.lib.fc_laura_slots_state_bytes_queued(eng._h, self.slots, self.max_positions, int(self.with_score), self.queue))
        elif self.wide and self.slots > self.MAX_SLOTS:                 # up to 16 slots a wide session is the one below, call for call
            nbytes = int(self.lib.fc_laura_slots_state_bytes_wide(eng._h, self.slots, self.max_positions, int(self.with_logp),
                                                                  int(self.with_score)))
        elif self.with_score:
            nbytes = int(self.lib.fc_laura_slots_state_bytes_scored(eng._h, self.slots, self.max_positions, int(self.with_logp), 1))
        else:                                                            # the session without scores: the call it always was
            nbytes = int(self.lib.fc_laura_slots_state_bytes(eng._h, self.slots, self.max_positions, int(self.with_logp)))
        #: everything the session carries between calls (fc_laura_slots_state_bytes): one allocation
        self.state = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=self.device) if nbytes else None
        if self.state is not None:
            torch.cuda.current_stream(self.device).synchronize()      # fc_laura_slots_create writes with copies that this stream does not order
        h = C.c_void_p()
        if self.queue is not None:
            eng._check(self.lib.fc_laura_slots_create_queued(eng._h, self.slots, self.max_positions, int(self.with_score), self.queue,
                                                             self.source._handle(), _ptr(self.state), nbytes, C.byref(h)))
        elif self.wide and self.slots > self.MAX_SLOTS:
            eng._check(self.lib.fc_laura_slots_create_wide(eng._h, self.slots, self.max_positions, int(self.with_logp), int(self.with_score),
                                                           _ptr(self.state), nbytes, C.byref(h)))
        elif self.with_score:
            eng._check(self.lib.fc_laura_slots_create_scored(eng._h, self.slots, self.max_positions, int(self.with_logp), 1, _ptr(self.state),
                                                             nbytes, C.byref(h)))
        else:
            eng._check(self.lib.fc_laura_slots_create(eng._h, self.slots, self.max_positions, int(self.with_logp), _ptr(self.state), nbytes,
                                                      C.byref(h)))
        self._h = h

    def free(self) -> None:
        """End the session and release its state."""
        if getattr(self, "_h", None):
            self.lib.fc_laura_slots_destroy(self._h)
            self._h = None
        self.state = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise EngineError("decoding session: used after free()")
        return self._h

    def _run_stream(self):
        # the step is a captured HIP graph; the legacy default stream cannot be captured (see LauraEngine.decode_codec)
        eng = self.engine
        cur = torch.cuda.current_stream(self.device)
        run = cur
        if cur.cuda_stream == 0:
            if eng._side is None:
                eng._side = torch.cuda.Stream(self.device)
            run = eng._side
            run.wait_stream(cur)
        return cur, run

    @contextlib.contextmanager
    def _launching(self):
        """The stream a call's launches go to (``_run_stream``); the caller's stream waits for it when the call is out, refused or not."""
        cur, run = self._run_stream()
        try:
            yield C.c_void_p(run.cuda_stream)
        finally:
            if run is not cur:
                cur.wait_stream(run)

    def _token_rows(self, what: str, name: str, t, rows: Optional[int] = None) -> torch.Tensor:
        """`t` as int64 [n, nq] on the device, a leading 1 squeezed; `rows`: the n the call requires (None: any, "C")."""
        nq = self.engine.spec.predict_nq
        t = self.engine._dev(t, torch.int64)
        if t.dim() == 3 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 2 or t.shape[1] != nq or (rows is not None and t.shape[0] != rows):
            raise EngineError(f"{what}: {name} must be int64 [{'C' if rows is None else rows}, {nq}], got {tuple(t.shape)}")
        return t

    def _refuse_queued(self, call: str) -> None:
        if self.queue is not None:
            raise EngineError(f"decoding session: {call}: a queued session is fed by its queue only (submit, collect)")

    def _need_queue(self, call: str) -> None:
        if self.queue is None:
            raise EngineError(f"decoding session: {call}: the session was opened without a queue (open_decode(queue=, source=))")

    @_on_device
    def submit(self, row: int, max_length: int = 30 * 25, sampling: Union[bool, int, float] = True, seed: int = 0,
               rules: Optional[SamplingRules] = None) -> int:
        """A ticket into the queue of a queued session: the prompt that row `row` of the source session holds, with the ticket's own
        max_length, sampling, seed and rules (no forced tokens).  Returns the ticket number, 0, 1, 2, ... in submit order; tickets are
        claimed in that order, by free slots in ascending order, at the head of every decoding step.  One small launch, no
        synchronisation.  The slot that claims the ticket is the slot ``start_from(slot, row, source=held, ...)`` gives, bit for bit,
        so the result is a function of the row and these parameters alone.  Refused, naming the ticket and the row and changing
        nothing: a row that holds no prompt, prefix + max_length beyond this session's max_positions, sampling and rules that do
        not agree, and a queue whose `queue` result entries are all waiting, running or uncollected (``collect`` frees them)."""
        self._need_queue("submit")
        h = self._handle()
        row, max_length = int(row), int(max_length)
        if rules is not None and not isinstance(rules, SamplingRules):
            raise ValueError(f"decode session submit: ticket {self._submitted} (row {row}): rules must be a SamplingRules or None, "
                             f"got {type(rules).__name__}")
        mode, k, p = sampling_args(sampling)
        t, n, tp, w, r = (rules or SamplingRules()).args()
        ticket = C.c_int32(-1)
        with self._launching() as stream:
            self.engine._check(self.lib.fc_laura_slots_submit(h, row, max_length, mode, k, p, _u64(seed), t, n, tp, w, r,
                                                              C.byref(ticket), stream))
        self._submitted += 1
        self._ticket_max_length[int(ticket.value)] = max_length
        return int(ticket.value)

    def _queue_status(self) -> None:
        v = [C.c_int64(0) for _ in range(5)]
        self._slot_tickets = (C.c_int32 * max(self.slots, 1))()
        self.engine._check(self.lib.fc_laura_slots_queue_status(self._handle(), *[C.byref(x) for x in v], self._slot_tickets))
        self._submitted, self._claimed, self._finished, self._failed, self._collected = (int(x.value) for x in v)

    @property
    def claimed(self) -> int:
        """Tickets claimed so far, as the last ``step`` read it back (monotone): every ticket below this number has left the queue, so
        a held row may be overwritten once ``claimed`` covers all its tickets."""
        self._need_queue("claimed")
        return self._claimed

    @property
    def finished(self) -> int:
        """Tickets retired into the result ring so far, as the last ``step`` read it back (failed ones not counted)."""
        self._need_queue("finished")
        return self._finished

    @property
    def submitted(self) -> int:
        self._need_queue("submitted")
        return self._submitted

    @property
    def pending(self) -> int:
        """Tickets waiting or running: ``step`` has work while this is not 0."""
        self._need_queue("pending")
        return self._submitted - self._finished - self._failed

    def slot_tickets(self) -> Dict[int, int]:
        """{slot: the ticket it runs}, as the last ``step`` read it back."""
        self._need_queue("slot_tickets")
        t = getattr(self, "_slot_tickets", None)
        return {} if t is None else {i: int(t[i]) for i in range(self.slots) if int(t[i]) >= 0}

    @_on_device
    def collect(self, score_rows: bool = False) -> list:
        """The results the last ``step`` calls retired, out of the ring with one synchronisation for all of them; their entries are
        free afterwards.  [(ticket, tokens [len, nq] int64 = prompt tokens + generated ones, len, score)], failed tickets first, then
        in the order of finishing.  score: None for a session without scores, else (sum, count, ended_on_eos) as ``DecodeSlots.score``
        gives it, or with score_rows (row float32 [max_positions] on the host, count, end) as ``score_row`` does.  A ticket that ran
        in a step call whose persistent step timed out is failed: (ticket, None, 0, None), never tokens."""
        self._need_queue("collect")
        h = self._handle()
        self._queue_status()
        cap = self._finished + self._failed - self._collected
        if cap <= 0:
            return []
        nq, R = self.engine.spec.predict_nq, self.max_positions
        i32 = lambda: (C.c_int32 * cap)()
        tickets, states, lens, gens, ends = i32(), i32(), i32(), i32(), i32()
        tokens = torch.zeros((cap, R, nq), dtype=torch.int64, device=self.device)
        rows = torch.zeros((cap, R), dtype=torch.float32) if self.with_score else None
        torch.cuda.current_stream(self.device).synchronize()          # the copies run on the session's stream
        n = C.c_int32(0)
        self.engine._check(self.lib.fc_laura_slots_collect(h, cap, tickets, states, lens, gens, ends, _ptr(tokens),
                                                           C.c_void_p(rows.data_ptr()) if rows is not None else None, C.byref(n)))
        out = []
        for j in range(int(n.value)):
            t = int(tickets[j])
            self._ticket_max_length.pop(t, None)
            if int(states[j]) != 2:
                out.append((t, None, 0, None))
                continue
            count, end = int(gens[j]) + (1 if int(ends[j]) == 2 else 0), int(ends[j])
            score = None
            if rows is not None:
                score = (rows[j].clone(), count, end) if score_rows else (float(rows[j, :count].double().sum()), count, end == 2)
            out.append((t, tokens[j, : int(lens[j])].clone(), int(lens[j]), score))
        self._queue_status()
        return out

    #: rows moved so far (``move``; an elastic session's ``step`` moves rows by itself)
    moves = 0

    def _phys(self, slot: int) -> int:
        """The row of the session that slot `slot` lies in: the slot itself (an ``ElasticSlots`` keeps a table)."""
        return int(slot)

    @property
    def blocks(self) -> int:
        """Column blocks of 16 rows the last ``step`` launched (0: it had no running slot and launched nothing)."""
        return int(self.lib.fc_laura_slots_step_blocks(self._handle()))

    @_on_device
    def move(self, pairs) -> None:
        """[(src, dst), ...] rows of the session: after the call row dst IS row src -- a running slot goes on as if it had never moved,
        an ended one is taken from dst -- and src is free.  Everything the session keeps per slot is copied in one launch; nothing is
        computed again, so the bits of the moved slot do not change.  Stream-ordered, no synchronisation.  Refused, naming the slot
        and changing nothing: a row outside the session, named twice or on both sides, a source that holds no utterance, a destination
        that is not free, a queued session."""
        self._refuse_queued("move")
        h = self._handle()
        pairs = [(int(a), int(b)) for a, b in pairs]
        if not pairs:
            raise EngineError("decoding session: move: no moves")
        with self._launching() as stream:
            self.engine._check(self.lib.fc_laura_slots_move(h, len(pairs), _i32([a for a, _ in pairs]), _i32([b for _, b in pairs]), stream))
        for a, b in pairs:
            self._max_length[b], self._n_gen[b], self._status[b] = self._max_length[a], self._n_gen[a], self._status[a]
            self._n_gen[a], self._status[a] = 0, 0
        self.moves += len(pairs)

    def _set_rules(self, slot: int, rules: Optional[SamplingRules]) -> None:
        """`rules` (None: the neutral ones) as the rules the next start / start_from / fork into `slot` writes: per call, like sampling
        and seed.  Nothing on the device changes here."""
        if rules is not None and not isinstance(rules, SamplingRules):
            raise ValueError(f"decode session: slot {slot}: rules must be a SamplingRules or None, got {type(rules).__name__}")
        t, n, p, w, r = (rules or SamplingRules()).args()
        self.engine._check(self.lib.fc_laura_slots_set_rules(self._handle(), int(slot), t, n, p, w, r))

    @_on_device
    def start(self, slot: int, text_outs: torch.Tensor, text_len: int, max_length: int = 30 * 25, sampling: Union[bool, int, float] = True,
              seed: int = 0, continual: Optional[torch.Tensor] = None, forced: Optional[torch.Tensor] = None,
              rules: Optional[SamplingRules] = None) -> None:
        """One prompt into `slot`: text_outs [L, D] or [1, L, D] (rows < text_len are used), continual int64 [C, nq] prompt tokens, forced
        int64 [max_length, nq], rules a ``SamplingRules`` (None: neutral).  A running slot's utterance is abandoned.  A refused call
        changes nothing for any slot."""
        self._refuse_queued("start")
        eng = self.engine
        h = self._handle()
        text_outs = eng._dev(text_outs, torch.float32)
        if text_outs.dim() == 2:
            text_outs = text_outs.unsqueeze(0)
        eng._check_text_outs("decode session start", text_outs)
        text_len, max_length = int(text_len), int(max_length)
        if text_outs.shape[0] != 1 or not 1 <= text_len <= text_outs.shape[1]:
            raise EngineError(f"decode session start: slot {slot}: one prompt [L, D] with 1 <= text_len <= L, got {tuple(text_outs.shape)}, text_len {text_len}")
        if max_length < 1:
            raise EngineError(f"decode session start: slot {slot}: max_length {max_length} < 1")
        text = text_outs[0, :text_len].contiguous()
        cont_len = 0
        if continual is not None:
            continual = self._token_rows(f"decode session start: slot {slot}", "continual", continual)
            cont_len = continual.shape[0]
            continual = continual.contiguous() if cont_len else None
        if forced is not None:
            forced = self._token_rows(f"decode session start: slot {slot}", "forced", forced, max_length)
        mode, k, p = sampling_args(sampling)
        self._set_rules(slot, rules)
        ws = eng._grown(int(self.lib.fc_laura_slots_workspace_bytes(h, text_len, cont_len)))
        with self._launching() as stream:
            eng._check(self.lib.fc_laura_slots_start(h, int(slot), _ptr(text), text_len, _ptr(continual), cont_len, max_length, mode, k, p,
                                                     _u64(seed), _ptr(forced), _ptr(ws), ws.numel(), stream))
        self._max_length[int(slot)] = max_length
        self.prefix_passes += 1

    START_MANY_KEYS = ("text_outs", "text_len", "max_length", "sampling", "seed", "continual", "rules")

    def _many_rows(self, requests) -> List[tuple]:
        """The argument checks of ``start_many`` that need no device: [(slot, request dict with ``start``'s defaults filled in)]."""
        what = "decode session start_many"
        items = list(requests.items()) if isinstance(requests, Mapping) else [tuple(r) for r in requests]
        if not items:
            raise EngineError(f"{what}: no requests")
        rows, seen = [], set()
        for slot, req in items:
            slot = int(slot)
            if not 0 <= slot < self.slots:
                raise EngineError(f"{what}: slot {slot} outside 0 .. {self.slots - 1}")
            if slot in seen:
                raise EngineError(f"{what}: slot {slot} is named twice")
            seen.add(slot)
            if not isinstance(req, Mapping):
                raise EngineError(f"{what}: slot {slot}: a request is a dict of {', '.join(self.START_MANY_KEYS)}")
            unknown = sorted(set(req) - set(self.START_MANY_KEYS))
            if unknown:
                hint = " (start_many takes no forced tokens: start forces)" if "forced" in unknown else ""
                raise EngineError(f"{what}: slot {slot}: unknown key(s) {unknown}{hint}")
            if "text_outs" not in req or "text_len" not in req:
                raise EngineError(f"{what}: slot {slot}: text_outs and text_len are required")
            r = dict(max_length=30 * 25, sampling=True, seed=0, continual=None, rules=None)
            r.update(req)
            if int(r["max_length"]) < 1:
                raise EngineError(f"{what}: slot {slot}: max_length {int(r['max_length'])} < 1")
            rows.append((slot, r))
        if len(rows) > min(16, self.slots):
            raise EngineError(f"{what}: slot {rows[min(16, self.slots)][0]}: at most min(16, slots) = {min(16, self.slots)} prompts per call, "
                              f"got {len(rows)}")
        return rows

    @_on_device
    def start_many(self, requests) -> None:
        """n different prompts into n slots with ONE prefix pass: `requests` maps slot -> dict(text_outs, text_len, max_length, sampling,
        seed, continual, rules) with ``start``'s meanings and defaults (or is a sequence of such (slot, dict) pairs); 1 <= n <=
        min(16, slots), the slots distinct, in any order.  Every named slot is, bit for bit, the slot ``start`` gives for its prompt and
        parameters -- how a slot was started changes its cost, never its result.  No forced tokens here: ``start`` forces.  A running
        slot's utterance is abandoned.  A refused call names the slot and changes nothing for any slot."""
        self._refuse_queued("start_many")
        eng, nq = self.engine, self.engine.spec.predict_nq
        h = self._handle()
        rows = self._many_rows(requests)
        n = len(rows)
        texts, conts = [], []
        for slot, r in rows:
            t = eng._dev(r["text_outs"], torch.float32)
            if t.dim() == 3 and t.shape[0] == 1:
                t = t[0]
            text_len = int(r["text_len"])
            if t.dim() != 2 or t.shape[1] != eng.spec.codebook_dim or not 1 <= text_len <= t.shape[0]:
                raise EngineError(f"decode session start_many: slot {slot}: one prompt [L, {eng.spec.codebook_dim}] with 1 <= text_len <= L, "
                                  f"got {tuple(t.shape)}, text_len {text_len}")
            texts.append(t[:text_len])
            c = r["continual"]
            if c is not None:
                c = self._token_rows(f"decode session start_many: slot {slot}", "continual", c)
            conts.append(c)
        L = max(t.shape[0] for t in texts)
        Cmax = max((c.shape[0] for c in conts if c is not None), default=0)
        text = torch.zeros((n, L, eng.spec.codebook_dim), dtype=torch.float32, device=self.device)
        cont = torch.zeros((n, Cmax, nq), dtype=torch.int64, device=self.device) if Cmax else None
        for b, (t, c) in enumerate(zip(texts, conts)):
            text[b, : t.shape[0]] = t
            if c is not None and c.shape[0]:
                cont[b, : c.shape[0]] = c
        modes = [sampling_args(r["sampling"]) for _, r in rows]
        for slot, r in rows:
            self._set_rules(slot, r["rules"])
        ws = eng._grown(int(self.lib.fc_laura_slots_start_many_workspace_bytes(h, n, L, Cmax)))
        slots_a = _i32([slot for slot, _ in rows])
        tl_a = _i32([t.shape[0] for t in texts])
        cl_a = _i32([0 if c is None else c.shape[0] for c in conts]) if cont is not None else None
        ml_a = _i32([int(r["max_length"]) for _, r in rows])
        mode_a, k_a = _i32([m[0] for m in modes]), _i32([m[1] for m in modes])
        p_a = (C.c_float * n)(*[m[2] for m in modes])
        seed_a = (C.c_uint64 * n)(*[_u64(r["seed"]) for _, r in rows])
        with self._launching() as stream:
            eng._check(self.lib.fc_laura_slots_start_many(h, n, slots_a, _ptr(text), tl_a, L, _ptr(cont), cl_a, Cmax, ml_a, mode_a, k_a, p_a,
                                                          seed_a, _ptr(ws), ws.numel(), stream))
        for slot, r in rows:
            self._max_length[slot] = int(r["max_length"])
        self.prefix_passes += 1

    @_on_device
    def start_from(self, dst: int, src: int, max_length: Optional[int] = None, sampling: Union[bool, int, float] = True, seed: int = 0,
                   forced: Optional[torch.Tensor] = None, rules: Optional[SamplingRules] = None,
                   source: Optional["DecodeSlots"] = None) -> None:
        """The prompt that slot `src` holds (text and continual tokens) into slot `dst` with `dst`'s own max_length (default: the
        source's), sampling, seed, rules and forced tokens: a device copy of the source's prefix instead of a prefix pass.  `dst` is, bit for
        bit, the slot that ``start`` gives for the same prompt and parameters; `src` is not disturbed, may be running or ended (not yet
        taken), and may itself come from a start_from.  A running `dst` is abandoned.  A refused call changes nothing for any slot."""
        self._refuse_queued("start_from")
        eng = self.engine
        h = self._handle()
        dst, src = int(dst), int(src)
        if source is self:
            source = None
        if source is not None and not isinstance(source, DecodeSlots):
            raise EngineError(f"decode session start_from: slot {dst}: source must be a DecodeSlots or None, got {type(source).__name__}")
        held = self if source is None else source
        src = held._phys(src)
        if max_length is None:
            if not 0 <= src < held.slots:
                raise EngineError(f"decode session start_from: source slot {src} outside 0 .. {held.slots - 1}")
            max_length = held._max_length[src]
        max_length = int(max_length)
        if forced is not None:
            forced = self._token_rows(f"decode session start_from: slot {dst}", "forced", forced, max_length)
        mode, k, p = sampling_args(sampling)
        self._set_rules(dst, rules)
        with self._launching() as stream:
            if source is None:
                eng._check(self.lib.fc_laura_slots_start_from(h, dst, src, max_length, mode, k, p, _u64(seed), _ptr(forced),
                                                              stream))
            else:                           # the prompt lies in another session of this engine; both sessions run on this stream
                eng._check(self.lib.fc_laura_slots_start_from_session(h, dst, source._handle(), src, max_length, mode, k, p,
                                                                      _u64(seed), _ptr(forced), stream))
        self._max_length[dst] = max_length

    @_on_device
    def fork(self, dst: int, src: int, keep: Optional[int] = None, max_length: Optional[int] = None,
             sampling: Union[bool, int, float] = True, seed: int = 0, rules: Optional[SamplingRules] = None) -> None:
        """Slot `dst` holds slot `src`'s utterance as it stood after its first `keep` generated tokens (default: all that the last
        ``step`` reported, ``n_gen(src)``) and goes on from there with its own sampling, seed, rules (None: neutral, whatever the
        source's) and max_length (default: the source's):
        a device copy of the source's cache positions, tokens and log-probability rows, no prefix pass and no decoding step.  With the
        source's own sampling and seed `dst` ends exactly as the source does; with any other, its per-step log-probabilities are those
        of ``start`` with its final tokens forced.  `src` is not disturbed, may be running or ended (by <eos> or by length, not yet
        taken) and may itself come from a fork or a start_from; keep = 0 is ``start_from``.  A running `dst` is abandoned.  A refused
        call changes nothing for any slot."""
        self._refuse_queued("fork")
        h = self._handle()
        dst, src = int(dst), int(src)
        if not 0 <= src < self.slots:
            raise EngineError(f"decode session fork: source slot {src} outside 0 .. {self.slots - 1}")
        src = self._phys(src)
        keep = -1 if keep is None else int(keep)
        if keep < -1:
            raise EngineError(f"decode session fork: slot {dst}: keep {keep} < 0")
        if max_length is not None and int(max_length) < 1:
            raise EngineError(f"decode session fork: slot {dst}: max_length {int(max_length)} < 1")
        max_length = 0 if max_length is None else int(max_length)         # 0: the source's, which the library knows
        mode, k, p = sampling_args(sampling)
        self._set_rules(dst, rules)
        with self._launching() as stream:
            self.engine._check(self.lib.fc_laura_slots_fork(h, dst, src, keep, max_length, mode, k, p, _u64(seed), stream))
        self._max_length[dst] = max_length or self._max_length[src]
        self._n_gen[dst] = self._n_gen[src] if keep < 0 else keep

    def rewind(self, slot: int, keep: int, max_length: Optional[int] = None, sampling: Union[bool, int, float] = True, seed: int = 0,
               rules: Optional[SamplingRules] = None) -> None:
        """``fork(slot, slot, keep, ...)``: the slot goes back to its first `keep` generated tokens in place and goes on from there
        with the given sampling, seed, rules and max_length (default: its own).  An ended slot (not yet taken) runs again; one that ended on
        <eos>, rewound to keep = n_gen, draws its ending again."""
        self._refuse_queued("rewind")
        self.fork(slot, slot, keep, max_length, sampling, seed, rules)

    def n_gen(self, slot: int) -> int:
        """Tokens slot `slot` has generated, as the last ``step`` reported it (after a fork or rewind: the tokens kept)."""
        slot = int(slot)
        if not 0 <= slot < self.slots:
            raise EngineError(f"decoding session: slot {slot} outside 0 .. {self.slots - 1}")
        return int(self._n_gen[slot])

    @_on_device
    def step(self, n: int = 16) -> Dict[int, str]:
        """n decoding steps for every running slot; {slot: "running" | "done" | "failed"} for every slot that holds an utterance."""
        h = self._handle()
        before = self.engine.persistent_step_fallbacks
        with self._launching() as stream:
            self.engine._check(self.lib.fc_laura_slots_step(h, int(n), self._status, self._n_gen, stream))
        if self.queue is not None:                  # the queue's counters and the slots' tickets, out of the same read-back
            self._queue_status()
        if self.engine.persistent_step_fallbacks != before:
            self.engine._fallbacks_seen = self.engine.persistent_step_fallbacks
            import warnings
            warnings.warn("decoding session: the persistent decoding step timed out at a hand-off (CUs held by another stream / process?); the "
                          "running slots are failed (start them again) and the session stays on the kernel chain", RuntimeWarning)
        return {i: SLOT_STATES[int(self._status[i])] for i in range(self.slots) if int(self._status[i]) in SLOT_STATES}

    @_on_device
    def score_row(self, slot: int):
        """The score row of a slot that holds an utterance, running or ended: (row float32 [max_positions] on the host, count, end).
        row[j] is the log-probability of generated step j's picks: the sum over the groups of log softmax(logits[group])[pick], the
        probability the reference's ``sampling_ids`` gives the pick before any top-k / nucleus truncation, a forced token counting as
        the pick.  It is a function of the step's logits and picks only: the same bits in every sampling mode.  count = the terms
        written: the tokens generated as the last ``step`` reported (after a fork or rewind: the tokens kept), plus the ending step of
        a slot that ended on <eos>; the row is zero behind them.  end: 0 running, 1 ended by length, 2 ended on <eos>.  Refused, with
        the slot named, for a session opened without score=True."""
        self._refuse_queued("score_row")
        h = self._handle()
        slot = int(slot)
        if not 0 <= slot < self.slots:
            raise EngineError(f"decoding session: slot {slot} outside 0 .. {self.slots - 1}")
        if not self.with_score:
            raise EngineError(f"decoding session: slot {slot}: the session was opened without scores (open_decode(score=True))")
        row = torch.zeros(self.max_positions, dtype=torch.float32)
        torch.cuda.current_stream(self.device).synchronize()          # the copy runs on the session's stream
        count, end = C.c_int32(0), C.c_int32(0)
        self.engine._check(self.lib.fc_laura_slots_score(h, slot, C.c_void_p(row.data_ptr()), row.numel(), C.byref(count), C.byref(end)))
        return row, int(count.value), int(end.value)

    def score(self, slot: int):
        """(sum, count, ended_on_eos) of an ended slot, which stays as it is: the float64 sum, on the host, of the fp32 terms
        [0, count) of ``score_row``.  ``pick_best`` ranks these.  Refused for a slot that has not ended, and for a session without
        scores."""
        row, count, end = self.score_row(slot)
        if end == 0:
            raise EngineError(f"decoding session: slot {int(slot)} has not ended")
        return float(row[:count].double().sum()), count, end == 2

    @_on_device
    def take(self, slot: int, return_logp: bool = False, return_score: bool = False):
        """What an ended slot generated: (tokens [len, nq] int64 = prompt tokens + generated ones, len) and, with return_logp, the
        per-step log-probabilities [max_length, vocab]; with return_score, (sum, count, ended_on_eos) as ``score`` gives it is appended.
        The slot is free afterwards.  Refused for a slot that has not ended."""
        self._refuse_queued("take")
        h = self._handle()
        slot = int(slot)
        if not 0 <= slot < self.slots:
            raise EngineError(f"decoding session: slot {slot} outside 0 .. {self.slots - 1}")
        scored = self.score(slot) if return_score else None            # ahead of the take, which frees the slot
        nq = self.engine.spec.predict_nq
        cap = self.max_positions
        tokens = torch.zeros((cap, nq), dtype=torch.int64, device=self.device)
        logp = None
        if return_logp:
            logp = torch.zeros((max(self._max_length[slot], 1), self.engine.spec.lm_vocab), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()          # the copies run on the session's stream
        n = C.c_int32(0)
        self.engine._check(self.lib.fc_laura_slots_take(h, slot, _ptr(tokens), cap, C.byref(n), _ptr(logp)))
        tokens = tokens[: n.value].clone()
        out = (tokens, int(n.value), logp) if return_logp else (tokens, int(n.value))
        return out + (scored,) if return_score else out


def compact_plan(busy_rows: Sequence[int], S: int, held: Sequence[int] = ()) -> List[tuple]:
    """The compaction rule of an elastic session, a plain function of which rows are busy: the fewest moves [(src, dst), ...], highest
    busy rows into lowest free rows, that bring the busy (running) rows of a session of S rows into the fewest column blocks of 16.
    Empty when that does not lower the block count.  `held` rows are occupied but not busy (ended, not taken): they are no
    destination and do not hold the width up, so they stay where they are."""
    busy = sorted(set(int(r) for r in busy_rows))
    kept = set(int(r) for r in held) - set(busy)
    if not busy:
        return []
    if busy[0] < 0 or busy[-1] >= S or any(not 0 <= r < S for r in kept):
        raise ValueError(f"compact_plan: a row outside 0 .. {S - 1}")
    now = busy[-1] // 16 + 1
    for nb in range(1, now):                       # the fewest blocks whose rows, less the held ones, take every busy row
        top = min(S, 16 * nb)
        if top - sum(1 for r in kept if r < top) >= len(busy):
            free = [r for r in range(top) if r not in kept and r not in busy]
            return list(zip([r for r in reversed(busy) if r >= top], free))
    return []


class RowTable:
    """Logical slot -> physical row of an elastic session: a slot that starts takes the lowest free row and keeps it until it is
    taken (``release``) or moved (``moved``)."""

    def __init__(self, S: int):
        self.S = int(S)
        self.row: Dict[int, int] = {}

    def free_rows(self) -> List[int]:
        used = set(self.row.values())
        return [r for r in range(self.S) if r not in used]

    def place(self, slot: int) -> tuple:
        """(row, new): the row `slot` holds, else the lowest free one, which it holds from now on."""
        if slot in self.row:
            return self.row[slot], False
        self.row[slot] = self.free_rows()[0]          # S logical slots over S rows: one is free
        return self.row[slot], True

    def release(self, slot: int) -> None:
        self.row.pop(slot, None)

    def moved(self, pairs) -> None:
        at = {r: s for s, r in self.row.items()}
        for src, dst in pairs:
            if src in at:
                self.row[at[src]] = dst

    def slot_of(self) -> Dict[int, int]:
        return {r: s for s, r in self.row.items()}


class ElasticSlots(DecodeSlots):
    """``open_decode(..., elastic=True)``: a DecodeSlots whose step is as wide as the slots in use.  Slot numbers are the caller's own
    (logical); the session keeps the table slot -> row.  A slot that starts (``start``, ``start_many``, a ``start_from`` / ``fork``
    destination) takes the lowest free row, ``take`` frees it, and ``step`` first applies ``compact_plan`` to the running rows
    (``move``) -- ended rows that are not yet taken stay put and do not hold the width up -- then steps the column blocks up to the
    highest running row (fc_laura_slots_set_elastic).  A slot's bits depend neither on its row nor on its neighbours, and a cut step
    is the full step on its rows, so every result is the non-elastic session's, bit for bit.  ``blocks``: the blocks of the last step;
    ``moves``: rows moved so far; ``rows()``: the table; ``blocks_hist``: {blocks: steps run at that width}."""

    elastic = True

    def __init__(self, engine: "LauraEngine", slots: int, max_positions: Optional[int] = None, logp: bool = True, score: bool = False,
                 wide: bool = False):
        self._table = RowTable(max(int(slots), 0))
        self._running = set()
        self.blocks_hist: Dict[int, int] = {}
        super().__init__(engine, slots, max_positions, logp, score, wide)
        self.engine._check(self.lib.fc_laura_slots_set_elastic(self._h, 1))

    def rows(self) -> Dict[int, int]:
        """{slot: row} of every slot that holds a row."""
        return dict(self._table.row)

    def _logical(self, slot: int) -> int:
        slot = int(slot)
        if not 0 <= slot < self.slots:
            raise EngineError(f"decoding session: slot {slot} outside 0 .. {self.slots - 1}")
        return slot

    def _phys(self, slot: int) -> int:
        slot = self._logical(slot)
        if slot not in self._table.row:
            raise EngineError(f"decoding session: slot {slot} holds no utterance (free or never started)")
        return self._table.row[slot]

    def _placed(self, slot: int, call, *args, **kw):
        slot = self._logical(slot)
        row, new = self._table.place(slot)
        try:
            out = call(row, *args, **kw)
        except Exception as err:
            if new:
                self._table.release(slot)
            if isinstance(err, EngineError):          # the library names the row: say whose it is
                raise EngineError(f"slot {slot} (row {row}): {err}") from err
            raise
        self._running.add(row)
        return out

    def start(self, slot: int, *args, **kw) -> None:
        return self._placed(slot, super().start, *args, **kw)

    def start_many(self, requests) -> None:
        rows = self._many_rows(requests)              # the checks on the caller's slot numbers, before any row is taken
        new, phys = [], []
        for slot, r in rows:
            row, fresh = self._table.place(slot)
            phys.append((row, r))
            if fresh:
                new.append(slot)
        try:
            super().start_many(phys)
        except Exception as err:
            for slot in new:
                self._table.release(slot)
            if isinstance(err, EngineError):          # the library names the row: say whose it is
                where = ", ".join(f"slot {slot} in row {row}" for (slot, _), (row, _) in zip(rows, phys))
                raise EngineError(f"{err} ({where})") from err
            raise
        self._running.update(row for row, _ in phys)

    def start_from(self, dst: int, src: int, *args, **kw) -> None:
        return self._placed(dst, lambda row: super(ElasticSlots, self).start_from(row, src, *args, **kw))

    def fork(self, dst: int, src: int, *args, **kw) -> None:
        return self._placed(dst, lambda row: super(ElasticSlots, self).fork(row, src, *args, **kw))

    def move(self, pairs) -> None:
        """``DecodeSlots.move`` on ROWS; the table follows, so every slot keeps its number."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        super().move(pairs)
        self._table.moved(pairs)
        at = dict(pairs)
        self._running = {at.get(r, r) for r in self._running}

    def n_gen(self, slot: int) -> int:
        return super().n_gen(self._phys(slot))

    def step(self, n: int = 16) -> Dict[int, str]:
        held = set(self._table.row.values()) - self._running
        plan = compact_plan(sorted(self._running), self.slots, sorted(held))
        if plan:
            self.move(plan)
        status = super().step(n)
        nb = self.blocks
        if nb:
            self.blocks_hist[nb] = self.blocks_hist.get(nb, 0) + int(n)
        self._running = {r for r, st in status.items() if st == "running"}
        at = self._table.slot_of()
        return {at[r]: st for r, st in status.items() if r in at}

    def score_row(self, slot: int):
        return super().score_row(self._phys(slot))

    def take(self, slot: int, return_logp: bool = False, return_score: bool = False):
        row = self._phys(slot)
        scored = self.score(slot) if return_score else None            # ahead of the take, which frees the row
        out = super().take(row, return_logp, False)
        self._table.release(int(slot))
        self._running.discard(row)
        return out + (scored,) if return_score else out


def refill(pending: Sequence[int], free_slots: Sequence[int]) -> List[tuple]:
    """The refill policy of a decoding session, a plain function of (arrival order, which slots are free): the waiting requests, in
    arrival order, go to the free slots in ascending order.  Returns [(slot, request)]."""
    return list(zip(sorted(free_slots), pending))


def prefill(need: int, held: Dict[int, int], rows: int, n_requests: int, fresh: int) -> List[tuple]:
    """Which requests a holding session of `rows` rows prefills, in ONE prefix pass, when a slot needs request `need`: a plain function
    of (the request needed, `held` = row -> the request it holds and has not released, `fresh` = the lowest request never prefilled).
    Nothing, if `need` is held.  Otherwise `need` itself, then the requests from max(need + 1, fresh) on in arrival order that are not
    held, as many as rows are free, into the free rows in ascending order; if no row is free the row holding the request needed last
    (the highest number) gives way -- it is prefilled again when its turn comes.  Returns [(row, request)], `need` first.

    In arrival order (the drivers' order without failures) need == fresh at every miss and all rows are free then, so request i is
    prefilled by pass i // rows and n requests cost ceil(n / rows) passes.  A request that comes back after its row was released (a
    failed slot's) is prefilled once more, with fresh requests beside it."""
    if not 0 <= need < n_requests:
        raise ValueError(f"prefill: request {need} outside 0 .. {n_requests - 1}")
    if rows < 1:
        raise ValueError(f"prefill: a holding session has at least one row, got {rows}")
    if need in held.values():
        return []
    free = sorted(r for r in range(rows) if r not in held)
    if not free:
        free = [max(held, key=lambda r: held[r])]
    want = [need] + [q for q in range(max(need + 1, fresh), n_requests) if q not in held.values()]
    return list(zip(free, want))


def queue_rows(held: Dict[int, int], claimed: int, rows: int) -> List[int]:
    """Which rows of the holding session of a QUEUED session may be filled with new prompts, a plain function of (`held` = row -> the
    number behind the last ticket submitted for the prompt the row holds, `claimed` = DecodeSlots.claimed): in ascending order, the
    rows that hold nothing and the rows all of whose tickets have been claimed (tickets are claimed in submit order, so tickets
    < held[row] claimed means claimed >= held[row]).  A claim copies the row's prefix inside the step that claims, so a claimed
    ticket no longer reads the row; a row with a ticket still waiting is never returned."""
    if rows < 1:
        raise ValueError(f"queue_rows: a holding session has at least one row, got {rows}")
    if claimed < 0:
        raise ValueError(f"queue_rows: claimed must be >= 0, got {claimed}")
    for row, end in held.items():
        if not 0 <= row < rows:
            raise ValueError(f"queue_rows: row {row} outside 0 .. {rows - 1}")
        if end < 0:
            raise ValueError(f"queue_rows: row {row}: ticket bound {end} < 0")
    return [r for r in range(rows) if r not in held or claimed >= held[r]]


def tail_groups(lengths: Sequence[int], rows: int = 16) -> List[List[int]]:
    """Which finished candidates go through the fine predictor and the codec decoder together (``generate_many(length_aware=True)``),
    a plain function of their lengths: the indices sorted by length, ties to the lower index, cut into groups of at most `rows`.  A
    length-aware call computes over its group's common width, so neighbours in length share a call; results do not depend on it."""
    if rows < 1:
        raise ValueError(f"tail_groups: a group has at least one row, got {rows}")
    order = sorted(range(len(lengths)), key=lambda i: (int(lengths[i]), i))
    return [order[i: i + rows] for i in range(0, len(order), rows)]


def pack_windows(x: torch.Tensor, lo: Sequence[int], hi: Sequence[int]) -> torch.Tensor:
    """x [B, T, ...] -> [B, max(hi - lo), ...] with x[j, lo[j]: hi[j]] at the front of row j and zeros behind: the rows of a
    length-aware decoder call start at frame 0 (a non-causal decoder run on a window is not a window of the decoder's output)."""
    if not (len(lo) == len(hi) == x.shape[0]):
        raise ValueError(f"pack_windows: one window per row ({x.shape[0]}), got {len(lo)} and {len(hi)}")
    for j, (a, b) in enumerate(zip(lo, hi)):
        if not 0 <= a <= b <= x.shape[1]:
            raise ValueError(f"pack_windows: row {j}: window [{a}, {b}) outside 0 .. {x.shape[1]}")
    out = x.new_zeros((x.shape[0], max((b - a for a, b in zip(lo, hi)), default=0)) + tuple(x.shape[2:]))
    for j, (a, b) in enumerate(zip(lo, hi)):
        out[j, : b - a] = x[j, a: b]
    return out


class HeldPrompts:
    """The bookkeeping of ``generate_many(prefill=P)`` around ``prefill``, no device in it: which row of the holding session holds
    which request, and when a row is released -- once all `samples` candidates of its request have started."""

    def __init__(self, rows: int, n_requests: int, samples: int = 1):
        self.rows, self.n_requests, self.samples = int(rows), int(n_requests), int(samples)
        self.held: Dict[int, int] = {}          # row -> request
        self.started: Dict[int, int] = {}       # request -> candidates started from its row so far
        self.fresh = 0
        self.passes = 0

    def need(self, request: int) -> List[tuple]:
        """[(row, request)] to prefill in one pass before `request` can be started ([]: it is held); the rows are taken here."""
        plan = prefill(request, self.held, self.rows, self.n_requests, self.fresh)
        for row, q in plan:
            self.held[row] = q
            self.started[q] = 0
            self.fresh = max(self.fresh, q + 1)
        if plan:
            self.passes += 1
        return plan

    def row_of(self, request: int) -> int:
        for row, q in self.held.items():
            if q == request:
                return row
        raise KeyError(f"request {request} is not held")

    def start(self, request: int) -> int:
        """A candidate of `request` starts from its row (returned); the row is released behind the last one."""
        row = self.row_of(request)
        self.started[request] += 1
        if self.started[request] >= self.samples:
            del self.held[row]
        return row


def drive_slots(session, slots: int, n_requests: int, start, step_n: int = 1) -> list:
    """Run n_requests through a session of `slots` slots kept full in arrival order: ``start(slot, request)`` puts request number
    `request` into a slot; ``session.step(step_n)`` and ``session.take(slot)`` are a DecodeSlots' (or a stand-in's).  A slot that ended
    is taken and refilled at the next step boundary; a failed slot's request goes back to the head of the queue.  Returns the takes in
    request order.

    step_n = 1 looks after every step.  Then no request starts later than it would in ANY schedule that starts requests in arrival
    order on `slots` rows -- lock-step decode_codec calls of `slots` rows among them -- so the session never runs more steps than
    those (by induction over the requests: when the other schedule starts request j, fewer than `slots` of the earlier requests
    are still running in it, and here each of them started no later, so a slot is free here too).  A larger step_n saves a status
    read-back per step and ends slots up to step_n - 1 steps late."""
    pending = list(range(n_requests))
    owner: Dict[int, int] = {}
    free = list(range(slots))
    results = [None] * n_requests
    retries = 0
    while pending or owner:
        for slot, req in refill(pending, free):
            start(slot, req)
            owner[slot] = req
            pending.remove(req)
            free.remove(slot)
        status = session.step(step_n)
        failed = []
        for slot in sorted(owner):
            st = status.get(slot)
            if st == "running":
                continue
            req = owner.pop(slot)
            free.append(slot)
            if st == "done":
                results[req] = session.take(slot)
            else:                                   # failed: start revives the slot; the session is on the kernel chain from here on
                retries += 1
                if retries > n_requests:
                    raise EngineError(f"decoding session: request {req} failed again after the session fell back to the kernel chain")
                failed.append(req)
        pending[:0] = sorted(failed)
    return results


def drive_queue(session, rows: int, n_requests: int, samples: int, fill, submit, step_n: int = 16) -> list:
    """`samples` candidates of each of n_requests requests through a QUEUED session whose holding session has `rows` rows: the host
    fills rows and submits tickets, the device refills the slots.  ``fill([(row, request)])`` prefills those rows in one prefix pass
    (DecodeSlots.start_many on the holding session); ``submit(row, candidate)`` returns the ticket of candidate = request * samples + k;
    ``session.step`` / ``claimed`` / ``collect`` are a queued DecodeSlots' (or a stand-in's).  Requests go to rows in arrival order; the
    rows ``queue_rows`` gives are refilled once at least min(requests left, max(1, rows // 2)) of them may be -- a pass per freed row
    would bring back the serial prefix passes -- and a row never before all its tickets are claimed.  Between two looks the session runs
    step_n steps; while requests are left to prefill and the slots without a ticket (``session.slots`` - ``session.slot_tickets()``) could
    take every waiting ticket, it runs ONE, so that a session wider than the holding session fills in a few steps instead of rows per
    step_n.  Returns the collected (tokens, len[, score]) per candidate, in candidate order.  A failed ticket (a timed-out persistent
    step) raises: its row may be gone."""
    total = n_requests * samples
    held: Dict[int, int] = {}               # row -> the number behind the last ticket of the request it holds
    owner: Dict[int, int] = {}              # ticket -> candidate
    results = [None] * total
    fresh, got, sent = 0, 0, 0
    while got < total:
        left = n_requests - fresh
        free = queue_rows(held, session.claimed, rows)
        if left and len(free) >= min(left, max(1, rows // 2)):
            batch = list(zip(free, range(fresh, n_requests)))
            fill(batch)
            for row, request in batch:
                for k in range(samples):
                    ticket = submit(row, request * samples + k)
                    owner[ticket] = request * samples + k
                    held[row] = ticket + 1
                    sent += 1
            fresh += len(batch)
        idle = session.slots - len(session.slot_tickets())
        session.step(1 if fresh < n_requests and sent - session.claimed <= idle else step_n)
        for ticket, tokens, n, score in session.collect():
            if tokens is None:
                raise EngineError(f"decoding session: ticket {ticket} failed (the persistent decoding step timed out); the session is on the "
                                  "kernel chain from here on: run the call again")
            results[owner.pop(ticket)] = (tokens, n) if score is None else (tokens, n, score)
            got += 1
    return results


def drive_samples(session, slots: int, n_requests: int, samples: int, start, start_from, step_n: int = 1) -> list:
    """`samples` candidates of each of n_requests requests through a session of `slots` slots: candidate number c = request * samples
    + k, in that (arrival) order through ``drive_slots``, whose policy is unchanged.  A candidate whose request already has a candidate
    running in some slot is started from that slot, ``start_from(slot, source_slot, c)``; otherwise ``start(slot, c)`` runs the prefix
    pass.  The two ways give the same bits (DecodeSlots.start_from), so which one a candidate gets is purely a matter of cost, never
    of result: a request whose candidates never overlap in time simply pays a prefix pass each.  Returns the takes, one list of
    `samples` per request."""
    held: Dict[int, int] = {}               # slot -> the candidate running in it (drive_slots' own `owner`, seen from the callbacks)

    class _Watched:                         # the session as drive_slots uses it: a slot that stopped running holds nothing any more
        def step(self, n):
            status = session.step(n)
            for slot in list(held):
                if status.get(slot) != "running":
                    del held[slot]
            return status

        def take(self, slot):
            return session.take(slot)

    def begin(slot, c):
        held.pop(slot, None)
        src = next((s for s in sorted(held) if held[s] // samples == c // samples), None)
        if src is None:
            start(slot, c)
        else:
            start_from(slot, src, c)
        held[slot] = c

    taken = drive_slots(_Watched(), slots, n_requests * samples, begin, step_n)
    return [taken[i * samples: (i + 1) * samples] for i in range(n_requests)]


RETRY_SEED_STRIDE = 0x9E3779B97F4A7C15


def retry_seed(seed: int, attempt: int) -> int:
    """The seed of attempt number `attempt` (0 = the candidate's own) of a candidate that is rewound after ending by length."""
    return (int(seed) + int(attempt) * RETRY_SEED_STRIDE) % (2 ** 64)


def drive_retries(session, slots: int, n_requests: int, samples: int, retries: int, max_length: int, start, start_from, rewind,
                  step_n: int = 1) -> list:
    """``drive_samples`` with second tries.  A candidate whose slot ends by length -- ``session.n_gen(slot) >= max_length``, so no
    <eos> -- is not taken: ``rewind(slot, c, keep, attempt)`` sends it back to its first keep = n_gen // 2 tokens to go on with
    ``retry_seed(seed, attempt)``, attempt = 1, 2, ... up to `retries` times per candidate; the last attempt is kept however it ends.
    A slot that ends on <eos> is never rewound.  ``drive_slots`` sees a rewound slot as still running, so its policy, the arrival
    order and ``drive_samples``' choice between start and start_from are unchanged; retries = 0 rewinds nothing.  Returns what
    ``drive_samples`` returns."""
    cand: Dict[int, int] = {}               # slot -> the candidate it holds
    tries: Dict[int, int] = {}              # slot -> rewinds of that candidate so far

    class _Retrying:
        def step(self, n):
            status = dict(session.step(n))
            for slot in sorted(cand):
                if status.get(slot) != "done" or tries[slot] >= retries:
                    continue
                g = session.n_gen(slot)
                if g < max_length:          # ended on <eos>
                    continue
                tries[slot] += 1
                rewind(slot, cand[slot], g // 2, tries[slot])
                status[slot] = "running"
            return status

        def take(self, slot):
            cand.pop(slot, None)
            tries.pop(slot, None)
            return session.take(slot)

    def begin(slot, c):
        cand[slot], tries[slot] = c, 0

    def start_(slot, c):
        start(slot, c)
        begin(slot, c)

    def start_from_(slot, src, c):
        start_from(slot, src, c)
        begin(slot, c)

    return drive_samples(_Retrying(), slots, n_requests, samples, start_, start_from_, step_n)


def pick_best(scores: Sequence[tuple]) -> int:
    """The ranking rule of ``generate_many(keep="best")``, a plain function of the candidates' (sum, count, ended_on_eos) as
    ``DecodeSlots.score`` gives them: the index of the candidate kept.  A candidate that ended on <eos> ranks above every candidate
    that ran to max_length (a run-away is what `retries` exists to get rid of); within a class the higher mean log-probability per
    step, sum / count, wins; ties go to the lower index.  count == 0 cannot occur for an ended slot and is refused."""
    if len(scores) < 1:
        raise ValueError("pick_best: no candidates")
    best, best_key = -1, None
    for i, (total, count, eos) in enumerate(scores):
        if int(count) < 1:
            raise ValueError(f"pick_best: candidate {i} has count {count}: an ended slot has at least one scored step")
        key = (1 if eos else 0, float(total) / int(count))
        if best_key is None or key > best_key:
            best, best_key = i, key
    return best


def keep_best(flat: Sequence[tuple], samples: int) -> list:
    """``pick_best`` over each request's `samples` consecutive candidates of `flat` (takes or collected entries in candidate order, the
    score last): [(k, take of candidate k)], one per request."""
    rows = (flat[i: i + samples] for i in range(0, len(flat), samples))
    return [(k, row[k]) for row in rows for k in [pick_best([t[-1] for t in row])]]


def drive_best(session, slots: int, n_requests: int, samples: int, retries: int, max_length: int, start, start_from, rewind,
               step_n: int = 1) -> list:
    """``drive_retries`` (retries = 0: ``drive_samples``) on a session opened with score=True, every candidate taken with its score
    (``session.take(slot, return_score=True)``: the last element of the take), then ``pick_best`` per request.  The drivers, their
    arrival order and which candidates start from a sibling are unchanged; a rewound candidate is ranked by its last attempt, whose
    score is that of its whole final path.  Returns [(k, take of candidate k)], one per request."""

    class _Scored:
        def step(self, n):
            return session.step(n)

        def n_gen(self, slot):
            return session.n_gen(slot)

        def take(self, slot):
            return session.take(slot, return_score=True)

    rows = drive_retries(_Scored(), slots, n_requests, samples, retries, max_length, start, start_from, rewind, step_n)
    return keep_best([t for row in rows for t in row], samples)


class CandidateRun:
    """What ``Text2Audio.generate_many`` runs its candidates on, no device and no Text2Audio in it: the main session, the holding session
    of prefill = P rows with its bookkeeping, and how candidate c = request * samples + k is started, rewound and submitted, each stated
    once, so that every option meets the same calls.  ``encode(i)`` gives request i's (text_outs [L, D], L) as a one-utterance call
    does; `continual` the prompt tokens per request, or None.  ``open``, then ``drive``; ``close`` frees whatever was opened."""

    def __init__(self, n_requests: int, samples: int, seeds: Sequence[int], rules: Optional[SamplingRules], encode, continual=None):
        self.n, self.N, self.seeds, self.rules, self.encode = int(n_requests), int(samples), seeds, rules, encode
        self.continual = continual if continual is not None else [None] * self.n
        self.max_length, self.sampling = None, None          # of every candidate: ``drive`` sets them
        self.texts: Dict[int, tuple] = {}                     # request -> (text_outs, len)
        self.session = self.held = self.plan = None

    def open(self, model, slots: int, prefill: int = 0, queue: bool = False, score: bool = False, elastic: bool = False) -> None:
        """The main session of `slots` slots (wide above 16) and, with prefill = P > 0, the holding session of P rows.  A queued
        session is opened on the holding session, which therefore comes first, with room for every ticket in flight."""
        self.slots, self.rows, self.queued, self.scored, self.elastic = slots, int(prefill), bool(queue), bool(score), bool(elastic)
        more = {key: True for key, on in (("score", score), ("wide", int(slots) > 16), ("elastic", elastic)) if on}
        hold = lambda: model.open_decode(self.rows, logp=False)
        if queue:
            self.held = hold()
            more.update(queue=int(slots) + self.rows * self.N, source=self.held)
        self.session = model.open_decode(slots, logp=False, **more)
        if self.rows and not queue:
            self.held, self.plan = hold(), HeldPrompts(self.rows, self.n, self.N)

    def close(self) -> Optional[dict]:
        """Frees the sessions that were opened.  Returns the run's {"prefix_passes": {"main", "held"}, "elastic": {"moves", "blocks"}
        or None}; None if the main session never opened."""
        session, held, self.session, self.held = self.session, self.held, None, None
        counts = None if session is None else dict(
            prefix_passes={"main": session.prefix_passes, "held": held.prefix_passes if held is not None else 0},
            elastic={"moves": session.moves, "blocks": dict(session.blocks_hist)} if self.elastic else None)
        for opened in (session, held):
            if opened is not None:
                opened.free()
        return counts

    def encoded(self, i: int) -> tuple:
        """Request i's (text_outs, len): encoded when first needed, alone, so its text_outs are those of a one-utterance call."""
        if i not in self.texts:
            self.texts[i] = self.encode(i)
        return self.texts[i]

    def fill(self, batch) -> None:
        """[(row, request)] into the holding session in one prefix pass; held rows start greedy with max_length 1, what they sample
        is never used."""
        requests = {}
        for row, q in batch:
            text_outs, text_len = self.encoded(q)
            requests[row] = dict(text_outs=text_outs, text_len=text_len, max_length=1, sampling=False, continual=self.continual[q])
        self.held.start_many(requests)

    def start(self, slot: int, c: int, src: Optional[int] = None) -> None:
        """Candidate c into `slot`, by one of three ways that give the same bits: with prefill EVERY candidate, first or sibling, is a
        copy from its request's row of the holding session (filled first if the request is not held); else a copy of the sibling
        running in slot `src`; else its own prefix pass."""
        i, args = c // self.N, (self.max_length, self.sampling, self.seeds[c])
        if self.plan is not None:
            todo = self.plan.need(i)
            if todo:
                self.fill(todo)
            self.session.start_from(slot, self.plan.start(i), *args, rules=self.rules, source=self.held)
        elif src is not None:
            self.session.start_from(slot, src, *args, rules=self.rules)
        else:
            self.session.start(slot, *self.encoded(i), *args, self.continual[i], rules=self.rules)

    def start_from(self, slot: int, src: int, c: int) -> None:
        self.start(slot, c, src)

    def rewind(self, slot: int, c: int, keep: int, attempt: int) -> None:
        self.session.rewind(slot, keep, self.max_length, self.sampling, retry_seed(self.seeds[c], attempt), rules=self.rules)

    def submit(self, row: int, c: int) -> int:
        return self.session.submit(row, self.max_length, self.sampling, self.seeds[c], rules=self.rules)

    def drive(self, max_length: int, sampling, retries: int = 0, step_n: int = 1) -> tuple:
        """Every candidate through the driver the options name.  Returns (taken, choice): taken is flat, what ``take`` / ``collect`` gave
        per candidate in candidate order, and choice None; on a session with scores taken holds each request's winner only and
        choice[i] = (k, its mean log-probability per step) names it."""
        self.max_length, self.sampling = max_length, sampling
        slot_drivers = (self.slots, self.n, self.N, retries, max_length, self.start, self.start_from, self.rewind, step_n)
        if self.queued:
            flat = drive_queue(self.session, self.rows, self.n, self.N, self.fill, self.submit, step_n)
        elif not self.scored:                # retries = 0 rewinds nothing: drive_samples
            flat = [t for row in drive_retries(self.session, *slot_drivers) for t in row]
        if not self.scored:
            return flat, None
        kept = keep_best(flat, self.N) if self.queued else drive_best(self.session, *slot_drivers)
        return [t for _, t in kept], [(k, t[-1][0] / t[-1][1]) for k, t in kept]


class LauraGenMI355X:
    """Drop-in for the inference surface of ``LauraGenModel``: same method names, argument meaning and return values
    (batch-1 tensors in, tensors out) as funcodec/models/audio_generation/laura_model.py, plus ``*_batch`` forms."""

    def __init__(self, spec: LauraSpec, device="cuda:0", max_positions: int = 2048):
        self.spec = spec
        self.engine = LauraEngine(spec, device, max_positions)
        self.device = self.engine.device
        self.vocab_size = spec.vocab_size
        self.token_list = spec.token_list
        self.predict_nq = spec.predict_nq
        self.codebook_size = spec.codebook_size
        self.codebook_dim = spec.codebook_dim
        self.sos_eos, self.task_id = 0, 1
        self.training = False
        self._seed_counter = 0

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def load_state_dict(self, state, strict: bool = False):
        self.engine.load_state_dict(state)

    # Text2Audio.tokenize_text reads model.token_embedding(token_idx) (bin/text2audio_inference.py:112); the lookup happens inside
    # fc_laura_encode, so the "embedding" of the drop-in is the id tensor itself
    def token_embedding(self, token_idx: torch.Tensor) -> torch.Tensor:
        return torch.as_tensor(token_idx).long()

    @torch.no_grad()
    def encode(self, text: torch.Tensor, text_lengths: torch.Tensor):
        lens = [int(v) for v in torch.as_tensor(text_lengths).reshape(-1)]
        return self.engine.encode(text, lens), torch.as_tensor(lens, dtype=torch.int64, device=self.device)

    def _next_seed(self) -> int:
        # the reference draws from torch's global generator; a generation here is a function of (torch seed, call index)
        self._seed_counter += 1
        return _u64(int(torch.initial_seed()) * 1000003 + self._seed_counter)

    @torch.no_grad()
    def decode_codec(self, text: torch.Tensor, text_lengths: torch.Tensor, max_length: int = 30 * 25,
                     sampling: Union[bool, int, float] = True, beam_size: int = 1, continual: List = None, seed: Optional[int] = None) -> torch.Tensor:
        """One utterance, like the reference: text [1, L, D] -> tokens [1, T, predict_nq]."""
        cont = None
        cl = None
        if continual is not None and len(continual) > 0:
            cont = torch.as_tensor(continual, dtype=torch.int64).reshape(1, -1, self.predict_nq)
            cl = [cont.shape[1]]
        tokens, lens = self.engine.decode_codec(text, [int(torch.as_tensor(text_lengths).reshape(-1)[0])], max_length, sampling,
                                                self._next_seed() if seed is None else seed, cont, cl)
        return tokens[:, : lens[0]]

    @torch.no_grad()
    def decode_codec_batch(self, text: torch.Tensor, text_lengths: Sequence[int], max_length: int = 30 * 25,
                           sampling: Union[bool, int, float] = True, continual: Optional[torch.Tensor] = None,
                           continual_lengths: Optional[Sequence[int]] = None, seed: Optional[int] = None):
        return self.engine.decode_codec(text, text_lengths, max_length, sampling, self._next_seed() if seed is None else seed, continual,
                                        continual_lengths)

    def open_decode(self, slots: int, max_positions: Optional[int] = None, logp: bool = True, score: bool = False,
                    wide: bool = False, queue: Optional[int] = None, source: Optional[DecodeSlots] = None,
                    elastic: bool = False) -> DecodeSlots:
        if elastic:
            return self.engine.open_decode(slots, max_positions, logp, score, wide, queue, source, elastic=True)
        if queue is None and source is None:
            return self.engine.open_decode(slots, max_positions, logp, score, wide)
        return self.engine.open_decode(slots, max_positions, logp, score, wide, queue, source)

    @torch.no_grad()
    def cal_codec_emb_batch(self, text, text_lengths, codec, codec_lengths):
        return self.engine.codec_emb(text, text_lengths, codec, codec_lengths)

    @torch.no_grad()
    def syn_audio(self, codec: torch.Tensor, text: torch.Tensor, text_lengths: torch.Tensor, codec_model, continual_length=None):
        """laura_model.py:550-567: codec [1, T, nq] -> waveform through the codec model's decode_emb."""
        tl = [int(torch.as_tensor(text_lengths).reshape(-1)[0])]
        emb = self.engine.codec_emb(text, tl, codec, [codec.shape[1]])
        _, _, recon_wav, _ = codec_model(emb[:, continual_length:], run_mod="decode_emb")
        return recon_wav
