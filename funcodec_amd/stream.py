"""Streaming encode / decode for causal checkpoints (``norm: weight_norm, causal: true``) on top of the fc_stream_* calls
(``CodecStream``: one batch in lock-step) and the fc_slots_* calls (``StreamSlots``: slots that start, push and end independently).

The reference has no streaming implementation (``streaming=`` of ``funcodec/bin/codec_inference.py`` selects a data
iterator), so the specification is causality itself: pushing an utterance through in chunks gives what the offline call
(``Encodec.inference_encoding`` / ``inference_decoding``, codec_basic.py:720-836) gives for the whole utterance.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import numbers
import struct
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .config import SEQ_FF, SEQ_HEADS
from .engine import (CodecEngine, EngineError, _on_device, _ptr, floor_refusal, floor_value, packed_refusal, rate_min_nq, row_nq_list,
                     rvq_beam_width)


def stream_refusal(arch, max_frames: Optional[int] = None) -> Optional[str]:
    """Why a model of this architecture cannot stream (the configuration key is named), or None.  max_frames: the bound of an
    utterance's frames that a session of a causal transformer net is opened with (the size of its key / value cache); without it such
    a net is refused, and with it a net that has no transformer bottleneck is: nothing is silently ignored."""
    if arch.model_type != "encodec":
        return "streaming is not available for model: freq_codec (the STFT frames overlap; time-domain codec only)"
    if not arch.causal:
        return "streaming needs encoder_conf.causal / decoder_conf.causal: true (a non-causal net looks ahead at every layer)"
    if arch.lstm_layers > 0 and arch.seq_model == "transformer":
        if max_frames is None:
            return ("streaming is not available for seq_model: transformer (it needs a key / value cache across pushes: "
                    "open_stream(..., max_frames=N) gives it a size)")
    if arch.segment_length is not None:
        return "streaming is not available with model_conf.segment_dur (segments are normalised and decoded as whole utterances)"
    if arch.q0_ds_ratio > 1:
        return "streaming is not available for quantizer_conf.q0_ds_ratio > 1 (the half-rate first stage looks across frame pairs)"
    if max_frames is not None:
        if not (arch.lstm_layers > 0 and arch.seq_model == "transformer"):
            return "max_frames bounds the key / value cache of seq_model: transformer; this net has no transformer bottleneck, open it without max_frames"
        samples, frames = min_first(arch)
        hop = 1
        for r in arch.ratios:
            hop *= r
        need = max(samples // hop, frames)
        if int(max_frames) < need:
            return f"max_frames must hold the first push of an utterance: at least {need} frames for this net, got {max_frames}"
    return None


FC_SLOT_START, FC_SLOT_FINAL = 1, 2

#: fc_graphstream_set's own wording for a lock-step session with a key / value cache (raised here before anything is opened)
GRAPH_MAX_FRAMES_REFUSAL = ("graph replay is not available for a lock-step session opened with max_frames: its key / value cache position is a "
                            "launch argument that changes with every push; a slot session opened with max_frames reads every row's position "
                            "from device memory and replays")


class _GraphBuffers:
    """What a session opened with ``graph=True`` owns so that the pointers of its pushes, which are part of the key of a captured push,
    repeat from push to push: one flat device buffer per argument, sized once for ``max_chunk`` and viewed from its base in the shape
    of the push (the pointer does not move with the push's width), its own workspace, and its own stream (the default stream cannot
    be captured).  The caching allocator gives no such promise for tensors allocated per push."""

    def __init__(self, sess, rows: int):
        eng, arch, dev = sess.engine, sess.arch, sess.device
        ch, D, n_q = eng.channels, arch.dimension, sess.n_q
        tf_enc = eng.frames(sess.max_chunk)                 # a FINAL encode push rounds up at every stride
        tf_dec = -(-sess.max_chunk // sess.hop)
        f32, i64 = torch.float32, torch.int64
        sizes = {"wav_in": (rows * ch * sess.max_chunk, f32), "codes": (n_q * rows * tf_enc, i64), "quantized": (rows * tf_enc * D, f32),
                 "enc_out": (rows * tf_enc * D, f32), "tokens": (rows * tf_dec * n_q, i64), "emb": (rows * tf_dec * D, f32),
                 "wav_out": (rows * ch * tf_dec * sess.hop, f32), "scale": (rows, f32)}
        if sess.per_frame:      # the decode pushes' stage counts per frame: part of a captured push's key, like every pointer
            sizes["frame_nq"] = (rows * tf_dec, torch.int32)
        self._flat = {k: torch.zeros(n, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
        self.ws = torch.empty(sess._ws_bytes, dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.Stream(device=dev)
        self.device = dev

    def view(self, name: str, shape) -> torch.Tensor:
        n = 1
        for v in shape:
            n *= int(v)
        return self._flat[name][:n].view(*shape)

    @contextlib.contextmanager
    def on_stream(self):
        """the push itself runs on the session's stream, ordered behind and in front of the caller's current stream"""
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        try:
            with torch.cuda.stream(self.stream):
                yield
        finally:
            cur.wait_stream(self.stream)


class _Side:
    """what a wrapper keeps per utterance and side (encode / decode)"""
    __slots__ = ("head", "started", "ended", "frames")

    def __init__(self):
        self.head, self.started, self.ended, self.frames = [], False, False, 0      # frames: pushed so far (read where max_frames bounds them)

    @property
    def running(self) -> bool:
        """the library holds state for this side: its first push is taken and its final one is not"""
        return self.started and not self.ended

    def copy(self, head=None, device=None) -> "_Side":
        """a copy that shares nothing that changes (the held pieces are never written in place); head: other pieces in place of its own"""
        sd = _Side()
        pieces = self.head if head is None else head
        sd.head = [t if device is None else t.to(device) for t in pieces]
        sd.started, sd.ended, sd.frames = self.started, self.ended, self.frames
        return sd


class _Session:
    """What CodecStream and StreamSlots share: the library's session over `rows` rows (the fc_stream_* or the fc_slots_* calls, `_family`),
    its state and sizes, and the start-up and splitting rule of an utterance."""
    _family = ""
    _cached_family = ""       # the pair that sizes and creates the kind's session with a key / value cache (max_frames)
    _graph_family = ""        # the three calls of the kind's graph replay (set, enabled, counts)

    def __init__(self, model, rows: int, n_q: Optional[int], max_chunk: Optional[int], max_frames: Optional[int] = None, graph: bool = False,
                 rvq_beam: Optional[int] = None, min_n_q: int = 1, per_frame: bool = False):
        why = stream_refusal(model.arch, max_frames)
        if why:
            raise EngineError(why)
        #: a property of the session: a noise floor chooses a stage count per FRAME of a push (the push frame rule of
        #: csrc/rvq_rate_kernels.h), packets are of mode 1, and every decode push from codes runs under a count per frame
        self.per_frame = bool(per_frame)
        if self.per_frame and floor_refusal(model.arch):
            raise EngineError("per_frame=True: " + floor_refusal(model.arch))
        #: the noise floor of every row's encode pushes in dB (None: the row has none and runs its fixed count); set on the engine around
        #: each encode push while any row has one (the push rule of csrc/rvq_rate_kernels.h), min_n_q with it
        self._floor_db: List[Optional[float]] = [None] * int(rows)
        self._fused = True            # False: the four-launch chain in place of the fused launch (a measurement aid: same bits)
        #: width of the quantiser's search over the stages in this session's encode pushes (1: greedy); set on the engine around each of them
        self.rvq_beam = rvq_beam_width(model.arch, rvq_beam)
        if graph and max_frames is not None and self._family == "fc_stream":
            raise EngineError(GRAPH_MAX_FRAMES_REFUSAL)
        self.model, self.engine, self.arch = model, model.engine, model.arch
        eng = self.engine
        self.lib, self.device = eng.lib, eng.device
        #: the session's n_q: the first dimension of its codes, and the most any row may use (the cap of the per-row stage counts)
        self.n_q = int(n_q) if n_q is not None else self.arch.num_quantizers
        #: the rows' own stage counts; None while every row runs all n_q stages (nothing is set on the engine then)
        self._row_nq: Optional[List[int]] = None
        self.hop = eng.hop_length
        self._h = None
        #: the most frames an utterance may hold per side (a causal transformer net: the size of its key / value cache), or None
        self.max_frames = int(max_frames) if max_frames is not None else None
        #: True while the library replays this session's steady pushes as captured HIP graphs (False with FC_SESSION_GRAPH=0)
        self.graph = False
        self._g: Optional[_GraphBuffers] = None         # the fixed buffers of a session opened with graph=True; None: nothing of it exists
        self.min_n_q = rate_min_nq(self.arch, min_n_q, self.n_q, floor=0 if self.per_frame else 1)
        self._open(rows, max_chunk)
        #: the stage counts the last encode push under a noise floor chose, device int32 [rows]: one of the session's fixed buffers
        self._nq_table = torch.zeros(int(rows), dtype=torch.int32, device=self.device)
        #: per_frame: the counts per frame of the last such push, viewed dense [rows][its frames] from the base of a fixed device buffer
        #: sized for max_chunk, and the fixed workspace of the mode-1 pack launch's scan
        self._nqf_flat: Optional[torch.Tensor] = None
        self._nqf: Optional[torch.Tensor] = None
        self._pack_ws: Optional[torch.Tensor] = None
        if self.per_frame:
            tf_enc = self.engine.frames(self.max_chunk)
            self._nqf_flat = torch.zeros(int(rows) * tf_enc, dtype=torch.int32, device=self.device)
            self._pack_ws = torch.empty(int(self.lib.fc_frame_pack_workspace_bytes(int(rows), tf_enc)), dtype=torch.uint8, device=self.device)
        if graph:
            self._graph_open(rows)

    def _fn(self, name: str):
        return getattr(self.lib, f"{self._family}_{name}")

    def _graph_fn(self, name: str):
        return getattr(self.lib, f"{self._graph_family}_{name}")

    @_on_device
    def _open(self, rows, max_chunk):
        eng = self.engine
        cached = self.max_frames is not None            # a session with a key / value cache: sized and created by the fc_seq*_ pair of its kind
        seq = lambda name: getattr(self.lib, f"{self._cached_family}_{name}")
        nbytes = int(seq("state_bytes")(eng._h, rows, self.max_frames) if cached else self._fn("state_bytes")(eng._h, rows))
        if nbytes == 0:
            raise EngineError("this engine cannot stream")
        #: everything the session carries between pushes (fc_stream_state_bytes): one allocation, nothing else is kept on the device
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        if self.state.is_cuda:
            torch.cuda.current_stream(self.device).synchronize()      # fc_slots_create writes the scales (1) with a copy that is not ordered with this stream
        self.max_chunk = int(max_chunk) if max_chunk is not None else 100 * self.hop
        h = C.c_void_p()
        if cached:
            eng._check(seq("create")(eng._h, rows, self.max_chunk, self.n_q, self.max_frames, _ptr(self.state), nbytes, C.byref(h)))
        else:
            eng._check(self._fn("create")(eng._h, rows, self.max_chunk, self.n_q, _ptr(self.state), nbytes, C.byref(h)))
        self._h = h
        self.min_first_samples = int(self._fn("min_first")(h, 0))
        self.min_first_frames = int(self._fn("min_first")(h, 1))
        self._ws_bytes = int(self._fn("workspace_bytes")(h))

    @_on_device
    def _graph_open(self, rows):
        self.engine._check(self._graph_fn("set")(self._h, 1))
        self.graph = bool(self._graph_fn("enabled")(self._h))
        self._g = _GraphBuffers(self, rows)

    def graph_stats(self) -> Dict[str, int]:
        """{replays, captures, evictions, fallbacks} of this session's pushes since it was opened (all 0 without ``graph=True``):
        pushes replayed from a cached graph, pushes captured (a new key), cached graphs evicted (16 are kept), and pushes that ran
        eagerly because their capture could not be made."""
        out = (C.c_int64 * 4)()
        self._graph_fn("counts")(self._h, out)
        return dict(zip(("replays", "captures", "evictions", "fallbacks"), (int(v) for v in out)))

    # A push's tensors.  Without graph=True: allocated per push and returned as they are.  With it: views of the session's fixed
    # buffers, the push on the session's own stream and workspace, and what is returned are copies (the next push overwrites the buffers).
    def _buf(self, name: str, shape, dtype) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype, device=self.device) if self._g is None else self._g.view(name, shape)

    def _given(self, name: str, x: torch.Tensor) -> torch.Tensor:
        if self._g is None:
            return x
        buf = self._g.view(name, x.shape)
        buf.copy_(x)
        return buf

    def _out(self, t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        return t if self._g is None or t is None else t.clone()

    def _push_ws(self) -> torch.Tensor:
        return self._ws() if self._g is None else self._g.ws

    def _push_stream(self):
        return contextlib.nullcontext() if self._g is None else self._g.on_stream()

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    def _scratch(self, nbytes: int) -> torch.Tensor:
        # the engine's own scratch buffer, by the engine's own rule; called on the class because all it needs of the engine is `_ws` and `device`
        return CodecEngine._scratch(self.engine, nbytes)

    def _ws(self) -> torch.Tensor:
        return self._scratch(self._ws_bytes)

    def _take(self, sd: _Side, x: torch.Tensor, final: bool, tdim: int, unit: int, min_first: int, short):
        """The start-up and splitting rule of one side `sd` of one utterance.  What arrives along `tdim` (samples: unit = hop; frames:
        unit = 1) is held back until min_first of it is there; an utterance that ends (final) before that raises short(have).  Then
        everything held comes out at once, cut into pieces no longer than a call takes, all but the last whole hops:
        [(part, flags)] with START on the utterance's first piece and FINAL on its last.  Returns (pieces, what stays held back) and
        changes nothing."""
        head, flags = sd.head + [x], 0
        if not sd.started:
            have = sum(t.shape[tdim] for t in head)
            if have < min_first:
                if final:
                    raise short(have)
                return [], head
            flags = FC_SLOT_START
        x = torch.cat(head, tdim) if len(head) > 1 else head[0]
        n, cap = x.shape[tdim], self.max_chunk // (self.hop // unit)      # samples (unit = hop) or frames (unit = 1) per call
        step = cap // unit * unit
        out, pos = [], 0
        while pos < n:
            m = n - pos if n - pos <= cap else step
            out.append((x.narrow(tdim, pos, m), flags | (FC_SLOT_FINAL if final and pos + m == n else 0)))
            flags, pos = 0, pos + m
        return out, []

    def _checked_row_nq(self, rows, n: int) -> List[int]:
        """n stage counts in [1, the session's n_q], or an EngineError before anything is changed"""
        if not 1 <= self.n_q <= self.arch.num_quantizers:
            raise EngineError(f"n_q lies in [1, {self.arch.num_quantizers}], got {self.n_q}")
        return row_nq_list(self.arch, rows, n, self.n_q)

    def _engine_row_nq(self, rows):
        """the engine's table around one push; with no counts of its own a push does not touch the engine's table at all"""
        return contextlib.nullcontext() if rows is None else self.engine._row_nq(rows)

    def _engine_push_frame_nq(self, table):
        """the engine's stage count per frame around one decode push of a per_frame session; any other push does not touch the engine's at all"""
        return contextlib.nullcontext() if table is None else self.engine._push_frame_nq(table)

    def _engine_rvq_beam(self):
        """the width of the quantiser's search around one encode push; a session of width 1 does not touch the engine's at all"""
        return contextlib.nullcontext() if self.rvq_beam == 1 else self.engine._rvq_beam(self.rvq_beam)

    def _checked_floor(self, db) -> Optional[float]:
        """one row's noise_floor_db (None: no floor), or an EngineError before anything is changed"""
        if db is None:
            return None
        why = floor_refusal(self.arch)
        if why:
            raise EngineError(why)
        floor_value(self.arch, db)
        return float(db)

    def _push_floor(self):
        """what an encode push sets on the engine: every row's floor D * 10^(dB / 10) (None: the row is switched off), or None when no
        row has a floor (the push then does not touch the engine's floor at all)"""
        if all(v is None for v in self._floor_db):
            return None
        return [None if v is None else floor_value(self.arch, v) for v in self._floor_db]

    def _engine_floor(self, Tf: int = 0):
        """the engine's noise floor around one encode push of Tf frames; min_n_q is checked against the rows' caps before anything is set.
        per_frame: the push writes its counts per frame into the session's table, viewed [rows][Tf] (``_nqf``; None after a push without a floor)"""
        floors = self._push_floor()
        self._nqf = None
        if floors is None:
            return contextlib.nullcontext()
        rate_min_nq(self.arch, self.min_n_q, self.n_q, self._row_nq, floor=0 if self.per_frame else 1)
        if not self.per_frame:
            return self.engine._floor(floors, self.min_n_q, self._nq_table, self._fused)
        rows = len(floors)
        self._nqf = self._nqf_flat[:rows * int(Tf)].view(rows, int(Tf))
        return self.engine._floor(floors, self.min_n_q, self._nq_table, self._fused, n_q_frames_out=self._nqf)

    def _one_push(self, pieces, what: str) -> None:
        """a packet carries ONE count, a push under a noise floor chooses one per push: such a call is one push"""
        if len(pieces) > 1:
            raise EngineError(f"{what}: encode(packed=True) under a noise floor takes what fits one push (max_chunk = {self.max_chunk} samples): "
                              f"this call splits into {len(pieces)} pushes, each with a count of its own; nothing was changed")

    def _push_row_nq(self):
        """what a push sets on the engine: the rows' counts, or None when every row runs all n_q stages (the plain kernels)"""
        rows = self._row_nq
        return None if rows is None or all(v == self.n_q for v in rows) else rows

    def _fits(self, sd: _Side, frames: int, what: str) -> None:
        """the bound of a session with a key / value cache: a call whose frames would pass max_frames is refused before anything is pushed"""
        if self.max_frames is not None and sd.frames + frames > self.max_frames:
            raise EngineError(f"streaming {what}: this call's {frames} frames would take the utterance to {sd.frames + frames} frames, past the "
                              f"session's max_frames = {self.max_frames} (the size of its key / value cache); nothing was changed, reset() "
                              "starts the next utterance")

    # -- packets of a push (csrc/code_pack_kernels.h states the packet).  The pack / unpack launch is one more call on the session's
    # stream, behind / in front of the push and outside any captured graph; a push that asks for no packets launches what it did.
    def _packed_check(self) -> None:
        why = packed_refusal(self.arch)
        if why:
            raise EngineError(why)

    def _pack_rows(self, codes: torch.Tensor, frames, counts, counts_frames: Optional[torch.Tensor] = None) -> List[bytes]:
        """codes [n_q,R,Tf] of R rows with their own frames and stage counts -> R packets on the host (one launch, one copy).
        counts_frames (device int32 [R,Tf]; a per_frame session under a floor): packets of mode 1, a count per frame, instead."""
        with self._push_stream():
            if counts_frames is not None:
                packets = self.engine.pack_codes(codes, frames_rows=frames, n_q_frames=counts_frames, ws=self._pack_ws)
            else:
                packets = self.engine.pack_codes(codes, frames_rows=frames, n_q_rows=counts)
        return self.engine.packets_to_host(packets)

    def _unpack_rows_frames(self, packets, what: str):
        """a per_frame session: host packets of either mode, mixed -> (tokens [R,Tf,n_q], n_q_frames [R,Tf] i32, both on the device, frames):
        every header (a mode-1 packet's counts section too) validated on the host against the session's n_q, row and field named"""
        from .io import frame_packet_pitch
        packets = [bytes(p) for p in packets]
        try:
            _, frames, counts, _ = self.engine._parse_packets_any(packets, exact=True)
        except EngineError as err:
            raise EngineError(f"{what}: {err}") from None
        for b, k in enumerate(counts):
            if k > self.n_q:
                raise EngineError(f"{what}: row {b}: packet field k: {k} stages, more than the {self.n_q} of this session")
        if min(frames) < 1:
            raise EngineError(f"{what}: a packet without frames decodes to nothing; leave it out")
        import numpy as np
        Tf = max(frames)
        host = np.zeros((len(packets), frame_packet_pitch(Tf, self.n_q, self.engine.code_bits)), dtype=np.uint8)
        for b, p in enumerate(packets):
            host[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        with self._push_stream():
            tokens, kf = self.engine.unpack_frame_codes(torch.from_numpy(host).to(self.device), Tf, self.n_q)
        return tokens, kf, frames

    def _with_counts(self, codes: torch.Tensor, n_q_frames, count: int, what: str) -> torch.Tensor:
        """a per_frame session: codes [..., Tf, n_q] with the frames' stage counts as one more column, so that the start-up and splitting
        rule cuts both alike.  n_q_frames [..., Tf] (any integer tensor), else `count` in every frame."""
        shape = tuple(codes.shape[:-1])
        if n_q_frames is None:
            kf = torch.full(shape, int(count), dtype=torch.int64, device=self.device)
        else:
            kf = self.engine._dev(torch.as_tensor(n_q_frames), torch.int64)
            if tuple(kf.shape) != shape:
                raise EngineError(f"{what}: n_q_frames must be {list(shape)} (a count per frame of the codes), got {list(kf.shape)}")
        return torch.cat([codes, kf.unsqueeze(-1)], -1)

    def _unpack_rows(self, packets, what: str):
        """host packets -> (tokens [R,Tf,n_q] on the device, frames, counts), every header validated against the session's n_q"""
        packets = [bytes(p) for p in packets]
        for b, p in enumerate(packets):
            if len(p) > 6 and p[6] == 1:
                raise EngineError(f"{what}: row {b}: packet field mode: a stage count per frame (mode 1) is for offline calls only; "
                                  "sessions decode packets of mode 0")
        buf, Tf, counts = self.engine.packets_from_host(packets, n_q=self.n_q)
        frames = self.engine._parse_packets(packets, exact=True)[0]
        if min(frames) < 1:
            raise EngineError(f"{what}: a packet without frames decodes to nothing; leave it out")
        with self._push_stream():
            tokens = self.engine.unpack_codes(buf, Tf, self.n_q)
        return tokens, frames, counts

    # -- the slot record (csrc/slots_kernels.h states it): what both kinds of session share of export
    def _record_floats(self, enc: _Side, dec: _Side) -> int:
        """the length of the record of a slot whose sides are `enc` and `dec` (slot_record_floats, its segment list walked once per session)"""
        shape = getattr(self, "_rec_shape", None)
        if shape is None:
            segs = slot_record_segments(self.arch, self.max_frames is not None)
            cols = lambda side: sum(n for kind, sd, n in segs if kind in "KV" and sd == side)
            shape = self._rec_shape = (sum(n for kind, _, n in segs if kind not in "KV"), cols("encoder"), cols("decoder"))
        pitch = lambda sd: (sd.frames + 15) // 16 * 16 if sd.running else 0
        return shape[0] + shape[1] * pitch(enc) + shape[2] * pitch(dec)

    def _export_rows(self, call, rows: List[int], sides) -> Tuple[torch.Tensor, list]:
        """the records of `rows` (each with a side Running) by ONE launch: (device floats [n, pitch], [meta tuple]); sides: per row its
        (_Side, _Side), which size the buffer by the frames in use, never by max_frames"""
        n = len(rows)
        pitch = -(-max(self._record_floats(e, d) for e, d in sides) // 4) * 4        # rows of the buffer begin 16-byte aligned
        buf = torch.empty((n, pitch), dtype=torch.float32, device=self.device)
        metas = (_lib.FcSlotMeta * n)()
        with self._push_stream():
            self.engine._check(call(self._h, n, (C.c_int32 * n)(*rows), _ptr(buf), pitch, metas, self.engine._stream()))
        return buf, [tuple(int(getattr(m, f)) for f, _ in _lib.FcSlotMeta._fields_) for m in metas]

    def _lstm_scratch(self, x: torch.Tensor) -> torch.Tensor:
        B, H, T = x.shape
        return self._scratch(4 * (T * B * 4 * H + 2 * B * H * T) + (1 << 20))


class CodecStream(_Session):
    """One utterance batch pushed through a causal codec chunk by chunk; obtained from ``EncodecMI355X.open_stream``.

    * ``encode(wav, final=False) -> (codes [n_q,B,Tf], quantized [B,Tf,D])``: every push but the final one is a positive
      multiple of ``hop`` samples; the final one has any length >= 1.  A push that breaks the rule raises, it is never padded.
    * ``decode(codes [B,Tf,n_q])`` / ``decode_emb(emb [B,Tf,D]) -> wav [B,C,Tf*hop]``.
    * ``encode(wav, final, packed=True)`` also returns the push's packets, a list of B ``bytes`` (csrc/code_pack_kernels.h states the
      packet): this push's frames at every row's current stage count; ``decode_packed(packets, final=False)`` is the inverse and decodes
      every row with the count its packet carries.  Pack and unpack are one more launch beside the push, outside any captured graph.
    * ``reset(scale=None)`` starts the next utterance.
    * ``set_n_q(rows)``: a stage count per utterance, each in [1, n_q], for the pushes that follow -- in the middle of an utterance
      too (a residual quantiser is a prefix code and carries nothing from frame to frame).  ``open_stream(batch, n_q=[...])`` sets them
      from the start; the session's ``n_q``, the first dimension of its codes, is then the largest of the list.  Row b of a push is what
      a session with ``n_q = rows[b]`` gives it; its codes at later stages are 0, and ``decode`` does not read them.

    Start-up.  The offline call pads every causal conv on the left by *reflection* (``pad_mode: reflect``, conv.py:82-99,
    251-253), i.e. with the columns that follow: only there does a frame depend on later input.  The session therefore
    holds back the first ``min_first_samples`` (encode) / ``min_first_frames`` (decode) of an utterance: pushes shorter than
    that return empty tensors until enough has arrived, then everything held back comes out at once.  From then on a push
    of n frames returns n frames that depend on nothing later.  An utterance shorter than the start-up goes through the
    offline call: ``encode(..., final=True)`` raises for it, and so does ``decode(..., final=True)``; without ``final`` a decode
    session cannot know that the utterance has ended and keeps returning empty tensors while it gathers.  A push that fails
    half-way (an error from the library) invalidates the utterance: every later call raises until ``reset``.

    Volume scale.  ``audio_normalize`` derives its scale from the whole utterance (codec_basic.py:366-371), which no
    stream can know: the session takes one scale per utterance (``scale`` [B], default 1); encode divides by it and decode
    multiplies by it when ``use_scale`` is set, as the offline ``use_scale`` does.  Feeding the offline call's scale
    reproduces the offline result; a running volume estimate is not implemented.

    Transformer bottleneck.  A causal net with ``seq_model: transformer`` attends over every earlier frame, so its session keeps the keys
    and values of every block (fc_seqstream_create) and needs their size: ``max_frames``, the most frames one utterance may hold per side.
    A call whose frames would pass it raises before anything is pushed and changes nothing; ``reset`` starts the next utterance.  Without
    ``max_frames`` such a net is refused, with it any other net is.

    Noise floor (``noise_floor_db``, ``min_n_q``; ``set_noise_floor``).  With a floor every encode push chooses a stage count per row on
    the device, inside the push, from the row's frames of that push alone (the push rule of csrc/rvq_rate_kernels.h; ``engine.floor_pick``
    restates it): the smallest count in [min_n_q, the row's cap] whose residual lies at or below ``D * 10^(dB / 10)`` per frame, min_n_q
    for a row already below it, the best count where it is missed.  ``set_n_q`` remains the cap.  Row b of a push is what a session with
    ``set_n_q`` = that count gives it.  ``last_n_q_rows`` is the device table [batch] of the last push's counts (nothing is read back);
    ``encode(packed=True)`` hands it to the pack launch, so every packet carries its own count and ``decode_packed`` needs nothing else.
    Such a packed call must fit one push (``max_chunk``): a packet carries one count.  One more launch per push.

    Noise floor per frame (``per_frame=True``, a property of the session; False by default, and such a session is exactly what it was).
    Under a floor every FRAME of a push takes its own count (the push frame rule of csrc/rvq_rate_kernels.h; ``engine.floor_pick_frames``
    restates it): the smallest count in [min_n_q, the row's cap] whose residual of THAT frame lies at or below ``D * 10^(dB / 10)``,
    min_n_q (which may be 0: a silent frame costs its count bits and nothing else) for a frame already below it, the frame's best count
    where it is missed.  A frame's count depends on that frame alone, not on how the audio is cut into pushes.  ``last_n_q_frames`` is
    the device table [batch][frames of the last push].  ``encode(packed=True)`` gives packets of mode 1 (a count per frame) whenever a
    floor is set -- a row without one packs its cap in every frame -- and of mode 0 without a floor; ``decode_packed`` takes packets of
    either mode, mixed, and ``decode(codes, n_q_frames=)`` a table of its own.  Every decode push from codes of such a session runs under
    a count per frame (fc_engine_set_push_frame_nq); ``set_n_q`` still gives the count of the frames without one.  One launch per push at
    every width.

    Graph replay (``graph=True``, off by default).  The library captures a steady push (neither the first of an utterance nor the
    final one) as a HIP graph and replays it for every later push with the same key: call form, width, parity of the side's push
    count, n_q, use_scale and every pointer.  The session therefore owns fixed device buffers sized for ``max_chunk``, a workspace and a
    stream of its own, copies what it is given into them, and RETURNS COPIES of the results, because the next push overwrites the
    buffers.  The results are the eager session's bits.  ``graph_stats()`` counts replays, captures, evictions and fallbacks;
    ``FC_SESSION_GRAPH=0`` in the environment keeps such a session eager.  Not available together with ``max_frames`` (the cache position
    of a lock-step session is a launch argument): ``open_slots(..., max_frames=N, graph=True)`` is.
    """

    _family = "fc_stream"
    _cached_family = "fc_seqstream"
    _graph_family = "fc_graphstream"

    def __init__(self, model, batch: int, n_q: Optional[int] = None, scale: Optional[torch.Tensor] = None,
                 max_chunk: Optional[int] = None, max_frames: Optional[int] = None, graph: bool = False, rvq_beam: Optional[int] = None,
                 noise_floor_db=None, min_n_q: int = 1, per_frame: bool = False):
        self.batch = int(batch)
        rows = None
        if n_q is not None and not isinstance(n_q, numbers.Integral):       # a count per utterance: refused before anything is opened
            rows = row_nq_list(model.arch, n_q, self.batch)
            n_q = max(rows)
        super().__init__(model, self.batch, n_q, max_chunk, max_frames, graph, rvq_beam, min_n_q, per_frame)
        self._row_nq = rows
        self.set_noise_floor(noise_floor_db)
        self.reset(scale)

    def set_n_q(self, rows) -> None:
        """stage counts [batch], each in [1, n_q], of the pushes that follow; a refused call changes nothing"""
        self._row_nq = self._checked_row_nq(rows, self.batch)

    def set_noise_floor(self, rows) -> None:
        """noise_floor_db of the encode pushes that follow: one value for every utterance, one per utterance (an entry None: that row keeps
        its fixed count), or None (no floor: the pushes launch what they always did); between pushes, in the middle of an utterance too.
        A refused call changes nothing."""
        if rows is None or isinstance(rows, numbers.Real):
            rows = [rows] * self.batch
        elif hasattr(rows, "tolist"):
            rows = rows.tolist()
        rows = list(rows)
        if len(rows) != self.batch:
            raise EngineError(f"noise_floor_db must hold one entry per row ({self.batch}), got {len(rows)}")
        self._floor_db = [self._checked_floor(v) for v in rows]

    @property
    def last_n_q_rows(self) -> torch.Tensor:
        """device int32 [batch]: the stage counts the last encode push under a noise floor chose (the session's own table: the next such
        push overwrites it; nothing is read back)"""
        return self._nq_table

    @property
    def last_n_q_frames(self) -> Optional[torch.Tensor]:
        """a per_frame session: device int32 [batch][frames of the last push]: the stage count of every frame of the last encode push
        under a noise floor (a view of the session's own table: the next such push overwrites it; nothing is read back); None when
        that push had no floor"""
        return self._nqf

    @_on_device
    def reset(self, scale: Optional[torch.Tensor] = None) -> None:
        sc = None
        if scale is not None:
            sc = self.engine._dev(torch.as_tensor(scale).reshape(-1), torch.float32)
            if sc.numel() != self.batch:
                raise EngineError(f"scale must hold one value per utterance ({self.batch}), got {sc.numel()}")
        self.engine._check(self.lib.fc_stream_reset(self._h, _ptr(sc), self.engine._stream()))
        self._enc, self._dec = _Side(), _Side()       # pushes held back until the start-up length has arrived
        self._scale_rows = sc                         # the utterances' scales as given (None: 1), for export

    @_on_device
    def export(self, row: int) -> "SlotRecord":
        """Utterance `row` of this lock-step session as a ``SlotRecord``, which a slot session of a model with the same architecture
        imports (``StreamSlots.import_slot``) and continues bit for bit; this session is only read and goes on as before."""
        if not isinstance(row, int) or not 0 <= row < self.batch:
            raise EngineError(f"this session streams utterances 0 .. {self.batch - 1}, got {row!r}")
        enc = self._enc.copy([x[row] for x in self._enc.head])
        dec = self._dec.copy([x[row] for x in self._dec.head])
        floats = meta = None
        if enc.running or dec.running:
            buf, metas = self._export_rows(self.lib.fc_slotrec_export_stream, [row], [(enc, dec)])
            meta = metas[0]
            floats = buf[0, :self._record_floats(enc, dec)].clone()
        scale = 1.0 if self._scale_rows is None else float(self._scale_rows[row])
        return SlotRecord(floats, meta, enc, dec, self.n_q if self._row_nq is None else self._row_nq[row], self._floor_db[row], scale)

    # -- encode --------------------------------------------------------------------------------
    def _encode_call(self, wav: torch.Tensor, final: bool, want_enc_out: bool = False):
        B, T = wav.shape[0], wav.shape[-1]
        Tf, D = self.engine.frames(T), self.arch.dimension
        wav = self._given("wav_in", wav)
        codes = self._buf("codes", (self.n_q, B, Tf), torch.int64)
        quant = self._buf("quantized", (B, Tf, D), torch.float32)
        enc = self._buf("enc_out", (B, Tf, D), torch.float32) if (self.arch.bypass_quantizer or want_enc_out) else None
        n = C.c_int(0)
        ws = self._push_ws()
        with self._push_stream(), self._engine_row_nq(self._push_row_nq()), self._engine_rvq_beam(), self._engine_floor(Tf):
            self.engine._check(self.lib.fc_stream_encode(self._h, _ptr(wav), T, int(final), _ptr(codes), _ptr(quant), _ptr(enc), C.byref(n),
                                                         _ptr(ws), ws.numel(), self.engine._stream()))
        assert n.value == Tf
        codes, quant, enc = self._out(codes), self._out(quant), self._out(enc)
        if self.arch.bypass_quantizer:         # codec_basic.py:700-701: the encoder output in place of the quantised embeddings
            return torch.zeros((B, Tf), dtype=torch.long, device=self.device), enc, enc
        return codes, quant, enc

    @_on_device
    def encode(self, wav: torch.Tensor, final: bool = False, want_enc_out: bool = False, packed: bool = False) -> Tuple[torch.Tensor, ...]:
        """wav [B,T] or [B,C,T] -> (codes [n_q,B,Tf], quantized [B,Tf,D]), plus the encoder output [B,Tf,D] when want_enc_out, plus, with
        packed=True, the packets of the push last: a list of B ``bytes`` holding this push's frames at every row's current stage count
        (self-contained: ``decode_packed`` takes them); an empty list while the start-up is held back."""
        if packed:
            self._packed_check()
        floor = self._push_floor() is not None
        res = self._encode(wav, final, want_enc_out, one_push=packed and floor)
        if not packed:
            return res
        codes = res[0]
        if codes.shape[-1] == 0:
            return res + ([],)
        if floor and self.per_frame:        # mode 1: the DEVICE counts per frame of the push
            return res + (self._pack_rows(codes, None, None, self._nqf),)
        counts = self._nq_table if floor else self._row_nq       # under a floor: the DEVICE counts of the push, every packet carries its k_b
        return res + (self._pack_rows(codes, None, counts),)

    def _encode(self, wav: torch.Tensor, final: bool, want_enc_out: bool, one_push: bool = False) -> Tuple[torch.Tensor, ...]:
        wav = self.engine._wav_in(wav)
        if wav.dim() == 2:
            wav = wav.unsqueeze(1)
        if wav.shape[0] != self.batch:
            raise EngineError(f"this session streams {self.batch} utterances, got {wav.shape[0]}")
        T = wav.shape[-1]
        if T < 1 or (not final and T % self.hop != 0):
            raise EngineError(f"streaming encode: every push but the final one must be a positive multiple of the hop ({self.hop} samples), "
                              f"got {T}; it is not padded silently")
        pieces, head = self._take(self._enc, wav, final, -1, self.hop, self.min_first_samples, lambda have: EngineError(
            f"streaming encode: the first push of an utterance must hold at least {self.min_first_samples} samples (the offline call's "
            "reflected left padding spans them); shorter utterances go through the offline call"))
        frames = sum(self.engine.frames(p.shape[-1]) if f & FC_SLOT_FINAL else p.shape[-1] // self.hop for p, f in pieces)
        if one_push:
            self._one_push(pieces, "streaming encode")
        self._fits(self._enc, frames, "encode")
        self._enc.head = head
        if not pieces:
            D = self.arch.dimension
            empty = (self.n_q, self.batch, 0) if not self.arch.bypass_quantizer else (self.batch, 0)
            none = torch.empty((self.batch, 0, D), device=self.device)
            return (torch.empty(empty, dtype=torch.int64, device=self.device), none) + ((none,) if want_enc_out else ())
        self._enc.started = True
        self._enc.frames += frames
        outs = [self._encode_call(part.contiguous(), bool(f & FC_SLOT_FINAL), want_enc_out) for part, f in pieces]
        res = (torch.cat([o[0] for o in outs], -1), torch.cat([o[1] for o in outs], 1))
        return res + ((torch.cat([o[2] for o in outs], 1),) if want_enc_out else ())

    # -- decode --------------------------------------------------------------------------------
    def _decode_pushes(self, x: torch.Tensor, final: bool, call, rows_apply: bool = False) -> torch.Tensor:
        name = "tokens" if x.dtype == torch.int64 else "emb"
        if x.shape[0] != self.batch:
            raise EngineError(f"this session streams {self.batch} utterances, got {x.shape[0]}")
        pieces, head = self._take(self._dec, x, final, 1, 1, self.min_first_frames, lambda have: EngineError(
            f"streaming decode: the utterance ends after {have} frames, fewer than the {self.min_first_frames} the "
            "first push must hold (the offline call's reflected left padding spans them); decode it with the offline call"))
        frames = sum(p.shape[1] for p, _ in pieces)
        self._fits(self._dec, frames, "decode")
        self._dec.head = head
        if not pieces:
            return torch.empty((self.batch, self.engine.channels, 0), dtype=torch.float32, device=self.device)
        self._dec.started = True
        self._dec.frames += frames
        outs = []
        for part, _ in pieces:
            kf = None
            if name == "tokens" and self.per_frame:     # the last column: the frames' stage counts (_with_counts)
                kf = self._given("frame_nq", part[..., self.n_q].to(torch.int32).contiguous())
                part = part[..., :self.n_q]
            part = self._given(name, part.contiguous())
            wav = self._buf("wav_out", (self.batch, self.engine.channels, part.shape[1] * self.hop), torch.float32)
            ws = self._push_ws()
            with self._push_stream(), self._engine_row_nq(self._push_row_nq() if rows_apply and kf is None else None), \
                    self._engine_push_frame_nq(kf):
                self.engine._check(call(part, wav, ws))
            outs.append(self._out(wav))
        return outs[0] if len(outs) == 1 else torch.cat(outs, -1)

    @_on_device
    def decode(self, codes: torch.Tensor, use_scale: bool = True, final: bool = False, n_q_frames=None) -> torch.Tensor:
        """codes [B,Tf,n_q] (the reference's token layout) -> wav [B,C,Tf*hop].  final=True says the utterance ends here: it changes no
        sample (the decoder has no right padding) but raises if frames are still held back, instead of returning nothing for ever.
        n_q_frames [B,Tf] (a per_frame session alone): frame (b, t) sums its first n_q_frames[b, t] codes; without it every frame of a
        row takes the row's count, as in any session."""
        codes = self.engine._dev(codes, torch.int64)
        if codes.dim() != 3 or codes.shape[2] != self.n_q:
            raise EngineError(f"codes must be [B,Tf,{self.n_q}], got {tuple(codes.shape)}")
        if n_q_frames is not None and not self.per_frame:
            raise EngineError("decode: n_q_frames is for a session opened with per_frame=True")
        if self.per_frame:
            if n_q_frames is None and self._row_nq is not None and codes.shape[0] == self.batch:
                n_q_frames = torch.tensor(self._row_nq, dtype=torch.int64).view(-1, 1).expand(codes.shape[0], codes.shape[1])
            codes = self._with_counts(codes, n_q_frames, self.n_q, "decode")
        return self._decode_pushes(codes, final, lambda part, wav, ws: self.lib.fc_stream_decode_codes(
            self._h, _ptr(part), part.shape[1], int(use_scale), _ptr(wav), None, _ptr(ws), ws.numel(), self.engine._stream()), rows_apply=True)

    @_on_device
    def decode_packed(self, packets, final: bool = False, use_scale: bool = True) -> torch.Tensor:
        """The inverse of ``encode(..., packed=True)``: a list of B packets (``bytes``) of equal frame count -> wav [B,C,Tf*hop], every row
        decoded with the stage count its packet carries (the session's own counts are untouched); final as in decode."""
        self._packed_check()
        if len(packets) != self.batch:
            raise EngineError(f"this session streams {self.batch} utterances, got {len(packets)} packets")
        if self.per_frame:      # packets of either mode, mixed: tokens and a count per frame on the device, nothing of the session changed
            tokens, kf, frames = self._unpack_rows_frames(packets, "decode_packed")
            if any(f != frames[0] for f in frames):
                raise EngineError(f"decode_packed: the utterances of this session advance in lock-step, the packets hold {frames} frames")
            return self.decode(tokens, use_scale=use_scale, final=final, n_q_frames=kf)
        tokens, frames, counts = self._unpack_rows(packets, "decode_packed")
        if any(f != frames[0] for f in frames):
            raise EngineError(f"decode_packed: the utterances of this session advance in lock-step, the packets hold {frames} frames")
        keep, self._row_nq = self._row_nq, counts
        try:
            return self.decode(tokens, use_scale=use_scale, final=final)
        finally:
            self._row_nq = keep

    @_on_device
    def decode_emb(self, emb: torch.Tensor, use_scale: bool = True, final: bool = False) -> torch.Tensor:
        """emb [B,Tf,D] -> wav [B,C,Tf*hop]; final as in decode"""
        emb = self.engine._dev(emb, torch.float32)
        if emb.dim() != 3 or emb.shape[2] != self.arch.dimension:
            raise EngineError(f"emb must be [B,Tf,{self.arch.dimension}], got {tuple(emb.shape)}")
        return self._decode_pushes(emb, final, lambda part, wav, ws: self.lib.fc_stream_decode_emb(
            self._h, _ptr(part), part.shape[1], int(use_scale), _ptr(wav), _ptr(ws), ws.numel(), self.engine._stream()))

    @_on_device
    def lstm_forward(self, x: torch.Tensor, decoder: bool = False) -> torch.Tensor:
        """Test hook (fc_stream_lstm_forward): the SLSTM stage of a push alone, without the res_seq skip, on the session's encoder /
        decoder LSTM state: x [B,H,T] -> [B,H,T]; consecutive calls continue one recurrence."""
        x = self.engine._dev(x, torch.float32)
        B, H, T = x.shape
        if B != self.batch or H != self.arch.bottleneck_channels:
            raise EngineError(f"lstm_forward: x must be [{self.batch},{self.arch.bottleneck_channels},T], got {tuple(x.shape)}")
        y, ws, eng = torch.empty_like(x), self._lstm_scratch(x), self.engine
        eng._check(self.lib.fc_stream_lstm_forward(self._h, int(decoder), _ptr(x), T, _ptr(y), _ptr(ws), ws.numel(), eng._stream()))
        return y

    def seq_forward(self, x: torch.Tensor, decoder: bool = False) -> torch.Tensor:
        """Test hook (fc_seqstream_forward; CodecEngine.stream_seq_forward): the transformer stage of a push alone, without the res_seq
        skip, on the session's encoder / decoder key / value cache: x [B,C,T] -> [B,C,T]; consecutive calls continue one utterance."""
        return self.engine.stream_seq_forward(self, x, decoder=decoder)


class StreamSlots(_Session):
    """``slots`` independent utterances streamed through ONE batch; obtained from ``EncodecMI355X.open_slots``.

    A push is bound by its launches, so 32 callers in one push cost about what one costs.  Each slot holds one utterance at a
    time and does, per slot, what ``CodecStream`` does for its batch: the pushes of one utterance add up to the offline call on that
    utterance alone, whatever the other slots do in the meantime.

    * ``encode({slot: (wav, final)}) -> {slot: (codes [n_q,Tf], quantized [Tf,D])}`` (plus the encoder output [Tf,D] with
      ``want_enc_out``); ``wav`` is [C,T] or [T]; a bare tensor means ``final=False``.  Every push of a slot but its final one is a
      positive multiple of ``hop`` samples.  Slots that are not named sit idle; slots that emitted nothing are not in the result.
    * ``decode({slot: (codes [Tf,n_q], final)})`` / ``decode_emb({slot: (emb [Tf,D], final)}) -> {slot: wav [C,Tf*hop]}``.
    * ``encode(pushes, packed=True) -> (results, {slot: bytes})``: one packet per slot that emitted frames, with the slot's own frames and
      stage count (an idle slot gives none); ``decode_packed({slot: packet | (packet, final)})`` is the inverse.
    * ``start(slot, scale=None, n_q=None)`` begins the next utterance of a slot (a fresh session has every slot started, scale 1); on a
      slot whose utterance is still running it abandons that utterance.  There is no ``end``: the final push ends an utterance.
    * ``set_n_q(slot, n_q)``: the slot's stage count, in [1, the session's n_q], for the pushes that follow -- at any time between
      pushes, in the middle of an utterance too; ``start`` sets it as well (``None``: all n_q of the session).  The session's ``n_q`` is
      the most any slot may use and the first dimension of every slot's codes: a slot with fewer stages gets zeros at the later ones,
      everything else is what a session with that ``n_q`` gives it, and ``decode`` does not read its codes behind its count.

    * ``open_slots(..., noise_floor_db=, min_n_q=)``, ``start(slot, noise_floor_db=)``, ``set_noise_floor(slot, db | None)``: a noise floor per
      slot, as for ``CodecStream``: every encode push chooses the slot's stage count on the device from the slot's own frames of that push
      (a silent caller costs ``min_n_q`` stages); ``set_n_q`` remains the cap; a slot without a floor keeps its fixed count; an idle slot
      is left alone.  ``last_n_q_rows`` reads the counts back once, {slot: k}; the packets of ``encode(packed=True)`` carry them.

    * ``open_slots(..., per_frame=True)``: as for ``CodecStream`` ("Noise floor per frame"): under a floor every frame of a slot's push takes
      its own count (``min_n_q`` may be 0), ``last_n_q_frames`` is {slot: device int32 [its frames of the last push]}, packets are of mode 1
      and ``decode_packed`` takes either mode, mixed in one push.  ``SlotRecord`` is what it was: ``per_frame`` belongs to the session.

    Per slot: pushes are held back until ``min_first_samples`` / ``min_first_frames`` have arrived, then everything held comes
    out at once; an utterance that ends shorter than that raises (the offline call's job); what is longer than ``max_chunk`` is split.
    A call is checked as a whole before anything is pushed: a refused call changes nothing, and neither does a call whose first push
    the library refuses by one of its rules (it refuses before its first launch).  Any other error from the library -- a push that
    fails after it has begun, or a refusal after part of the call has been pushed -- invalidates every slot until it is restarted with
    ``start``, as the library itself then demands.

    Volume scale: one per utterance, set at ``start`` (default 1; a slot that was never started has scale 1).  It reaches the library
    with the utterance's first encode push and with its first decode push, so ``decode(use_scale=True)`` multiplies by it in a slot
    that only decodes as well.

    Transformer bottleneck.  As for ``CodecStream``, a causal net with ``seq_model: transformer`` needs ``max_frames``, the most frames
    one slot's utterance may hold per side (fc_seqslots_create): every slot has its own key / value cache and its own position in it,
    which ``start`` puts back to 0.  A call that would take a slot past the bound raises before anything is pushed, names the slot and
    changes nothing; ``start(slot)`` begins its next utterance.  Without ``max_frames`` such a net is refused, with it any other net is.

    Graph replay (``graph=True``, off by default).  As for ``CodecStream``: every push of a slot session is a steady one (START, FINAL and
    idle rows are data in device memory, copied in front of the replay), so every push replays once its key -- form, width, parity, n_q,
    use_scale, pointers -- has been captured.  The session owns fixed buffers, a workspace and a stream, and what ``encode`` / ``decode``
    RETURN ARE COPIES: the next push overwrites the buffers.  With ``max_frames`` too (every row's cache position is read on the device).
    """

    _family = "fc_slots"
    _cached_family = "fc_seqslots"
    _graph_family = "fc_graphslots"

    def __init__(self, model, slots: int, n_q: Optional[int] = None, max_chunk: Optional[int] = None, max_frames: Optional[int] = None,
                 graph: bool = False, rvq_beam: Optional[int] = None, noise_floor_db=None, min_n_q: int = 1, per_frame: bool = False):
        self.slots = int(slots)
        self.pad_value = 0.0          # what the assembled batch holds behind a row's count and in idle rows (never read; a test aid)
        super().__init__(model, self.slots, n_q, max_chunk, max_frames, graph, rvq_beam, min_n_q, per_frame)
        self._last_nqf: Dict[int, torch.Tensor] = {}       # per_frame: {slot: the counts of its frames of the last encode push under a floor}
        if noise_floor_db is not None and not isinstance(noise_floor_db, numbers.Real):
            noise_floor_db = noise_floor_db.tolist() if hasattr(noise_floor_db, "tolist") else list(noise_floor_db)
            if len(noise_floor_db) != self.slots:
                raise EngineError(f"noise_floor_db must hold one entry per slot ({self.slots}), got {len(noise_floor_db)}")
        else:
            noise_floor_db = [noise_floor_db] * self.slots
        self._floor_db = [self._checked_floor(v) for v in noise_floor_db]
        self._enc = [_Side() for _ in range(self.slots)]
        self._dec = [_Side() for _ in range(self.slots)]
        self._scale = [1.0] * self.slots
        self._poisoned = [False] * self.slots
        self._row_nq = [self.n_q] * self.slots

    def _slot(self, slot) -> int:
        if not isinstance(slot, int) or not 0 <= slot < self.slots:
            raise EngineError(f"this session has slots 0 .. {self.slots - 1}, got {slot!r}")
        return slot

    def set_n_q(self, slot: int, n_q: int) -> None:
        """the slot's stage count for the pushes that follow; a refused call changes nothing"""
        slot = self._slot(slot)
        self._row_nq[slot] = self._checked_row_nq([n_q], 1)[0]

    def set_noise_floor(self, slot: int, db) -> None:
        """the slot's noise_floor_db for the encode pushes that follow (None: the slot returns to its fixed n_q); between pushes, in the
        middle of an utterance too; a refused call changes nothing"""
        slot = self._slot(slot)
        self._floor_db[slot] = self._checked_floor(db)

    @property
    def last_n_q_rows(self) -> Dict[int, int]:
        """{slot: the stage count the slot's last encode push under a noise floor chose} (0: none yet), by ONE read-back of the session's
        device table; a slot that was idle in a push keeps its entry"""
        return dict(enumerate(self._nq_table.tolist()))

    @property
    def last_n_q_frames(self) -> Dict[int, torch.Tensor]:
        """a per_frame session: {slot: device int32 [its frames of the last encode push]} for the slots that emitted frames in the last
        encode push under a noise floor (a slot without a floor holds its cap in every frame); nothing is read back until the caller
        asks a tensor for its values"""
        return dict(self._last_nqf)

    _KEEP = object()

    def start(self, slot: int, scale=None, n_q=None, noise_floor_db=_KEEP) -> None:
        slot = self._slot(slot)
        n_q = self.n_q if n_q is None else self._checked_row_nq([n_q], 1)[0]      # refused before the slot is touched
        if noise_floor_db is not self._KEEP:                                      # not given: the slot keeps the floor it has
            self._floor_db[slot] = self._checked_floor(noise_floor_db)
        self._row_nq[slot] = n_q
        self._enc[slot], self._dec[slot] = _Side(), _Side()
        self._scale[slot] = 1.0 if scale is None else float(torch.as_tensor(scale).reshape(()))
        self._poisoned[slot] = False

    # -- the slot record: export a running call, import it in another session (csrc/slots_kernels.h states the record) ------------
    def _exportable(self, slot) -> int:
        slot = self._slot(slot)
        if self._poisoned[slot]:
            raise EngineError(f"slot {slot}: a push of this session failed inside the library: the slot's state is invalid and is not exported; "
                              f"start({slot}) begins the next utterance")
        return slot

    @_on_device
    def export(self, slot: int) -> "SlotRecord":
        """Everything the slot's utterance in flight owns, as a ``SlotRecord``: the device floats of the library's record and their meta
        (none while the slot still gathers its start-up: its record is the held pieces alone), the held-back pieces and counters of both
        sides, the slot's n_q, noise floor and scale.  The slot is only read and goes on as before, so export + import is also a fork."""
        slot = self._exportable(slot)
        enc, dec = self._enc[slot].copy(), self._dec[slot].copy()
        floats = meta = None
        if enc.running or dec.running:
            buf, metas = self._export_rows(self.lib.fc_slotrec_export, [slot], [(enc, dec)])
            meta = metas[0]
            floats = buf[0, :self._record_floats(enc, dec)].clone()
        return SlotRecord(floats, meta, enc, dec, self._row_nq[slot], self._floor_db[slot], self._scale[slot])

    def _importable(self, slot, n_q: int, floor, dec: Optional[_Side] = None) -> int:
        """what import_slot and migrate refuse before touching anything"""
        slot = self._slot(slot)
        if dec is not None and not self.per_frame and any(t.dtype == torch.int64 and t.shape[-1] == self.n_q + 1 for t in dec.head):
            raise EngineError(f"slot {slot}: the record's held decode frames carry a stage count per frame (a per_frame session's); "
                              "a session opened with per_frame=True takes it; nothing was changed")
        if any(self._poisoned):
            bad = [b for b, p in enumerate(self._poisoned) if p]
            raise EngineError(f"slot {slot}: a push of this session failed inside the library (slots {bad} await start()); it takes no record "
                              "until they are restarted; nothing was changed")
        if n_q > self.n_q:
            raise EngineError(f"slot {slot}: the record's n_q = {n_q} exceeds this session's n_q = {self.n_q} (the first dimension of its codes); "
                              "nothing was changed")
        self._checked_floor(floor)
        return slot

    def _adopt(self, slot: int, enc: _Side, dec: _Side, n_q: int, floor, scale: float) -> None:
        """the wrapper's side of an import: whatever the slot held is abandoned, as start() does"""
        self._row_nq[slot], self._floor_db[slot], self._scale[slot] = int(n_q), floor, float(scale)
        self._enc[slot], self._dec[slot] = enc.copy(device=self.device), dec.copy(device=self.device)
        if self.per_frame:      # held decode frames of a session without per_frame: every one with the record's count
            self._dec[slot].head = [self._with_counts(t, None, int(n_q), f"slot {slot}") if t.dtype == torch.int64 and t.shape[-1] == self.n_q else t
                                    for t in self._dec[slot].head]
        self._poisoned[slot] = False

    def _import_rows(self, slots: List[int], buf: torch.Tensor, metas) -> None:
        n = len(slots)
        arr = (_lib.FcSlotMeta * n)(*[_lib.FcSlotMeta(*m) for m in metas])
        with self._push_stream():
            rc = self.lib.fc_slotrec_import(self._h, n, (C.c_int32 * n)(*slots), _ptr(buf), buf.shape[-1], arr, self.engine._stream())
        if rc not in (0, 1):                            # 1: a refusal, nothing changed.  Anything else: the library has invalidated the slots it named
            for b in slots:
                self._poisoned[b] = True
        self.engine._check(rc)

    @_on_device
    def import_slot(self, slot: int, rec: "SlotRecord") -> None:
        """Slot `slot` takes the call that `rec` holds -- from any ``StreamSlots`` (other slots, max_chunk, max_frames, graph=) or
        ``CodecStream`` of a model with the same architecture -- and abandons what it held, as ``start`` does; the call then goes on bit
        for bit as if it had never moved.  Refused before anything is touched: a record whose n_q exceeds the session's, a session
        with invalidated slots, and whatever the library refuses (another layout, frames past max_frames, cache against no cache)."""
        slot = self._importable(slot, rec.n_q, rec.noise_floor_db, rec.dec)
        if rec.floats is not None:
            floats = self.engine._dev(rec.floats, torch.float32).reshape(1, -1)
            self._import_rows([slot], floats, [rec.meta])
        self._adopt(slot, rec.enc, rec.dec, rec.n_q, rec.noise_floor_db, rec.scale)

    @_on_device
    def migrate(self, dst: "StreamSlots", mapping: Dict[int, int]) -> None:
        """{slot here: slot of dst}: the named calls continue in `dst` -- ONE export launch here, ONE import launch there, the floats
        never leave the device, the buffer sized by the largest frame count among the named slots.  Frees nothing: the slots here go on
        as before (``start`` reuses them).  Checked as a whole before anything is touched.  `dst` may be this session (slots copied or
        exchanged in place): every record is exported before any is imported, and the wrapper's state is taken before any slot adopts."""
        pairs = [(self._exportable(a), b) for a, b in mapping.items()]
        seen = set()
        for a, b in pairs:
            dst._importable(b, self._row_nq[a], self._floor_db[a], self._dec[a])
            if b in seen:
                raise EngineError(f"slot {b}: named twice as a destination; nothing was changed")
            seen.add(b)
        moving = [(a, b) for a, b in pairs if self._enc[a].running or self._dec[a].running]
        if moving:
            buf, metas = self._export_rows(self.lib.fc_slotrec_export, [a for a, _ in moving], [(self._enc[a], self._dec[a]) for a, _ in moving])
            if buf.device != dst.device:
                buf = buf.to(dst.device)
            with torch.cuda.device(dst.device):
                dst._import_rows([b for _, b in moving], buf, metas)
        # what the wrapper keeps, taken before any slot adopts: dst may be this session, a destination may be another pair's source
        held = [(b, self._enc[a].copy(), self._dec[a].copy(), self._row_nq[a], self._floor_db[a], self._scale[a]) for a, b in pairs]
        for item in held:
            dst._adopt(*item)

    # -- what CodecStream does for its batch, per slot ------------------------------------------------
    def _plan(self, sides, pushes, tdim, unit, min_first, what):
        """Per named slot: the pieces [(tensor, flags)] this call pushes for it (none while it gathers its start-up) and the slot's
        state afterwards.  Raises before anything is changed."""
        plan = {}
        for slot, item in pushes.items():
            slot = self._slot(slot)
            x, final = item if isinstance(item, tuple) else (item, False)
            sd = sides[slot]
            n = x.shape[tdim]
            if self._poisoned[slot]:
                raise EngineError(f"slot {slot}: a push of this session failed inside the library; start({slot}) begins the next utterance")
            if sd.ended:
                raise EngineError(f"slot {slot}: the utterance took its final push; start({slot}) begins the next one")
            if n < 1 or (unit > 1 and not final and n % unit != 0):
                raise EngineError(f"slot {slot}: every push but the final one must be a positive multiple of the hop ({self.hop} samples), "
                                  f"got {n}; it is not padded silently")
            pieces, head = self._take(sd, x, bool(final), tdim, unit, min_first, lambda have: EngineError(
                f"slot {slot}: the utterance ends after {have} {what}, fewer than the {min_first} the first push must hold "
                "(the offline call's reflected left padding spans them); it goes through the offline call"))
            frames = sum(self.engine.frames(p.shape[tdim]) if unit > 1 and f & FC_SLOT_FINAL else p.shape[tdim] // unit for p, f in pieces)
            if self.max_frames is not None and sd.frames + frames > self.max_frames:      # _fits, per slot
                raise EngineError(f"slot {slot}: this call's {frames} frames would take the utterance to {sd.frames + frames} frames, past the "
                                  f"session's max_frames = {self.max_frames} (the size of its key / value cache); nothing was changed, "
                                  f"start({slot}) begins the next utterance")
            plan[slot] = (pieces, head, bool(pieces), bool(pieces) and bool(final), sd.frames + frames)
        return plan

    def _run(self, sides, plan, call) -> Dict[int, List]:
        """commit the plan and push its pieces round by round: round r holds piece r of every slot that has one"""
        before = {slot: (sides[slot].head, sides[slot].started, sides[slot].ended, sides[slot].frames) for slot in plan}
        for slot, (pieces, head, started, ended, frames) in plan.items():
            sides[slot].head, sides[slot].started, sides[slot].ended, sides[slot].frames = head, started, ended, frames
        outs: Dict[int, List] = {}
        rounds = max((len(v[0]) for v in plan.values()), default=0)
        r = 0
        try:
            for r in range(rounds):
                rows = {slot: v[0][r] for slot, v in plan.items() if r < len(v[0])}
                for slot, res in call(rows).items():
                    outs.setdefault(slot, []).append(res)
        except EngineError as err:
            # the library's rule refusals ("slot encode: ..." / "slot decode: ...", slots_check) come before its first launch and change
            # nothing there: if nothing of this call has been pushed either, the call is undone here too
            if r == 0 and str(err).startswith(("slot encode:", "slot decode:")):
                for slot, (head, started, ended, frames) in before.items():
                    sides[slot].head, sides[slot].started, sides[slot].ended, sides[slot].frames = head, started, ended, frames
            else:
                self._poisoned = [True] * self.slots
            raise
        return outs

    def _counts(self, rows, length):
        counts, flags = (C.c_int32 * self.slots)(), (C.c_int32 * self.slots)()
        for slot, (x, f) in rows.items():
            counts[slot], flags[slot] = length(x), f
        return counts, flags

    # -- encode --------------------------------------------------------------------------------------
    def _encode_call(self, rows, want_enc_out):
        S, D, ch = self.slots, self.arch.dimension, self.engine.channels
        counts, flags = self._counts(rows, lambda w: w.shape[-1])
        Tc = max(counts)
        Tf = self.engine.frames(Tc)
        wav = self._buf("wav_in", (S, ch, Tc), torch.float32).fill_(self.pad_value)
        scale = None
        for slot, (w, f) in rows.items():
            wav[slot, :, :w.shape[-1]] = w
            if f & FC_SLOT_START and scale is None:
                scale = torch.ones(S, dtype=torch.float32)
        if scale is None and self._g is not None:
            scale = torch.ones(S, dtype=torch.float32)         # one pointer whether a row STARTs or not (it is read for START rows only): one key
        if scale is not None:
            for slot, (w, f) in rows.items():
                if f & FC_SLOT_START:
                    scale[slot] = self._scale[slot]
            scale = self._given("scale", scale.to(self.device))
        codes = self._buf("codes", (self.n_q, S, Tf), torch.int64)
        quant = self._buf("quantized", (S, Tf, D), torch.float32)
        enc = self._buf("enc_out", (S, Tf, D), torch.float32) if (self.arch.bypass_quantizer or want_enc_out) else None
        ws = self._push_ws()
        with self._push_stream(), self._engine_row_nq(self._push_row_nq()), self._engine_rvq_beam(), self._engine_floor(Tf):
            self.engine._check(self.lib.fc_slots_encode(self._h, _ptr(wav), Tc, counts, flags, _ptr(scale), _ptr(codes), _ptr(quant), _ptr(enc),
                                                        _ptr(ws), ws.numel(), self.engine._stream()))
        out = {}
        self._last_nqf = {}
        table = None if self._nqf is None else self._nqf.clone()      # the table is the next push's to overwrite: ONE copy, on the device
        for slot, (w, f) in rows.items():
            n = self.engine.frames(w.shape[-1]) if f & FC_SLOT_FINAL else w.shape[-1] // self.hop
            if table is not None and n > 0:
                self._last_nqf[slot] = table[slot, :n]
            if self.arch.bypass_quantizer:     # codec_basic.py:700-701: the encoder output in place of the quantised embeddings
                e = self._out(enc[slot, :n])
                out[slot] = (torch.zeros((n,), dtype=torch.long, device=self.device), e, e)
            else:
                out[slot] = (self._out(codes[:, slot, :n]), self._out(quant[slot, :n]), self._out(enc[slot, :n]) if enc is not None else None)
        return out

    @_on_device
    def encode(self, pushes, want_enc_out: bool = False, packed: bool = False):
        """packed=True: returns (results, packets) with packets = {slot: bytes}: one packet per slot that emitted frames in this call,
        holding the slot's own frames at its own stage count (one pack launch and one copy for the whole push); an idle slot, or one still
        gathering its start-up, gives no packet."""
        if packed:
            self._packed_check()
        floor = self._push_floor() is not None
        res = self._encode(pushes, want_enc_out, one_push=packed and floor)
        if not packed:
            return res
        slots = [slot for slot, r in res.items() if r[0].shape[-1] > 0]
        if not slots:
            return res, {}
        frames = [int(res[slot][0].shape[-1]) for slot in slots]
        codes = torch.zeros((self.n_q, len(slots), max(frames)), dtype=torch.int64, device=self.device)
        for j, slot in enumerate(slots):
            codes[:, j, :frames[j]] = res[slot][0]
        if floor and self.per_frame:        # mode 1: the DEVICE counts per frame of the push (a slot without a floor: its cap in every frame)
            kf = torch.zeros((len(slots), max(frames)), dtype=torch.int32, device=self.device)
            for j, slot in enumerate(slots):
                kf[j, :frames[j]] = self._last_nqf[slot]
            return res, dict(zip(slots, self._pack_rows(codes, frames, None, kf)))
        # under a floor: the DEVICE counts of the push (a slot without a floor had its cap written there), every packet carries its k_b
        counts = self._nq_table[torch.tensor(slots, device=self.device)] if floor else [self._row_nq[slot] for slot in slots]
        return res, dict(zip(slots, self._pack_rows(codes, frames, counts)))

    def _encode(self, pushes, want_enc_out: bool = False, one_push: bool = False) -> Dict[int, Tuple[torch.Tensor, ...]]:
        ch = self.engine.channels

        def as_ct(item):
            w, final = item if isinstance(item, tuple) else (item, False)
            w = self.engine._dev(torch.as_tensor(w), torch.float32)
            if w.dim() == 1:
                w = w.unsqueeze(0)
            if w.dim() != 2 or w.shape[0] != ch:
                raise EngineError(f"a slot's wav must be [{ch},T]" + (" or [T]" if ch == 1 else "") + f", got {tuple(w.shape)}")
            return w, final
        pushes = {slot: as_ct(item) for slot, item in pushes.items()}
        plan = self._plan(self._enc, pushes, -1, self.hop, self.min_first_samples, "samples")
        if one_push:
            for slot, v in plan.items():
                self._one_push(v[0], f"slot {slot}")
        outs = self._run(self._enc, plan, lambda rows: self._encode_call(rows, want_enc_out))
        cat = lambda parts, i, dim: torch.cat([p[i] for p in parts], dim) if len(parts) > 1 else parts[0][i]
        return {slot: (cat(parts, 0, -1), cat(parts, 1, 0)) + ((cat(parts, 2, 0),) if want_enc_out else ()) for slot, parts in outs.items()}

    # -- decode --------------------------------------------------------------------------------------
    def _decode_call(self, rows, use_scale, emb):
        S, ch, inner = self.slots, self.engine.channels, (self.arch.dimension if emb else self.n_q)
        counts, flags = self._counts(rows, lambda t: t.shape[0])
        Tf = max(counts)
        if emb:
            x = self._buf("emb", (S, Tf, inner), torch.float32).fill_(self.pad_value)
        else:
            x = self._buf("tokens", (S, Tf, inner), torch.int64).zero_()
        kf = None
        if not emb and self.per_frame:          # the last column of a slot's rows: its frames' stage counts (_with_counts)
            kf = self._buf("frame_nq", (S, Tf), torch.int32).zero_()
            for slot, (t, f) in rows.items():
                kf[slot, :t.shape[0]] = t[:, inner]
            rows = {slot: (t[:, :inner], f) for slot, (t, f) in rows.items()}
        for slot, (t, f) in rows.items():
            x[slot, :t.shape[0]] = t
        starts = [slot for slot, (t, f) in rows.items() if f & FC_SLOT_START]
        if starts:      # the utterance's scale, for a slot whose encoder has not set it: the first S floats of the state (funcodec_amd.h)
            vals = torch.tensor([self._scale[slot] for slot in starts], dtype=torch.float32).to(self.device)
            self.state[:4 * S].view(torch.float32)[torch.tensor(starts, device=self.device)] = vals
        wav = self._buf("wav_out", (S, ch, Tf * self.hop), torch.float32)
        ws = self._push_ws()
        with self._push_stream():
            if emb:
                rc = self.lib.fc_slots_decode_emb(self._h, _ptr(x), Tf, counts, flags, int(use_scale), _ptr(wav), _ptr(ws), ws.numel(),
                                                  self.engine._stream())
            else:
                with self._engine_row_nq(self._push_row_nq() if kf is None else None), self._engine_push_frame_nq(kf):
                    rc = self.lib.fc_slots_decode_codes(self._h, _ptr(x), Tf, counts, flags, int(use_scale), _ptr(wav), None, _ptr(ws), ws.numel(),
                                                        self.engine._stream())
        self.engine._check(rc)
        return {slot: (self._out(wav[slot, :, :t.shape[0] * self.hop]),) for slot, (t, f) in rows.items()}

    def _decode(self, pushes, use_scale, emb, n_q_frames=None):
        inner, dtype = (self.arch.dimension, torch.float32) if emb else (self.n_q, torch.int64)

        def as_tn(item):
            t, final = item if isinstance(item, tuple) else (item, False)
            t = self.engine._dev(torch.as_tensor(t), dtype)
            if t.dim() != 2 or t.shape[1] != inner:
                raise EngineError(f"a slot's {'emb' if emb else 'codes'} must be [Tf,{inner}], got {tuple(t.shape)}")
            return t, final
        pushes = {slot: as_tn(item) for slot, item in pushes.items()}
        if n_q_frames is not None and (emb or not self.per_frame):
            raise EngineError("decode: n_q_frames is for a session opened with per_frame=True")
        if not emb and self.per_frame:          # every frame with its stage count: the table's, else the slot's own count
            given = {self._slot(slot): v for slot, v in (n_q_frames or {}).items()}
            pushes = {slot: (self._with_counts(t, given.get(self._slot(slot)), self._row_nq[self._slot(slot)], f"slot {slot}"), final)
                      for slot, (t, final) in pushes.items()}
        plan = self._plan(self._dec, pushes, 0, 1, self.min_first_frames, "frames")
        outs = self._run(self._dec, plan, lambda rows: self._decode_call(rows, use_scale, emb))
        return {slot: torch.cat([p[0] for p in parts], -1) if len(parts) > 1 else parts[0][0] for slot, parts in outs.items()}

    @_on_device
    def decode(self, pushes, use_scale: bool = True, n_q_frames=None) -> Dict[int, torch.Tensor]:
        """{slot: (codes [Tf,n_q], final)} -> {slot: wav [C,Tf*hop]}.  final=True says the slot's utterance ends here: it changes no sample
        but raises if frames are still held back, and the slot then needs ``start``.  n_q_frames {slot: [Tf]} (a per_frame session
        alone): a stage count per frame of the slot's codes; a slot without an entry takes its own count in every frame."""
        return self._decode(pushes, use_scale, False, n_q_frames)

    @_on_device
    def decode_packed(self, pushes, use_scale: bool = True) -> Dict[int, torch.Tensor]:
        """The inverse of ``encode(..., packed=True)``: {slot: packet | (packet, final)} -> {slot: wav [C,Tf*hop]}, every slot decoded from
        its own frames with the stage count its packet carries (the slots' own counts are untouched); final as in decode."""
        self._packed_check()
        items = {self._slot(slot): (item if isinstance(item, tuple) else (item, False)) for slot, item in pushes.items()}
        if not items:
            return {}
        slots = list(items)
        if self.per_frame:      # packets of either mode, mixed in one push; nothing of the session is changed
            tokens, kf, frames = self._unpack_rows_frames([items[slot][0] for slot in slots], "decode_packed")
            return self.decode({slot: (tokens[j, :frames[j]], items[slot][1]) for j, slot in enumerate(slots)}, use_scale=use_scale,
                               n_q_frames={slot: kf[j, :frames[j]] for j, slot in enumerate(slots)})
        tokens, frames, counts = self._unpack_rows([items[slot][0] for slot in slots], "decode_packed")
        keep = list(self._row_nq)
        for j, slot in enumerate(slots):
            self._row_nq[slot] = counts[j]
        try:
            return self.decode({slot: (tokens[j, :frames[j]], items[slot][1]) for j, slot in enumerate(slots)}, use_scale=use_scale)
        finally:
            self._row_nq = keep

    @_on_device
    def decode_emb(self, pushes, use_scale: bool = True) -> Dict[int, torch.Tensor]:
        """{slot: (emb [Tf,D], final)} -> {slot: wav [C,Tf*hop]}; final as in decode"""
        return self._decode(pushes, use_scale, True)

    @_on_device
    def lstm_forward(self, x: torch.Tensor, steps, start, decoder: bool = False) -> torch.Tensor:
        """Test hook (fc_slots_lstm_forward): the SLSTM stage of a slot push alone on the session's encoder / decoder LSTM state:
        x [S,H,T] -> [S,H,T]; slot b takes steps[b] <= T steps (zeros behind) and begins from zeros where start[b]."""
        x = self.engine._dev(x, torch.float32)
        S, H, T = x.shape
        if S != self.slots or H != self.arch.bottleneck_channels or len(steps) != S or len(start) != S:
            raise EngineError(f"lstm_forward: x must be [{self.slots},{self.arch.bottleneck_channels},T] with one step count and start flag per slot")
        y, ws, eng = torch.empty_like(x), self._lstm_scratch(x), self.engine
        st, fl = (C.c_int32 * S)(*[int(v) for v in steps]), (C.c_int32 * S)(*[int(bool(v)) for v in start])
        eng._check(self.lib.fc_slots_lstm_forward(self._h, int(decoder), _ptr(x), T, st, fl, _ptr(y), _ptr(ws), ws.numel(), eng._stream()))
        return y

    @_on_device
    def seq_forward(self, x: torch.Tensor, frames, start, decoder: bool = False) -> torch.Tensor:
        """Test hook (fc_seqslots_forward): the transformer stage of a slot push alone, without the res_seq skip, on the session's
        encoder / decoder key / value cache: x [S,C,T] -> [S,C,T]; slot b takes frames[b] <= T frames (zeros behind) at its own
        position, which begins at 0 where start[b]; consecutive calls continue every slot's own utterance."""
        x = self.engine._dev(x, torch.float32)
        S, Cc, T = x.shape
        if S != self.slots or Cc != self.arch.bottleneck_channels or len(frames) != S or len(start) != S:
            raise EngineError(f"seq_forward: x must be [{self.slots},{self.arch.bottleneck_channels},T] with one frame count and start flag per slot")
        y, eng = torch.empty_like(x), self.engine
        # the chunk's buffers and the partials of the attention's key split, as CodecEngine.stream_seq_forward sizes them, and the push's table
        ws = self._scratch(4 * S * T * (8 * Cc + SEQ_FF) + 4 * S * 256 * (Cc + 2 * SEQ_HEADS) + 12 * S + (1 << 20))
        fr, fl = (C.c_int32 * S)(*[int(v) for v in frames]), (C.c_int32 * S)(*[int(bool(v)) for v in start])
        eng._check(self.lib.fc_seqslots_forward(self._h, int(decoder), _ptr(x), T, fr, fl, _ptr(y), _ptr(ws), ws.numel(), eng._stream()))
        return y


# ---- the per-layer geometry of a push, restated in Python (tests/test_stream_host.py checks it against torch) ------------------
def conv_layers(arch):
    """Every conv of the 1-D encoder and decoder that carries a left context, in execution order:
    dicts(side, kind 'conv' | 'convtr', cin, cout, k, stride, dil, carry = columns carried,
    columns of its input per codec frame = cols_per_frame).  Mirrors the engine's plan (SEANetEncoder / SEANetDecoder, seanet_encoder.py:109-160,
    seanet_decoder.py:111-164)."""
    nf, out = arch.n_filters, []
    hop = 1
    for r in arch.ratios:
        hop *= r
    cpf = {"encoder": hop, "decoder": 1}          # columns of the next layer's input per codec frame

    def conv(side, cin, cout, k, stride=1, dil=1, tr=False):
        carry = 1 if tr else (k - 1) * dil - (stride - 1)
        out.append(dict(side=side, kind="convtr" if tr else "conv", cin=cin, cout=cout, k=k, stride=stride, dil=dil, carry=carry,
                        cols_per_frame=cpf[side]))
        cpf[side] = cpf[side] * stride if tr else cpf[side] // stride

    ch = arch.input_channels if arch.input_channels == 2 else 1
    mult = 1
    conv("encoder", ch, nf, arch.kernel_size)
    for ratio in reversed(list(arch.ratios)):
        c = mult * nf
        for j in range(arch.n_residual_layers):
            conv("encoder", c, c // arch.compress, arch.residual_kernel_size, 1, arch.dilation_base ** j)
        conv("encoder", c, 2 * c, 2 * ratio, ratio)
        mult *= 2
    conv("encoder", mult * nf, arch.dimension, arch.last_kernel_size)
    conv("decoder", arch.dimension, mult * nf, arch.kernel_size)
    for ratio in arch.ratios:
        c = mult * nf
        conv("decoder", c, c // 2, 2 * ratio, ratio, tr=True)
        for j in range(arch.n_residual_layers):
            conv("decoder", c // 2, c // 2 // arch.compress, arch.residual_kernel_size, 1, arch.dilation_base ** j)
        mult //= 2
    conv("decoder", nf, ch, arch.last_kernel_size)
    return out


def extra_padding(length: int, k: int, stride: int, padding_total: int) -> int:
    """get_extra_padding_for_conv1d (conv.py:57-64) in integers"""
    num = length - k + padding_total
    n_frames_ceil = -((-num) // stride) + 1
    return (n_frames_ceil - 1) * stride + (k - padding_total) - length


def chunk_geometry(layer, tc: int, final: bool):
    """(staged columns, output columns) of one push of tc input columns through `layer`: the conv runs without padding over
    [carry | chunk | extra], extra only at the final push."""
    if layer["kind"] == "convtr":
        return 1 + tc, tc * layer["stride"]
    pt = layer["carry"]
    extra = extra_padding(tc, layer["k"], layer["stride"], pt) if final else 0
    tp = pt + tc + extra
    return tp, (tp - ((layer["k"] - 1) * layer["dil"] + 1)) // layer["stride"] + 1


def min_first(arch):
    """(samples, frames): the shortest first push of an utterance for encode / decode (every layer's chunk must hold the reflected
    left padding of the offline call, carry + 1 columns); what fc_stream_min_first returns."""
    hop = 1
    for r in arch.ratios:
        hop *= r
    frames = {"encoder": 1, "decoder": 1}
    for L in conv_layers(arch):
        if L["kind"] == "conv":                   # a transposed conv starts from a zero column: nothing to hold
            frames[L["side"]] = max(frames[L["side"]], -(-(L["carry"] + 1) // L["cols_per_frame"]))
    return frames["encoder"] * hop, frames["decoder"]


# ---- the per-row staging rule of a slot push, restated in Python (tests/test_slots_host.py checks it against torch) -----------------
def slot_staged_width(layer, t: int) -> int:
    """columns of the staged buffer of a slot push whose common width at `layer` is t: it holds the widest row with the extra padding of
    a last push, whether a row of this push ends or not"""
    if layer["kind"] == "convtr":
        return 1 + t
    pt = layer["carry"]
    return pt + t + extra_padding(t, layer["k"], layer["stride"], pt)


def stage_slot_row(layer, carry, row, start: bool, final: bool, tp: int):
    """What slots_stage_kernel writes for one row of a push: (staged [cin, tp], new carry [cin, carry columns]).
    row [cin, n] is the activated input of the row's own n columns (n = 0: an idle row).  [left | row | extra if final | zeros] with
    left = the reflection of the row's own columns 1..pt at START (zeros in front of a transposed conv), else the carry; the new carry is
    the last pt columns of [left | row]; an idle row stages zeros and keeps its carry."""
    import torch.nn.functional as F
    pt, tr, n = layer["carry"], layer["kind"] == "convtr", row.shape[-1]
    if n == 0:
        return row.new_zeros(row.shape[0], tp), carry
    if start:
        if tr:
            left = row.new_zeros(row.shape[0], pt)
        else:                                          # pad1d zero-extends a row not longer than the padding before it reflects
            ext = torch.cat([row, row.new_zeros(row.shape[0], max(0, pt + 1 - n))], -1)
            left = ext[:, 1:pt + 1].flip(-1)
    else:
        left = carry
    buf = torch.cat([left, row], -1)
    new_carry = buf[:, buf.shape[-1] - pt:]
    extra = extra_padding(n, layer["k"], layer["stride"], pt) if (final and not tr) else 0
    if extra:
        buf = F.pad(buf[None], (0, extra), "reflect")[0]
    return torch.cat([buf, row.new_zeros(row.shape[0], tp - buf.shape[-1])], -1), new_carry


# ---- the slot record, restated in Python (csrc/slots_kernels.h is the specification; tests/test_slot_record_host.py counts it by hand) ----
def slot_record_segments(arch, cached: bool):
    """[(kind, side, floats)] of the library's slot record in its order: the scale, then per side (encoder, decoder) every carried conv's
    cin * carry floats, per LSTM layer h and c, and with a key / value cache per transformer block K and V, whose entry is the floats
    per cached frame column (C): such a plane holds C * seq_cache_pitch(frames of the side) floats."""
    segs = [("scale", None, 1)]
    tf = arch.lstm_layers > 0 and arch.seq_model == "transformer"
    for side in ("encoder", "decoder"):
        segs += [("carry", side, L["cin"] * L["carry"]) for L in conv_layers(arch) if L["side"] == side and L["carry"] > 0]
        for _ in range(0 if tf else arch.lstm_layers):
            segs += [("h", side, arch.bottleneck_channels), ("c", side, arch.bottleneck_channels)]
        for _ in range(arch.lstm_layers if tf and cached else 0):
            segs += [("K", side, arch.bottleneck_channels), ("V", side, arch.bottleneck_channels)]
    return segs


def slot_record_floats(arch, enc_frames: int = 0, dec_frames: int = 0, cached: bool = False) -> int:
    """the length of a slot record (fc_slotrec_floats): a side that is not running counts 0 frames"""
    pitch = {"encoder": (int(enc_frames) + 15) // 16 * 16, "decoder": (int(dec_frames) + 15) // 16 * 16}
    return sum(n * pitch[side] if kind in "KV" else n for kind, side, n in slot_record_segments(arch, cached))


SLOT_RECORD_MAGIC = b"FCSLOTRC"
SLOT_RECORD_VERSION = 1
#: what a record's tensors may be: the floats and held-back audio or embeddings (float32), held-back codes (int64)
SLOT_RECORD_DTYPES = {"float32": torch.float32, "int64": torch.int64}


class SlotRecord:
    """One call in flight, taken out of its session (``StreamSlots.export`` / ``CodecStream.export``; ``StreamSlots.import_slot`` puts it
    into another):

    * ``floats``: the library's slot record on the device (csrc/slots_kernels.h states it), cut to the frames in use, and ``meta``:
      (layout, enc_phase, dec_phase, enc_frames, dec_frames) of fc_slot_meta; both None for a slot still gathering its start-up, which
      has no device state yet;
    * ``enc`` / ``dec``: what the wrapper keeps per side -- the held-back start-up pieces, started, ended, frames;
    * ``n_q``, ``noise_floor_db``, ``scale``: the slot's stage count, noise floor and volume scale.

    The stage counts the last push chose under a noise floor do not travel.  ``to_bytes`` / ``from_bytes`` take it through host memory.
    ``meta[0]`` tells architectures apart, not checkpoints: a record continues correctly only under the weights it was made with."""

    def __init__(self, floats, meta, enc: _Side, dec: _Side, n_q: int, noise_floor_db, scale: float):
        self.floats, self.meta, self.enc, self.dec = floats, (None if meta is None else tuple(int(v) for v in meta)), enc, dec
        self.n_q, self.noise_floor_db, self.scale = int(n_q), (None if noise_floor_db is None else float(noise_floor_db)), float(scale)

    def _tensors(self):
        return ([] if self.floats is None else [self.floats]) + self.enc.head + self.dec.head

    def to_bytes(self) -> bytes:
        """magic, version, a JSON header, then the raw little-endian tensors: the record's floats and the held pieces"""
        side = lambda sd: {"started": sd.started, "ended": sd.ended, "frames": sd.frames,
                           "head": [{"shape": list(t.shape), "dtype": str(t.dtype).replace("torch.", "")} for t in sd.head]}
        header = json.dumps({"meta": self.meta, "floats": None if self.floats is None else int(self.floats.numel()), "n_q": self.n_q,
                             "noise_floor_db": self.noise_floor_db, "scale": self.scale, "enc": side(self.enc), "dec": side(self.dec)}).encode()
        body = b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in self._tensors())
        return SLOT_RECORD_MAGIC + struct.pack("<II", SLOT_RECORD_VERSION, len(header)) + header + body

    @classmethod
    def from_bytes(cls, blob: bytes, device=None) -> "SlotRecord":
        blob = bytes(blob)
        n = len(SLOT_RECORD_MAGIC)
        if blob[:n] != SLOT_RECORD_MAGIC:
            raise EngineError(f"SlotRecord.from_bytes: bad magic {blob[:n]!r}, a slot record begins with {SLOT_RECORD_MAGIC!r}")
        if len(blob) < n + 8:
            raise EngineError("SlotRecord.from_bytes: the blob ends inside its header")
        version, hlen = struct.unpack_from("<II", blob, n)
        if version != SLOT_RECORD_VERSION:
            raise EngineError(f"SlotRecord.from_bytes: version {version} is not understood, this library reads version {SLOT_RECORD_VERSION}")
        pos = n + 8
        try:
            h = json.loads(blob[pos:pos + hlen].decode())
            sides_h = [h["enc"], h["dec"]]
            pieces = [(list(p["shape"]), p["dtype"]) for sd in sides_h for p in sd["head"]]
            for sd in sides_h:
                bool(sd["started"]), bool(sd["ended"]), int(sd["frames"])
            int(h["n_q"]), float(h["scale"]), h["meta"], h["floats"], h["noise_floor_db"]
        except (ValueError, KeyError, TypeError) as err:
            raise EngineError(f"SlotRecord.from_bytes: the header is not a slot record's ({type(err).__name__}: {err})") from None
        if h["meta"] is not None and not (isinstance(h["meta"], list) and len(h["meta"]) == 5 and all(isinstance(v, int) for v in h["meta"])):
            raise EngineError(f"SlotRecord.from_bytes: header field meta holds five integers or null, got {h['meta']!r}")
        if h["floats"] is not None and not (isinstance(h["floats"], int) and h["floats"] >= 0):
            raise EngineError(f"SlotRecord.from_bytes: header field floats is a count or null, got {h['floats']!r}")
        if (h["floats"] is None) != (h["meta"] is None):
            raise EngineError("SlotRecord.from_bytes: header fields floats and meta travel together")
        if h["noise_floor_db"] is not None and not isinstance(h["noise_floor_db"], (int, float)):
            raise EngineError(f"SlotRecord.from_bytes: header field noise_floor_db is a number or null, got {h['noise_floor_db']!r}")
        for shape, dtype in pieces:
            if dtype not in SLOT_RECORD_DTYPES:
                raise EngineError(f"SlotRecord.from_bytes: header field dtype of a held piece is one of {sorted(SLOT_RECORD_DTYPES)}, got {dtype!r}")
            if not all(isinstance(v, int) and v >= 0 for v in shape):
                raise EngineError(f"SlotRecord.from_bytes: header field shape of a held piece holds counts, got {shape!r}")
        pos += hlen

        def take(shape, dtype):
            nonlocal pos
            dt = SLOT_RECORD_DTYPES[dtype]
            count = 1
            for v in shape:
                count *= int(v)
            nbytes = count * torch.empty((), dtype=dt).element_size()
            if pos + nbytes > len(blob):
                raise EngineError("SlotRecord.from_bytes: the blob is shorter than its header says")
            t = torch.frombuffer(bytearray(blob[pos:pos + nbytes]), dtype=dt).reshape(shape) if count else torch.empty(shape, dtype=dt)
            pos += nbytes
            return t if device is None else t.to(device)

        floats = None if h["floats"] is None else take([h["floats"]], "float32")
        sides = []
        for key in ("enc", "dec"):
            sd = _Side()
            sd.started, sd.ended, sd.frames = bool(h[key]["started"]), bool(h[key]["ended"]), int(h[key]["frames"])
            sd.head = [take(p["shape"], p["dtype"]) for p in h[key]["head"]]
            sides.append(sd)
        if pos != len(blob):
            raise EngineError("SlotRecord.from_bytes: the blob is longer than its header says")
        return cls(floats, h["meta"], sides[0], sides[1], h["n_q"], h["noise_floor_db"], h["scale"])
