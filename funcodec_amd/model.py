"""Drop-in for the inference surface of the reference's ``Encodec`` model
(funcodec/models/codec_basic.py:670-836) on top of :class:`funcodec_amd.engine.CodecEngine`.

Same method names, argument meaning and return dictionaries as the reference, so that
``Speech2Token`` (and LauraTTS's use of it, funcodec/bin/text2audio_inference.py:85-94,157,180-190)
can switch without touching call sites.
"""
from __future__ import annotations

import numbers
import types
from typing import Dict, Optional

import torch

from .config import ArchSpec
from .engine import CodecEngine, EngineError, packed_refusal, ragged_refusal, rate_min_nq, rate_min_nq_frames, rate_targets, row_nq_list, rvq_beam_width


class EncodecMI355X:
    def __init__(self, arch: ArchSpec, device="cuda:0"):
        self.arch = arch
        self.engine = CodecEngine(arch, device)
        self.device = self.engine.device
        # attributes other reference code reaches into
        self.quantizer = types.SimpleNamespace(
            sampling_rate=arch.quantizer_sampling_rate,
            encoder_hop_length=arch.encoder_hop_length,
            codebook_size=arch.codebook_size,
            code_dim=arch.dimension,
            get_num_quantizers_for_bandwidth=lambda sr, bw=None: arch.num_quantizers_for_bandwidth(bw),
        )
        self.sample_rate = arch.sample_rate
        self.training = False

    # nn.Module-ish no-ops so callers written against the reference keep working
    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def load_state_dict(self, state, strict: bool = False):
        self.engine.load_state_dict(state)

    def open_stream(self, batch: int, n_q: Optional[int] = None, scale: Optional[torch.Tensor] = None, max_chunk: Optional[int] = None,
                    max_frames: Optional[int] = None, graph: bool = False, rvq_beam: Optional[int] = None, noise_floor_db=None, min_n_q: int = 1,
                    per_frame: bool = False):
        """A streaming encode / decode session for `batch` utterances of a causal checkpoint (funcodec_amd/stream.py CodecStream):
        n_q quantisers (default: all; a list of `batch` counts gives every utterance its own, and ``set_n_q`` changes them between
        pushes), one volume scale per utterance (default 1), pushes of at most max_chunk samples per call.  A causal net whose bottleneck is
        a transformer (seq_model: transformer) needs max_frames, the most frames one utterance may hold per side: the size of the
        session's key / value cache.  Any other net is refused with it.  graph=True: steady pushes are replayed as captured HIP graphs
        from fixed buffers of the session, and what a push returns are copies (CodecStream, "Graph replay"); refused with max_frames.
        rvq_beam (2, 4, 8): the session's encode pushes search over the quantiser's stages (``inference(rvq_beam=)``); a frame's codes
        equal the offline call's.
        noise_floor_db (one value or one per utterance; optional) and min_n_q: every encode push chooses a stage count per row on the
        device, inside the push, by an absolute noise floor (CodecStream, "Noise floor"); n_q / ``set_n_q`` are then the caps.
        per_frame=True (a property of the session): the count is chosen per FRAME of the push (CodecStream, "Noise floor per frame"),
        min_n_q may be 0, packets are of mode 1 and ``decode_packed`` takes either mode."""
        from .stream import CodecStream
        return CodecStream(self, batch, n_q=n_q, scale=scale, max_chunk=max_chunk, max_frames=max_frames, graph=graph, rvq_beam=rvq_beam,
                           noise_floor_db=noise_floor_db, min_n_q=min_n_q, per_frame=per_frame)

    def open_slots(self, slots: int, n_q: Optional[int] = None, max_chunk: Optional[int] = None, max_frames: Optional[int] = None,
                   graph: bool = False, rvq_beam: Optional[int] = None, noise_floor_db=None, min_n_q: int = 1,
                   per_frame: bool = False):
        """A slot session of a causal checkpoint (funcodec_amd/stream.py StreamSlots): `slots` independent utterances that start, push
        and end at their own times and share every push of the batch; n_q quantisers at the most (default: all; ``start(slot, n_q=)`` and
        ``set_n_q(slot, n_q)`` give a slot fewer, at any time between pushes), at most max_chunk samples per call.  As for
        ``open_stream``, a net whose bottleneck is a transformer needs max_frames, the most frames one slot's utterance may hold per
        side (every slot has its own key / value cache and its own position in it); any other net is refused with it.  graph=True: pushes
        are replayed as captured HIP graphs from fixed buffers of the session, and what a push returns are copies (StreamSlots).
        rvq_beam, noise_floor_db, min_n_q: as for ``open_stream`` (noise_floor_db: one value or one per slot; ``start(slot,
        noise_floor_db=)`` and ``set_noise_floor(slot, db)`` change a slot's); per_frame: as for ``open_stream``."""
        from .stream import StreamSlots
        return StreamSlots(self, slots, n_q=n_q, max_chunk=max_chunk, max_frames=max_frames, graph=graph, rvq_beam=rvq_beam,
                           noise_floor_db=noise_floor_db, min_n_q=min_n_q, per_frame=per_frame)

    # -- helpers -------------------------------------------------------------------------------
    def _as_bct(self, speech: torch.Tensor) -> torch.Tensor:
        if speech.dim() == 2:
            speech = speech.unsqueeze(1)
        assert speech.dim() == 3, "speech must be [B,T] or [B,C,T]"          # codec_basic.py:342
        assert 0 < speech.shape[1] <= 2                                       # codec_basic.py:344
        if speech.shape[1] != self.engine.channels:      # the reference's first conv would raise on the channel mismatch
            raise ValueError(f"this model takes {self.engine.channels}-channel audio (config input_size), got {speech.shape[1]} channels")
        return speech

    # -- Encodec._encode / _decode with segment_dur set (codec_basic.py:334-359,382-396,77-116) --
    def _inference_segmented(self, wav: torch.Tensor, n_q: int, need_recon: bool, use_scale: bool, bypass: bool = False):
        """Every frame is an independent utterance for the engine (own volume scale, GroupNorm statistics, LSTM state), so
        all frames of equal length go through ONE engine call as extra batch rows; the ragged tail frames follow.  Like the
        reference's _decode, every frame is decoded to its FULL length ceil(len/hop)*hop (longer than the segment when the
        segment length is not a multiple of the hop), the triangle window is sized from the first decoded frame, and the
        overlap-add result is trimmed to the input length last (fc_overlap_add)."""
        B, T = wav.shape[0], wav.shape[-1]
        seg, stride = self.arch.segment_length, self.arch.segment_stride
        offsets = list(range(0, T, stride))
        lens = [min(seg, T - o) for o in offsets]
        results = [None] * len(offsets)
        by_len = {}
        for i, n in enumerate(lens):
            by_len.setdefault(n, []).append(i)
        for n, ids in by_len.items():
            stack = torch.cat([wav[..., offsets[i]:offsets[i] + n] for i in ids], 0).contiguous()   # [len(ids)*B, (C,) n]
            r = self._encode_or_bypass(stack, n_q, bypass)
            rec = None
            if need_recon:
                rec = self.engine.decode_emb(r["quantized"], r["scale"] if use_scale else None)   # untrimmed: Tf*hop samples
            for j, i in enumerate(ids):
                sl = slice(j * B, (j + 1) * B)
                results[i] = dict(codes=r["codes"][sl] if bypass else r["codes"][:, sl], quantized=r["quantized"][sl],
                                  sub_quants=r["sub_quants"][sl] if bypass else r["sub_quants"][:, sl],
                                  scale=r["scale"][sl] if r.get("scale") is not None else None,
                                  recon=rec[sl] if need_recon else None)
        recon = None
        if need_recon:
            recon = self.engine.overlap_add([r["recon"] for r in results], stride, out_len=T)
        return dict(recon_speech=recon, code_indices=[r["codes"] for r in results],
                    code_embeddings=[(r["quantized"], r["scale"] if use_scale else None) for r in results],
                    sub_quants=[r["sub_quants"] for r in results])

    def _encode_or_bypass(self, wav: torch.Tensor, n_q: int, bypass: bool):
        """engine.encode, or with model_conf.bypass_quantizer (codec_basic.py:700-701, Encodec.inference only) the encoder output in place of
        the quantised embeddings, zero indices [B, Tf] and zero sub_quants like the reference builds them."""
        if not bypass:
            return self.engine.encode(wav, n_q)
        r = self.engine.encode(wav, 1, want_sub_quants=False, want_enc_out=True)     # the quantiser's stage is computed and dropped
        emb = r["enc_out"]
        return dict(codes=torch.zeros(emb.shape[0], emb.shape[1], dtype=torch.long, device=emb.device), quantized=emb,
                    sub_quants=torch.zeros_like(emb), scale=r["scale"])

    @staticmethod
    def _one_bit_width(bit_width) -> bool:
        """one value for the whole batch (None, a Python or numpy number, a 0-dim tensor or array), as the reference takes it"""
        return bit_width is None or isinstance(bit_width, numbers.Real) or (hasattr(bit_width, "ndim") and bit_width.ndim == 0)

    def _bit_widths(self, bit_width, B: int):
        """(n_q of the call, per-row stage counts or None) of a ``bit_width`` that is one value for the batch, as in the reference, or a
        sequence / 1-D tensor of B of them: every entry goes through num_quantizers_for_bandwidth, the call's n_q is the largest."""
        if self._one_bit_width(bit_width):
            return self.arch.num_quantizers_for_bandwidth(float(bit_width) if hasattr(bit_width, "ndim") else bit_width), None
        if hasattr(bit_width, "ndim"):                 # a tensor or an array
            if bit_width.ndim != 1:
                raise EngineError(f"bit_width must be one value or a sequence / 1-D tensor of one per row, got shape {tuple(bit_width.shape)}")
            bit_width = bit_width.tolist()
        rows = row_nq_list(self.arch, [self.arch.num_quantizers_for_bandwidth(bw) for bw in bit_width], B)
        return max(rows), rows

    # -- Encodec.inference (codec_basic.py:670-718) ------------------------------------------
    @torch.no_grad()
    def inference(self, speech: torch.Tensor, need_recon: bool = True, bit_width: int = None,
                  use_scale: bool = True, _quantise_always: bool = False, speech_lengths=None, rvq_beam: int = None,
                  target_snr_db=None, min_n_q: int = 1, packed: bool = False, per_frame: bool = False) -> Dict[str, torch.Tensor]:
        """bit_width: one value for the batch, as in the reference, or a sequence / 1-D tensor of B: row b is then what this call returns
        for it with ``bit_width[b]``; ``code_indices`` is [max n_q, B, Tf] with zeros at the stages a row does not take (``sub_quants`` too).
        speech_lengths [B] (optional): samples per row.  With it, row b of every output is what this call returns for
        ``speech[b, ..., :speech_lengths[b]]`` alone (its own volume scale, GroupNorm statistics, end padding), zeros behind its
        ``engine.frames(len)`` frames / ``len`` samples; without it, the call over the whole batch width, as the reference runs it.
        rvq_beam (2, 4 or 8; optional): the quantiser searches over its stages with that many hypotheses per frame instead of taking the
        nearest code stage by stage; no frame is coded worse, the outputs keep their shapes and decode like any other.  It is set on the
        engine around this call only, and combines with ``speech_lengths`` and a per-row ``bit_width``.
        target_snr_db (one value or B of them, dB; optional): row b takes the smallest number of stages in [min_n_q, its cap] whose
        quantiser-domain SNR reaches its target (``engine.rate_pick`` states the rule; +inf: the best count), chosen on the device inside
        this one call; a per-row ``bit_width`` is the per-row cap.  Every output is then what this call returns with the ``bit_width`` of
        those counts (``rvq_beam``: the first k codes of the full-depth search).  The dict gains ``n_q_rows`` [B] int32 and ``row_snr_db``
        [B] float64 (10 log10(E[0] / E[k]) of every row at its count), both on the device; a decoder needs the counts, code 0 is a valid code.
        packed=True: the dict gains ``packets``, uint8 [B, pitch] on the device: one self-describing packet per row (csrc/code_pack_kernels.h
        states it) holding the row's own frames (``speech_lengths``) and stage count (a per-row ``bit_width``; with ``target_snr_db`` the
        counts go from the device tensor into the packer, nothing is read back).  ``engine.packets_to_host`` cuts them into bytes and
        ``inference_decoding_packed`` decodes them.  Everything else the call returns, and launches, is unchanged.
        per_frame=True (with ``target_snr_db``): a stage count per FRAME (``engine.rate_pick_frames`` states the rule; csrc/
        rvq_rate_kernels.h): frame (b, t) takes the fewest stages in [min_n_q, its row's cap] that bring it down to the row's noise
        floor, min_n_q in [0, cap] (0: a frame may take no stage).  The dict gains ``n_q_frames`` [B, Tf] int32, ``n_q_rows`` (every
        row's largest frame count), ``n_codes_rows`` [B] int32 (the sum of its frame counts) and ``row_snr_db`` (achieved: 10 log10(E[0] /
        sum_t err[k_t])); ``packets`` are then of mode 1 and carry the counts.  It composes with ``speech_lengths``, a per-row ``bit_width``
        (the caps) and ``rvq_beam``; without a target, or with ``segment_dur``, ``bypass_quantizer`` or ``q0_ds_ratio > 1``, it is refused
        before anything reaches the device."""
        if per_frame and target_snr_db is None:        # refused before anything reaches the device
            raise EngineError("per_frame chooses a stage count per frame by target_snr_db: give a target")
        if packed:                                     # refused before anything reaches the device
            why = packed_refusal(self.arch)
            if why:
                raise EngineError(why)
        if target_snr_db is not None:                  # refused before anything reaches the device
            rate_targets(self.arch, target_snr_db, speech.shape[0])
        with self.engine._rvq_beam(rvq_beam_width(self.arch, rvq_beam)):           # refused before anything reaches the device
            ret = self._inference(speech, need_recon, bit_width, use_scale, _quantise_always, speech_lengths, target_snr_db, min_n_q, per_frame)
            if packed:
                ret["packets"] = self._packets(ret, bit_width, speech_lengths)
            return ret

    def _packets(self, ret, bit_width, speech_lengths):
        """the packets of a call's codes: frames per row from the engine's own frames() of speech_lengths, counts from the call's device
        tensor (target_snr_db), else from a per-row bit_width, else every row has all stages of the call"""
        codes = ret["code_indices"][0]
        frames = None
        if speech_lengths is not None:
            frames = [self.engine.frames(int(n)) for n in torch.as_tensor(speech_lengths).reshape(-1).tolist()]
        if ret.get("n_q_frames") is not None:          # per_frame: packets of mode 1, the counts from the call's device tensor
            return self.engine.pack_codes(codes, frames_rows=frames, n_q_frames=ret["n_q_frames"])
        rows = ret.get("n_q_rows")
        if rows is None:
            rows = self._bit_widths(bit_width, codes.shape[1])[1]
        return self.engine.pack_codes(codes, frames_rows=frames, n_q_rows=rows)

    def _inference(self, speech, need_recon, bit_width, use_scale, _quantise_always, speech_lengths, target_snr_db=None, min_n_q=1,
                   per_frame=False):
        speech = self._as_bct(speech)
        bypass = self.arch.bypass_quantizer and not _quantise_always
        n_q, rows = self._bit_widths(bit_width, speech.shape[0])
        rate = {}
        if target_snr_db is not None:
            floor = (rate_min_nq_frames if per_frame else rate_min_nq)(self.arch, min_n_q, n_q, rows)
            rate = dict(target_snr_db=target_snr_db, min_n_q=floor, **(dict(per_frame=True) if per_frame else {}))
        wav = speech[:, 0, :] if self.engine.channels == 1 else speech
        if speech_lengths is not None:
            why = ragged_refusal(self.arch)
            if why:
                raise EngineError(why)
            if bypass:     # inference() alone: inference_encoding quantises whatever the flag says, the decode calls never see it
                raise EngineError("Encodec.inference with speech_lengths is not built for model_conf.bypass_quantizer (it would decode the "
                                  "encoder output of every row by its own frames); inference_encoding and the decode calls take lengths")
            r = (self.engine.encode_decode(wav, n_q, use_scale=use_scale, lengths=speech_lengths, n_q_rows=rows, **rate) if need_recon
                 else self.engine.encode(wav, n_q, lengths=speech_lengths, n_q_rows=rows, **rate))
            return dict(recon_speech=r.get("recon"), code_indices=[r["codes"]],
                        code_embeddings=[(r["quantized"], r["scale"] if use_scale else None)], sub_quants=[r["sub_quants"]],
                        **self._rate_outputs(r))
        if self.arch.segment_length is not None:
            wav = wav.to(self.device, torch.float32)
            return self._inference_segmented(wav, n_q, need_recon, use_scale, bypass)
        if bypass:
            r = self._encode_or_bypass(wav, n_q, True)
            recon = None
            if need_recon:             # _decode_frame on the encoder output, trimmed like recon[:, :, :T] (:711)
                T = wav.shape[-1]
                recon = self.engine.decode_emb(r["quantized"], r["scale"] if use_scale else None,
                                               out_len=min(T, self.engine.decoded_samples(r["quantized"].shape[1])))
        elif need_recon:
            r = self.engine.encode_decode(wav, n_q, use_scale=use_scale, n_q_rows=rows, **rate)
            recon = r["recon"]
        else:
            r = self.engine.encode(wav, n_q, n_q_rows=rows, **rate)
            recon = None
        scale = r["scale"] if use_scale else None
        return dict(recon_speech=recon, code_indices=[r["codes"]], code_embeddings=[(r["quantized"], scale)],
                    sub_quants=[r["sub_quants"]], **self._rate_outputs(r))

    @staticmethod
    def _rate_outputs(r):
        """n_q_rows and row_snr_db of an engine call made with a target (device tensors; torch is plumbing here: a gather and a log of B values)"""
        if "n_q_rows" not in r:
            return {}
        E = r["row_errors"]
        if "n_q_frames" in r:                          # per_frame: the achieved error is the sum over the frames at their own counts
            return dict(n_q_rows=r["n_q_rows"], n_q_frames=r["n_q_frames"], n_codes_rows=r["n_codes_rows"],
                        row_snr_db=10.0 * torch.log10(E[:, 0] / r["achieved_errors"]))
        Ek = E.gather(1, r["n_q_rows"].long().unsqueeze(1)).squeeze(1)
        return dict(n_q_rows=r["n_q_rows"], row_snr_db=10.0 * torch.log10(E[:, 0] / Ek))

    # -- Encodec.inference_encoding (codec_basic.py:720-764) ---------------------------------
    @torch.no_grad()
    def inference_encoding(self, speech: torch.Tensor, need_recon: bool = False, bit_width: int = None,
                           use_scale: bool = True, speech_lengths=None, rvq_beam: int = None, target_snr_db=None,
                           min_n_q: int = 1, packed: bool = False, per_frame: bool = False) -> Dict[str, torch.Tensor]:
        # (model_conf.bypass_quantizer does not reach this entry point in the reference: it quantises, :748-750)
        return self.inference(speech, need_recon=need_recon, bit_width=bit_width, use_scale=use_scale, _quantise_always=True,
                              speech_lengths=speech_lengths, rvq_beam=rvq_beam, target_snr_db=target_snr_db, min_n_q=min_n_q, packed=packed,
                              per_frame=per_frame)

    # -- Encodec.inference_decoding (codec_basic.py:766-802) ---------------------------------
    @torch.no_grad()
    def inference_decoding(self, token_idx: torch.Tensor, need_recon: bool = True, bit_width: int = None,
                           use_scale: bool = True, token_lengths=None, n_q_frames=None) -> Dict[str, torch.Tensor]:
        """token_lengths [B] (optional): frames per row; row b is then decoded from its own frames alone, zeros behind frames * hop.
        bit_width: ignored when it is one value, as in the reference (the tokens' last dimension says how many stages there are); a
        sequence / 1-D tensor of B gives row b its own count: its tokens behind that are not read.
        n_q_frames [B, Tf] (optional; ``n_q_frames`` of a ``per_frame`` call as it is): a stage count per frame; a frame's tokens behind
        its count are not read."""
        rows = None
        if not self._one_bit_width(bit_width):
            rows = self._bit_widths(bit_width, token_idx.shape[0])[1]
        recon, emb = self.engine.decode_codes(token_idx, lengths=token_lengths, n_q_rows=rows, n_q_frames=n_q_frames)
        if self.arch.segment_length is not None and need_recon:      # _decode: one frame through the overlap-add (codec_basic.py:396)
            recon = self.engine.overlap_add([recon], self.arch.segment_stride or 1)
        return dict(recon_speech=recon if need_recon else None, code_indices=None,
                    code_embeddings=[(emb, None)], sub_quants=None)

    # -- not in the reference: decoding from the packets of ``inference(..., packed=True)`` ---------------------------------
    @torch.no_grad()
    def inference_decoding_packed(self, packets, need_recon: bool = True, use_scale: bool = True) -> Dict[str, torch.Tensor]:
        """packets: a list of B ``bytes`` (one packet each; every header is validated) or the device buffer uint8 [B, pitch] of a packed
        call -> what ``inference_decoding`` returns for the codes they hold, every row decoded with the stage count its packet carries:
        unpack on the device (fc_codes_unpack), the counts of the headers as per-row stage counts, then the decode call there is.  Rows
        of different frame counts go through ``token_lengths`` where the architecture has length-aware calls; otherwise rows of equal
        length are required.  The dict also holds ``n_q_rows`` and ``token_lengths`` (lists, from the headers).  Packets of mode 1 (a
        count per frame), alone or mixed with mode 0: fc_codes_unpack_frames writes the counts of every frame on the device and the decode
        call takes them from there; the dict then also holds ``n_q_frames`` [B, Tf] int32 (device), and ``n_q_rows`` every row's largest."""
        why = packed_refusal(self.arch)
        if why:
            raise EngineError(why)
        eng = self.engine
        if isinstance(packets, torch.Tensor):
            if packets.dim() != 2 or packets.dtype != torch.uint8:
                raise EngineError(f"inference_decoding_packed: a packet buffer is uint8 [B, pitch], got {packets.dtype} {tuple(packets.shape)}")
            # the host needs the headers (the counts are a host argument of the decode call): 8 bytes per row
            modes, frames, counts, _ = eng._parse_packets_any([bytes(h) for h in packets[:, :8].cpu().numpy()], exact=None)
            buf = packets
        else:
            buf, _, counts = eng.packets_from_host(packets)
            modes, frames = eng._parse_packets_any(packets, exact=True)[:2]
        Tf, n_q = max(frames), max(counts)
        lengths = None
        if any(f != Tf for f in frames):
            why = ragged_refusal(self.arch)
            if why:
                raise EngineError(f"inference_decoding_packed: the packets hold {frames} frames and rows of equal length are required: {why}")
            lengths = frames
        if any(modes):
            tokens, kf = eng.unpack_frame_codes(buf, Tf, n_q)
            recon, emb = eng.decode_codes(tokens, lengths=lengths, n_q_frames=kf)
            return dict(recon_speech=recon if need_recon else None, code_indices=None, code_embeddings=[(emb, None)], sub_quants=None,
                        n_q_rows=counts, token_lengths=frames, n_q_frames=kf)
        tokens = eng.unpack_codes(buf, Tf, n_q)
        rows = counts if any(k != n_q for k in counts) else None
        recon, emb = eng.decode_codes(tokens, lengths=lengths, n_q_rows=rows)
        return dict(recon_speech=recon if need_recon else None, code_indices=None, code_embeddings=[(emb, None)], sub_quants=None,
                    n_q_rows=counts, token_lengths=frames)

    # -- Encodec.inference_decoding_emb (codec_basic.py:804-836) -----------------------------
    @torch.no_grad()
    def inference_decoding_emb(self, token_idx: torch.Tensor, need_recon: bool = True, bit_width: int = None,
                               use_scale: bool = True, token_lengths=None) -> Dict[str, torch.Tensor]:
        if token_lengths is not None and not need_recon:
            self.engine._lengths_in(token_lengths, token_idx.shape[0])      # a refused architecture raises whatever is asked for
        recon = self.engine.decode_emb(token_idx, lengths=token_lengths) if need_recon else None
        if self.arch.segment_length is not None and recon is not None:
            recon = self.engine.overlap_add([recon], self.arch.segment_stride or 1)
        return dict(recon_speech=recon, code_indices=None, code_embeddings=[(token_idx, None)], sub_quants=None)
