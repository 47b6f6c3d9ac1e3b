"""``Speech2Token`` -- same constructor, call signature and 4-tuple as the reference's
funcodec/bin/codec_inference.py:41-150, running on the MI355X engine.

    from funcodec_amd.bin.codec_inference import Speech2Token
    s2t = Speech2Token("config.yaml", "model.pth", device="cuda")
    code_indices, code_embeddings, recon_speech, sub_quants = s2t(wav)        # run_mod="inference"
"""
from __future__ import annotations

import logging
import math
from pathlib import Path
from typing import Any, Optional, Union

import numpy as np
import torch

from ..config import arch_from_config
from ..model import EncodecMI355X


def build_model_from_file(config_file, model_file, device="cuda"):
    """Counterpart of GANSpeechCodecTask.build_model_from_file (funcodec/tasks/abs_task.py:1895-1947):
    yaml -> architecture, torch.load(model.pth) -> tolerant state_dict load."""
    import argparse
    import yaml
    with open(config_file, "rt", encoding="utf-8") as f:
        args = yaml.safe_load(f)
    arch = arch_from_config(args)
    model = EncodecMI355X(arch, device=device)
    if model_file is not None:
        state = torch.load(model_file, map_location="cpu")
        model.load_state_dict(state)
    return model, argparse.Namespace(**args)


class Speech2Token:
    """Speech2Token class (drop-in for funcodec.bin.codec_inference.Speech2Token)."""

    def __init__(
            self,
            config_file: Union[Path, str] = None,
            model_file: Union[Path, str] = None,
            device: str = "cpu",          # the reference's default (codec_inference.py:53-63); this engine then refuses loudly, see below
            batch_size: int = 1,
            dtype: str = "float32",
            streaming: bool = False,
            sampling_rate: int = 24_000,
            bit_width: int = 24_000,
            check_status: bool = True,
            rvq_beam: int = 1,
    ):
        if dtype not in ("float16", "float32", "float64"):
            raise ValueError(f"dtype must be float16, float32 or float64, got {dtype!r}")
        # The engine computes in fp32 whatever `dtype` says (index exactness).  The reference converts the MODEL with
        # model.to(dtype) (:78) and feeds the caller's tensors unchanged; here float16 / float64 means: inputs of that dtype are
        # accepted and the floating-point outputs are returned in it (fp32 arithmetic in between).
        # Same signature and default as the reference -- so `Speech2Token(cfg, pth)` does NOT silently pick a GPU: it fails the same way an
        # explicit device="cpu" does, with the fix in the message.
        if str(device).startswith("cpu"):
            raise RuntimeError("funcodec_amd.Speech2Token runs on MI355X only: pass device='cuda' (or 'cuda:<n>'); the default 'cpu' is the "
                               "reference's signature (funcodec/bin/codec_inference.py:56) -- use the reference itself for CPU inference")
        model, model_args = build_model_from_file(config_file, model_file, device)
        self.model = model
        self.model_args = model_args
        self.device = device
        self.dtype = dtype
        self.already_stat_flops = False
        # device-side failures (an out-of-range code index, which the reference's F.embedding raises on; a persistent-LSTM barrier
        # timeout) are recorded by the kernels and can only be read after the stream has drained: by default every call ends with
        # that check, like the reference raises in line.  check_status=False keeps calls asynchronous (the caller then uses
        # model.engine.check_status() itself).
        self.check_status = check_status
        # not in the reference: the width of the quantiser's search over its stages in the two encoding modes (1: the reference's greedy
        # quantiser); a call's own rvq_beam= goes first.  Refused here, before any call, for a model that cannot take it.
        from ..engine import rvq_beam_width
        self.rvq_beam = rvq_beam_width(model.arch, rvq_beam)
        self.last_n_q_rows = self.last_row_snr_db = None          # of the last call made with target_snr_db
        self.last_packets = None                                  # of the last call made with packed=True
        self.last_n_q_frames = self.last_n_codes_rows = None      # of the last call made with per_frame=True

    @torch.no_grad()
    def __call__(
            self,
            speech: Union[torch.Tensor, np.ndarray],
            ppg: Optional[Union[torch.Tensor, np.ndarray]] = None,
            need_recon: bool = True,
            bit_width: int = None,
            use_scale: bool = True,
            run_mod: str = "inference",
            speech_lengths: Optional[Union[torch.Tensor, np.ndarray]] = None,
            rvq_beam: Optional[int] = None,
            target_snr_db=None,
            min_n_q: int = 1,
            packed: bool = False,
            n_q_rows=None,
            per_frame: bool = False,
            n_q_frames=None,
    ):
        """Returns (code_indices, code_embeddings, recon_speech, sub_quants) like the reference (:86-134).

        speech_lengths [B] (not in the reference; default None = the reference's behaviour): samples per row (frames per row for the
        two decode modes).  With it every row is computed as if it were alone in the batch, cut at its own length, zeros behind
        (EncodecMI355X.inference).

        rvq_beam (not in the reference; default None = the instance's, whose default 1 is the reference's greedy quantiser): 2, 4 or 8
        hypotheses per frame through the quantiser's stages in the modes that encode; the two decode modes do not quantise.

        target_snr_db, min_n_q (not in the reference; default None = off): in the modes that encode, every row takes the fewest stages that
        reach its target SNR in the quantiser's domain (EncodecMI355X.inference).  The 4-tuple stays; the chosen counts of the last such
        call stand in ``last_n_q_rows`` (device int32 [B]) and their SNRs in ``last_row_snr_db``; they are None after any other call.

        packed (not in the reference; default False): in the modes that encode, the call also writes one packet per row (EncodecMI355X.inference,
        csrc/code_pack_kernels.h).  The 4-tuple stays; the packets (device uint8 [B, pitch]) stand in ``last_packets``, None after any other call.

        n_q_rows (not in the reference; run_mod="decode" only): a stage count per row, as the packets of ``codecs.fcb`` carry it; row b's
        tokens behind its count are not read.

        per_frame (not in the reference; with target_snr_db, in the modes that encode): a stage count per FRAME (EncodecMI355X.inference,
        csrc/rvq_rate_kernels.h); min_n_q may then be 0.  The counts of the last such call stand in ``last_n_q_frames``
        (device int32 [B, Tf]) and ``last_n_codes_rows``; ``last_n_q_rows`` holds every row's largest, ``last_packets`` packets of mode 1.

        n_q_frames (not in the reference; run_mod="decode" only): a stage count per frame [B, T], as mode-1 packets carry it."""
        if per_frame and run_mod not in ("inference", "encode"):
            raise ValueError(f"per_frame belongs to the modes that encode (inference, encode), not run_mod={run_mod!r}")
        if per_frame and target_snr_db is None:
            raise ValueError("per_frame chooses a stage count per frame by target_snr_db: give a target")
        if n_q_frames is not None and run_mod != "decode":
            raise ValueError(f"n_q_frames belongs to run_mod='decode', not run_mod={run_mod!r}")
        if packed and run_mod not in ("inference", "encode"):
            raise ValueError(f"packed belongs to the modes that encode (inference, encode), not run_mod={run_mod!r}")
        if n_q_rows is not None and run_mod != "decode":
            raise ValueError(f"n_q_rows belongs to run_mod='decode', not run_mod={run_mod!r}")
        self.last_packets = None
        if target_snr_db is not None and run_mod not in ("inference", "encode"):
            raise ValueError(f"target_snr_db belongs to the modes that encode (inference, encode), not run_mod={run_mod!r}")
        rate = {} if target_snr_db is None else dict(target_snr_db=target_snr_db, min_n_q=min_n_q)
        if per_frame:
            rate["per_frame"] = True
        if packed:
            rate["packed"] = True
        self.last_n_q_rows = self.last_row_snr_db = self.last_n_q_frames = self.last_n_codes_rows = None
        rvq_beam = getattr(self, "rvq_beam", 1) if rvq_beam is None else rvq_beam       # (an instance built around a ready model has none)
        if ppg is not None:
            raise NotImplementedError("ppg conditioning (codec_semantic_aug) is outside the hot-path scope")
        if isinstance(speech, np.ndarray):
            speech = torch.from_numpy(speech)
        speech = speech.to(self.model.device)
        if run_mod == "inference":
            ret = self.model.inference(speech, need_recon=need_recon, bit_width=bit_width, use_scale=use_scale, speech_lengths=speech_lengths,
                                       rvq_beam=rvq_beam, **rate)
        elif run_mod == "encode":
            ret = self.model.inference_encoding(speech, need_recon=False, bit_width=bit_width, speech_lengths=speech_lengths, rvq_beam=rvq_beam,
                                                **rate)
        elif run_mod == "decode_emb":
            ret = self.model.inference_decoding_emb(speech, token_lengths=speech_lengths)
        else:
            q = self.model.quantizer
            bit_per_quant = (q.sampling_rate // q.encoder_hop_length) * int(math.log2(q.codebook_size))
            nq = None
            if bit_width is not None:
                nq = int(max(bit_width // bit_per_quant, 1))
            speech = speech[:, :, :nq]
            logging.info("use %d quantizers.", speech.shape[-1])
            if n_q_frames is not None:       # the counts of mode-1 packets: the device clamps them to the stages kept
                ret = self.model.inference_decoding(speech, token_lengths=speech_lengths, n_q_frames=n_q_frames)
            elif n_q_rows is not None:       # the counts of the rows' packets, no larger than the stages kept
                rows = [min(int(k), speech.shape[-1]) for k in torch.as_tensor(n_q_rows).reshape(-1).tolist()]
                recon, emb = self.model.engine.decode_codes(speech, lengths=speech_lengths,
                                                            n_q_rows=rows if any(k != speech.shape[-1] for k in rows) else None)
                if self.model.arch.segment_length is not None:
                    recon = self.model.engine.overlap_add([recon], self.model.arch.segment_stride or 1)
                ret = dict(recon_speech=recon, code_indices=None, code_embeddings=[(emb, None)], sub_quants=None)
            else:
                ret = self.model.inference_decoding(speech, token_lengths=speech_lengths)
        self.last_packets = ret.get("packets")
        self.last_n_q_rows, self.last_row_snr_db = ret.get("n_q_rows"), ret.get("row_snr_db")
        self.last_n_q_frames, self.last_n_codes_rows = ret.get("n_q_frames"), ret.get("n_codes_rows")
        if self.check_status:
            self.model.engine.check_status(sync=True)
        if self.dtype != "float32":
            td = getattr(torch, self.dtype)
            cast = lambda t: t.to(td) if isinstance(t, torch.Tensor) and t.is_floating_point() else t   # noqa: E731
            ret = dict(ret,
                       code_embeddings=[(cast(q), cast(sc)) for q, sc in ret["code_embeddings"]],
                       recon_speech=cast(ret["recon_speech"]),
                       sub_quants=None if ret["sub_quants"] is None else [cast(x) for x in ret["sub_quants"]])
        return (ret["code_indices"], ret["code_embeddings"], ret["recon_speech"], ret["sub_quants"])

    def open_stream(self, batch: int = 1, n_q: Optional[int] = None, scale=None, max_chunk: Optional[int] = None,
                    max_frames: Optional[int] = None, graph: bool = False, rvq_beam: Optional[int] = None, noise_floor_db=None, min_n_q: int = 1,
                    per_frame: bool = False):
        """A streaming session of the loaded (causal) model: funcodec_amd.stream.CodecStream.  Not in the reference, whose
        `streaming=` keyword selects a data iterator; that keyword keeps its meaning here (accepted, unused).  graph: replay steady
        pushes as captured HIP graphs (results are then copies)."""
        return self.model.open_stream(batch, n_q=n_q, scale=scale, max_chunk=max_chunk, max_frames=max_frames, graph=graph,
                                      rvq_beam=getattr(self, "rvq_beam", 1) if rvq_beam is None else rvq_beam,
                                      noise_floor_db=noise_floor_db, min_n_q=min_n_q, per_frame=per_frame)

    def open_slots(self, slots: int, n_q: Optional[int] = None, max_chunk: Optional[int] = None, max_frames: Optional[int] = None,
                   graph: bool = False, rvq_beam: Optional[int] = None, noise_floor_db=None, min_n_q: int = 1,
                   per_frame: bool = False):
        """A slot session of the loaded (causal) model: funcodec_amd.stream.StreamSlots, independent utterances sharing every push
        (max_frames: the bound a transformer bottleneck needs, as for open_stream; graph: as for open_stream)."""
        return self.model.open_slots(slots, n_q=n_q, max_chunk=max_chunk, max_frames=max_frames, graph=graph,
                                     rvq_beam=getattr(self, "rvq_beam", 1) if rvq_beam is None else rvq_beam,
                                     noise_floor_db=noise_floor_db, min_n_q=min_n_q, per_frame=per_frame)

    @staticmethod
    def from_pretrained(model_tag: Optional[str] = None, **kwargs: Optional[Any]):
        """Like the reference (codec_inference.py:136-150: "model_tag ... Currently, not used"): the instance is built from **kwargs
        (config_file / model_file / device ...).  A non-None tag cannot select a model here either -- there is no hub access -- and that is
        said instead of silently dropped."""
        if model_tag is not None:
            logging.warning("Speech2Token.from_pretrained: model_tag=%r is not used (the reference ignores it as well, codec_inference.py:144); "
                            "the model comes from config_file / model_file", model_tag)
            if not (kwargs.get("config_file") and kwargs.get("model_file")):
                raise ValueError(f"Speech2Token.from_pretrained(model_tag={model_tag!r}) needs config_file= and model_file=: model tags are "
                                 "not resolved (no hub access), the tag alone selects nothing")
        return Speech2Token(**kwargs)


class Token2Speech:
    """Convenience wrapper (the reference has no such class; decoding is Speech2Token(run_mod='decode'))."""

    def __init__(self, config_file=None, model_file=None, device: str = "cuda", speech2token: Speech2Token = None):
        self.s2t = speech2token or Speech2Token(config_file, model_file, device=device)

    @torch.no_grad()
    def __call__(self, tokens: torch.Tensor, bit_width: int = None) -> torch.Tensor:
        """tokens [B,Tf,n_q] int64 -> waveform [B,1,Tf*hop]"""
        return self.s2t(tokens, bit_width=bit_width, run_mod="decode")[2]


# ================================================================================================
# CLI / batch pipeline: same function names, arguments and output files as the reference's
# funcodec/bin/codec_inference.py:164-580 (egs/LibriTTS/codec/encoding_decoding.sh drives exactly this).
# ================================================================================================
def save_audio(wav, path, sample_rate: int, rescale: bool = False):
    from ..io import save_audio as _save
    _save(wav, str(path), sample_rate, rescale)


def inference_modelscope(
        output_dir: Optional[str] = None,
        batch_size: int = 1,
        dtype: str = "float32",
        ngpu: int = 1,
        seed: int = 0,
        num_workers: int = 0,
        log_level: Union[int, str] = "INFO",
        key_file: Optional[str] = None,
        config_file: Optional[str] = "config.yaml",
        model_file: Optional[str] = "model.pth",
        model_tag: Optional[str] = None,
        allow_variable_data_keys: bool = True,
        streaming: bool = False,
        sampling_rate: int = 16_000,
        bit_width: int = 8_000,
        param_dict: Optional[dict] = None,
        use_scale: Optional[bool] = True,
        **kwargs,
):
    """Returns ``_forward(data_path_and_name_and_type | raw_inputs, output_dir_v2, param_dict)`` (reference :164-382)."""
    import os
    from .. import io as fio
    if param_dict is not None:
        kwargs.update(param_dict)
    if ngpu > 1:
        raise NotImplementedError("only single GPU decoding is supported")       # reference :190-191
    if ngpu < 1:
        raise RuntimeError("funcodec_amd runs on MI355X only (ngpu must be >= 1); use the reference for CPU decoding")
    logging.basicConfig(level=log_level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    torch.manual_seed(seed)
    my_model = Speech2Token.from_pretrained(model_tag=model_tag, config_file=config_file, model_file=model_file,
                                            device="cuda", dtype=dtype, streaming=streaming,
                                            sampling_rate=sampling_rate, bit_width=bit_width,
                                            rvq_beam=int(kwargs.get("rvq_beam") or 1),
                                            check_status=False)      # ONE status check per batch, below (not one per call + one per batch)

    def _forward(data_path_and_name_and_type=None, raw_inputs=None, output_dir_v2: Optional[str] = None,
                 param_dict: Optional[dict] = None):
        if param_dict is not None:
            kwargs.update(param_dict)
        if data_path_and_name_and_type is None and raw_inputs is not None:
            uttid = "utt"
            if isinstance(raw_inputs, str):
                uttid = os.path.basename(raw_inputs).rsplit(".")[0]
                raw_inputs, sr = fio.read_wav(raw_inputs)
                if sr != sampling_rate:                                        # librosa.load(sr=...) in the reference (:240)
                    raw_inputs = fio.resample(torch.from_numpy(raw_inputs), sr, sampling_rate).numpy()
            if isinstance(raw_inputs, torch.Tensor):
                raw_inputs = raw_inputs.numpy()
            loader = [([uttid], dict(speech=torch.from_numpy(np.asarray(raw_inputs))[None, :],
                                     speech_lengths=torch.tensor([raw_inputs.shape[0]], dtype=torch.int64)))]
        else:
            loader = fio.iter_batches(data_path_and_name_and_type, batch_size, key_file)
        output_path = output_dir_v2 if output_dir_v2 is not None else output_dir
        if output_path is not None:
            os.makedirs(output_path, exist_ok=True)
        file_sr = kwargs.get("file_sampling_rate")
        should_resample = file_sr not in (None, sampling_rate)               # reference :270-273
        indices_writer, sub_quants_writer, n_q_writer = None, None, None
        target_snr_db = kwargs.get("target_snr_db")
        if target_snr_db is not None and output_path is not None:
            # next to the indices: `key k snr_db` per utterance.  The indices files keep their shape with zeros behind k; a decoder needs k
            # (a bit_width per row), since code 0 is a valid code
            n_q_writer = open(os.path.join(output_path, "codec_n_q.txt"), "wt")
        per_frame = _str2bool(kwargs.get("per_frame", False))
        min_n_q_arg = int(kwargs.get("min_n_q") or 1)                        # --min_n_q 0 is a floor of frame mode alone
        if per_frame and kwargs.get("min_n_q") is not None:
            min_n_q_arg = int(kwargs.get("min_n_q"))
        if per_frame and target_snr_db is None:
            raise ValueError("--per_frame chooses a stage count per frame by --target_snr_db: give a target")
        if per_frame and kwargs.get("need_indices") and kwargs.get("indices_save_type") != "packed":
            raise ValueError("--per_frame with --need_indices requires --indices_save_type packed: the text and ark forms have no place for "
                             f"the counts of the frames, got --indices_save_type {kwargs.get('indices_save_type')}")
        ark_indices = kwargs.get("indices_save_type") == "ark"
        packed_indices = bool(kwargs.get("need_indices")) and kwargs.get("indices_save_type") == "packed"
        run_mod = kwargs.get("run_mod", "inference")
        fcb_writer = None
        if packed_indices:
            # codecs.fcb + codecs.fcb.scp in place of codecs.txt: one packet per utterance with its own frames and stage count
            # (csrc/code_pack_kernels.h; funcodec_amd.io.FcbWriter)
            if run_mod not in ("inference", "encode"):
                raise ValueError(f"--indices_save_type packed belongs to the modes that encode, not --run_mod {run_mod}")
            from ..engine import EngineError, packed_refusal
            why = packed_refusal(my_model.model.arch)
            if why:
                raise EngineError(why)
            bw0 = param_dict["bit_width"] if param_dict is not None and "bit_width" in param_dict else bit_width
            fcb_writer = fio.FcbWriter(os.path.join(output_path, "codecs.fcb"), my_model.model.engine.code_bits,
                                       my_model.model.arch.num_quantizers_for_bandwidth(bw0), sampling_rate,
                                       my_model.model.quantizer.encoder_hop_length)
        elif kwargs.get("need_indices"):
            if ark_indices:
                indices_writer = fio.KaldiMatrixWriter(os.path.join(output_path, "indices"))
            else:
                indices_writer = open(os.path.join(output_path, "codecs.txt"), "wt")
        if kwargs.get("need_sub_quants"):
            sub_quants_writer = fio.KaldiMatrixWriter(os.path.join(output_path, "codec_emb"))

        result_list = []
        hop = my_model.model.quantizer.encoder_hop_length

        # Host pipeline around the engine (the engine does 160 audio-seconds in 17 ms; reading / padding the next batch and writing
        # the previous one must not sit on its critical path): a loader thread keeps up to 3 batches ready, each finished batch is
        # copied to the host ONCE per output and handed to a small writer pool (wav files: the library's C writer, GIL released);
        # codecs.txt lines and ark entries are appended by this thread in batch order.
        import queue
        import threading
        from concurrent.futures import ThreadPoolExecutor

        def _prefetch(it, depth=3):
            q: "queue.Queue" = queue.Queue(maxsize=depth)
            end = object()

            def run():
                try:
                    for item in it:
                        q.put(item)
                    q.put(end)
                except BaseException as ex:          # noqa: BLE001 -- re-raised in the consumer
                    q.put(ex)

            threading.Thread(target=run, daemon=True).start()
            while True:
                item = q.get()
                if item is end:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item

        def _write_batch(keys, speech_length, recon_host, tok_host):
            """wav files of one batch + its codecs.txt lines (returned, written in order by the caller)."""
            lines, results = [], []
            for i, key in enumerate(keys):
                if run_mod in ["decode", "decode_emb"]:
                    codec_len = int(speech_length[i])
                    ilen = codec_len * hop
                else:
                    ilen = int(speech_length[i])
                    codec_len = int(math.ceil(ilen / hop))
                recon_wav = recon_host[i][:, :ilen] if recon_host is not None else None
                if output_path is None:
                    results.append({"key": key, "value": recon_wav})
                    continue
                if recon_wav is not None:
                    save_audio(recon_wav, os.path.join(output_path, key + ".wav" if not key.endswith(".wav") else key),
                               rescale=True, sample_rate=file_sr if should_resample else sampling_rate)
                if tok_host is not None and indices_writer is not None and not ark_indices:
                    lines.append(fio.format_codec_line(key, tok_host, i, codec_len))
            return lines, results

        def _drain(job):
            keys, speech_length, tok_host, sq_host, fut, nq_host, packets_host = job
            lines, results = fut.result()
            result_list.extend(results)
            if packets_host is not None:
                for key, packet, n in zip(keys, packets_host, speech_length):
                    fcb_writer(key, packet, int(n))
            if nq_host is not None and n_q_writer is not None:
                if len(nq_host) == 3:      # --per_frame: `key k_max snr_db mean_k` (mean_k over the utterance's own frames)
                    n_q_writer.write("".join(f"{key} {int(k)} {float(snr):.4f} {float(mk):.4f}\n" for key, k, snr, mk in zip(keys, *nq_host)))
                else:
                    n_q_writer.write("".join(f"{key} {int(k)} {float(snr):.4f}\n" for key, k, snr in zip(keys, *nq_host)))
            if lines:
                indices_writer.write("".join(lines))
            for i, key in enumerate(keys):               # Kaldi ark writers keep file offsets: sequential, in order
                codec_len = int(speech_length[i]) if run_mod in ["decode", "decode_emb"] else int(math.ceil(int(speech_length[i]) / hop))
                if tok_host is not None and indices_writer is not None and ark_indices and output_path is not None:   # [T, n_q] (reference :292-294)
                    mats = [x[:, i, :codec_len].float().numpy().T for x in tok_host]
                    indices_writer(key, np.concatenate(mats, axis=0))
                if sq_host is not None and sub_quants_writer is not None and output_path is not None:                # [T, n_q*D] (reference :301-311)
                    sq = torch.cat(sq_host, dim=-1).permute(1, 3, 0, 2)[i][:codec_len]
                    sub_quants_writer(key, sq.reshape(sq.shape[0], -1).numpy())

        if kwargs.get("stat_flops") and not my_model.already_stat_flops:     # reference :328-342 (thop profile of a 1 s random input)
            eng = my_model.model.engine
            nq = my_model.model.arch.num_quantizers_for_bandwidth(bit_width)
            w = eng.work(1, int(sampling_rate), nq)
            params = sum(int(np.prod(shape)) for shape in eng.expected_tensors().values())
            logging.info(f"Model total MACs: {w['total_flops'] / 2e9:.2f} G (conv {w['conv_flops'] / 2e9:.2f}, lstm {w['lstm_flops'] / 2e9:.2f}, "
                         f"rvq {w['rvq_flops'] / 2e9:.2f}; 1 s of audio, n_q = {nq}), params: {params / 1e6:.2f} M")
            my_model.already_stat_flops = True
        pool = ThreadPoolExecutor(max_workers=4)
        jobs = []
        try:
            for keys, batch in _prefetch(loader):
                if should_resample:                                                 # reference :318-322 (lengths stay in file samples)
                    batch["speech"] = fio.resample(batch["speech"], file_sr, sampling_rate)
                speech_length = batch.pop("speech_lengths")
                if "speech_n_q" in batch:                               # a codec_fcb input: every row decodes with the count its packet carries
                    batch["n_q_rows"] = batch.pop("speech_n_q")
                if "speech_n_q_frames" in batch:                        # mode-1 packets in the batch: a count per frame (a mode-0 row: its k in every frame)
                    batch["n_q_frames"] = batch.pop("speech_n_q_frames")
                    batch.pop("n_q_rows", None)
                if _str2bool(kwargs.get("length_aware", False)):        # opt-in: the lengths go to the model instead of being dropped
                    if should_resample:
                        raise NotImplementedError("length_aware with file_sampling_rate != sampling_rate (the lengths count file samples)")
                    batch["speech_lengths"] = speech_length
                bw = param_dict["bit_width"] if param_dict is not None and "bit_width" in param_dict else bit_width
                token_id, token_emb, recon_speech, sub_quants = my_model(**batch, need_recon=True, bit_width=bw,
                                                                         use_scale=use_scale, run_mod=run_mod,
                                                                         **({} if target_snr_db is None else dict(
                                                                             target_snr_db=float(target_snr_db), per_frame=per_frame,
                                                                             min_n_q=min_n_q_arg)))
                # device-side failures cannot raise in-line like the reference's F.embedding / asserts do: synchronise and ask the
                # engine before anything of this batch is written (corrupt token files, LSTM barrier timeout)
                my_model.model.engine.check_status(sync=True)
                if should_resample and recon_speech is not None:                    # reference :352-356
                    recon_speech = fio.resample(recon_speech, sampling_rate, file_sr)
                recon_host = recon_speech.cpu() if recon_speech is not None else None
                tok_host = [x.cpu().contiguous() for x in token_id] if (token_id is not None and indices_writer is not None) else None
                sq_host = [x.cpu() for x in sub_quants] if (sub_quants is not None and sub_quants_writer is not None) else None
                nq_host = None if target_snr_db is None else (my_model.last_n_q_rows.tolist(), my_model.last_row_snr_db.tolist())
                if per_frame:
                    fr = [max(int(math.ceil(int(n) / hop)), 1) for n in speech_length]
                    nq_host = ([max(k, 1) for k in nq_host[0]], nq_host[1], [c / f for c, f in zip(my_model.last_n_codes_rows.tolist(), fr)])
                packets_host = None
                if fcb_writer is not None:
                    # the frames the text form writes for a row (ceil(samples / hop)); the counts of a target go from the device tensor into the packer
                    eng = my_model.model.engine
                    frames = [int(math.ceil(int(n) / hop)) for n in speech_length]
                    packets_host = eng.packets_to_host(eng.pack_codes(token_id[0], frames_rows=frames, n_q_rows=my_model.last_n_q_rows,
                                                                      n_q_frames=my_model.last_n_q_frames))
                jobs.append((keys, speech_length, tok_host, sq_host, pool.submit(_write_batch, keys, speech_length, recon_host, tok_host), nq_host,
                             packets_host))
                while len(jobs) > 3:                                                # bounds the host memory held by queued batches
                    _drain(jobs.pop(0))
            while jobs:
                _drain(jobs.pop(0))
        finally:
            pool.shutdown(wait=True)
        for w in (indices_writer, sub_quants_writer, n_q_writer, fcb_writer):
            if w is not None:
                w.close()
        return result_list

    return _forward


def inference(output_dir, batch_size, dtype, ngpu, seed, num_workers, log_level, data_path_and_name_and_type, key_file,
              config_file, model_file, model_tag, allow_variable_data_keys=True, streaming=False, sampling_rate=24_000,
              bit_width=24_000, use_scale=True, **kwargs):
    pipeline = inference_modelscope(output_dir=output_dir, batch_size=batch_size, dtype=dtype, ngpu=ngpu, seed=seed,
                                    num_workers=num_workers, log_level=log_level, key_file=key_file, config_file=config_file,
                                    model_file=model_file, model_tag=model_tag,
                                    allow_variable_data_keys=allow_variable_data_keys, streaming=streaming,
                                    sampling_rate=sampling_rate, bit_width=bit_width, use_scale=use_scale, **kwargs)
    return pipeline(data_path_and_name_and_type, raw_inputs=None)


def _str2bool(v: str) -> bool:
    return str(v).lower() in ("true", "1", "yes", "y", "t")


def _str2triple(v: str):
    a, b, c = v.split(",")
    return a.strip(), b.strip(), c.strip()


def get_parser():
    """Same flags (names, types, defaults) as the reference parser (:428-558)."""
    import argparse
    p = argparse.ArgumentParser(description="Speech Tokenizer", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--log_level", type=lambda x: x.upper(), default="INFO",
                   choices=("CRITICAL", "ERROR", "WARNING", "INFO", "DEBUG", "NOTSET"))
    p.add_argument("--output_dir", type=str, required=False)
    p.add_argument("--ngpu", type=int, default=0)
    p.add_argument("--gpuid_list", type=str, default="")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--dtype", default="float32", choices=["float16", "float32", "float64"])
    p.add_argument("--num_workers", type=int, default=0)
    g = p.add_argument_group("Input data related")
    g.add_argument("--data_path_and_name_and_type", type=_str2triple, required=False, action="append")
    g.add_argument("--key_file", type=lambda s: None if s in ("none", "None", "null", "") else s)
    g.add_argument("--allow_variable_data_keys", type=_str2bool, default=False)
    g = p.add_argument_group("The model configuration related")
    g.add_argument("--config_file", type=str)
    g.add_argument("--model_file", type=str)
    g.add_argument("--model_tag", type=str)
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--sampling_rate", type=int, default=24_000)
    p.add_argument("--file_sampling_rate", type=int, default=None)
    p.add_argument("--bit_width", type=int, default=16_000)
    p.add_argument("--use_scale", type=_str2bool, default=True)
    g.add_argument("--need_indices", type=_str2bool)
    # text: codecs.txt; ark: a Kaldi float matrix; packed (not in the reference): codecs.fcb + codecs.fcb.scp, the codec's own bit stream --
    # one packet per utterance with its frames and stage count; --run_mod decode reads it back as input type codec_fcb
    g.add_argument("--indices_save_type", type=str, default="text")
    g.add_argument("--need_sub_quants", type=_str2bool)
    g.add_argument("--run_mod", type=str, choices=["inference", "encode", "decode", "decode_emb"], default="inference")
    g.add_argument("--stat_flops", type=_str2bool, default=False)
    # not in the reference: every utterance of a batch is coded as if it were alone (its own volume scale, normalisation statistics and
    # end padding), so that --batch_size N writes what --batch_size 1 writes
    g.add_argument("--length_aware", type=_str2bool, default=False)
    # not in the reference: hypotheses per frame through the quantiser's stages (1: the reference's greedy quantiser); same files, no frame
    # coded worse
    g.add_argument("--rvq_beam", type=int, choices=[1, 2, 4, 8], default=1)
    # not in the reference: every utterance takes the fewest quantiser stages (at least --min_n_q, at most those of --bit_width) that reach
    # this SNR in the quantiser's domain; codec_n_q.txt (`key k snr_db`) is written next to the indices, which keep their shape
    g.add_argument("--target_snr_db", type=float, default=None)
    g.add_argument("--min_n_q", type=int, default=1)
    # not in the reference: with --target_snr_db, a stage count per FRAME (every frame is coded down to the utterance's noise floor; a frame
    # may take no stage with --min_n_q 0).  With --need_indices it requires --indices_save_type packed (mode-1
    # packets carry the counts); codec_n_q.txt lines become `key k_max snr_db mean_k`
    g.add_argument("--per_frame", type=_str2bool, default=False)
    return p


def main(cmd=None):
    """One process per GPU; the job index and the GPU come from the suffix of --output_dir (``output.JOB``) and
    --gpuid_list exactly as in the reference (:561-580); on ROCm the mask is HIP_VISIBLE_DEVICES and the process then
    uses device 0 (the reference's set_device(int(gpuid)) after masking is only correct for gpuid 0)."""
    import os
    import sys
    print(" ".join(sys.argv), file=sys.stderr)
    args = get_parser().parse_args(cmd)
    if args.file_sampling_rate is None:
        args.file_sampling_rate = args.sampling_rate
    kwargs = vars(args)
    gpus = [g for g in args.gpuid_list.split(",") if g != ""]
    if gpus:
        jobid = 1 if args.output_dir is None else int(args.output_dir.split(".")[-1])
        os.environ["HIP_VISIBLE_DEVICES"] = gpus[(jobid - 1) % len(gpus)]
    kwargs.pop("gpuid_list", None)
    kwargs.pop("stat_flops", None)
    inference(**kwargs)


if __name__ == "__main__":
    main()
