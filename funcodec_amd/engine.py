"""Host side of the MI355X engine: owns the engine handle, checkpoint ingestion and the device
workspace.  PyTorch is used only for device memory, streams and checkpoint I/O; every arithmetic
operation of the hot path happens inside libfuncodec_amd.so (HIP, gfx950).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import logging
import numbers
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .config import SEQ_FF, SEQ_HEADS, ArchSpec


class EngineError(RuntimeError):
    pass


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _on_device(fn):
    """Run a method with the engine's GPU as the thread's current device (kernels are launched on that device's stream;
    a caller whose current device is another GPU must not have to know)."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *a, **kw):
        if not torch.cuda.is_available():          # GPU-less box: let the call reach the library's own loud error
            return fn(self, *a, **kw)
        with torch.cuda.device(self.device):
            return fn(self, *a, **kw)
    return wrapper


def ragged_refusal(arch) -> Optional[str]:
    """Why a model of this architecture has no length-aware (``speech_lengths`` / ``token_lengths``) calls, or None.  The
    configuration key is named, as ``stream_refusal`` does."""
    if arch.model_type != "encodec":
        return "length-aware batches are not available for model: freq_codec (time-domain codec only)"
    if arch.lstm_layers > 0 and arch.seq_model == "transformer":
        return "length-aware batches are not available for seq_model: transformer (it needs a key mask per row)"
    if arch.q0_ds_ratio > 1:
        return "length-aware batches are not available for quantizer_conf.q0_ds_ratio > 1 (the half-rate first stage is laid out per batch width)"
    if arch.segment_length is not None:
        return "length-aware batches are not available with model_conf.segment_dur (segments are a host loop over whole utterances)"
    return None


def row_nq_refusal(arch) -> Optional[str]:
    """Why a model of this architecture takes no per-row stage counts (a ``bit_width`` / ``n_q`` per row), or None.  The configuration
    key is named, as ``ragged_refusal`` does."""
    if arch.segment_length is not None:
        return "a bit rate per row is not available with model_conf.segment_dur (segments are extra batch rows of the engine call)"
    if arch.bypass_quantizer:
        return "a bit rate per row is not available with model_conf.bypass_quantizer (the quantiser's result is dropped)"
    return None


def packed_refusal(arch) -> Optional[str]:
    """Why a model of this architecture writes no packets (``packed=True``; csrc/code_pack_kernels.h states the packet), or None.  The
    configuration key is named, as ``ragged_refusal`` does."""
    if arch.segment_length is not None:
        return "packets are not available with model_conf.segment_dur (a segment's codes are a list of frames, not one row per utterance)"
    if arch.bypass_quantizer:
        return "packets are not available with model_conf.bypass_quantizer (the quantiser's result is dropped)"
    if arch.q0_ds_ratio > 1:
        return "packets are not available for quantizer_conf.q0_ds_ratio > 1 (stage 0 runs at half the frame rate; its packet form is not built)"
    return None


RVQ_BEAM_WIDTHS = (1, 2, 4, 8)


def rvq_beam_refusal(arch) -> Optional[str]:
    """Why a model of this architecture takes no search over the quantiser's stages (``rvq_beam`` above 1), or None.  The configuration
    key is named, as ``ragged_refusal`` does."""
    if arch.bypass_quantizer:
        return "rvq_beam is not available with model_conf.bypass_quantizer (the quantiser's result is dropped)"
    if arch.q0_ds_ratio > 1:
        return ("rvq_beam is not available for quantizer_conf.q0_ds_ratio > 1 (stage 0 is shared by frame pairs, so the frames are "
                "not independent)")
    return None


def rvq_beam_width(arch, width) -> int:
    """A checked ``rvq_beam``: None and 1 are the greedy quantiser; raises before any engine call."""
    if width is None:
        return 1
    if isinstance(width, bool) or not isinstance(width, numbers.Integral) or int(width) not in RVQ_BEAM_WIDTHS:
        raise EngineError(f"rvq_beam: a width is one of {', '.join(map(str, RVQ_BEAM_WIDTHS))}, got {width!r}")
    if int(width) > 1:
        why = rvq_beam_refusal(arch)
        if why:
            raise EngineError(why)
    return int(width)


def rate_refusal(arch) -> Optional[str]:
    """Why a model of this architecture takes no stage count per row by target SNR (``target_snr_db``), or None.  The configuration key
    is named, as ``ragged_refusal`` does."""
    if arch.segment_length is not None:
        return "target_snr_db is not available with model_conf.segment_dur (segments are extra batch rows of the engine call)"
    if arch.bypass_quantizer:
        return "target_snr_db is not available with model_conf.bypass_quantizer (the quantiser's result is dropped)"
    if arch.q0_ds_ratio > 1:
        return ("target_snr_db is not available for quantizer_conf.q0_ds_ratio > 1 (stage 0 quantises another frame's row, so a frame's "
                "residual is not its input minus its codes)")
    return None


def rate_targets(arch, target, B: int) -> list:
    """The ratios rho_b = 10^(-target_b / 10) of a ``target_snr_db`` that is one value or B of them, as B Python floats (float64: the
    device multiplies the same doubles); raises before any engine call.  +inf is "the best k" (rho = 0), -inf is "the floor"."""
    why = rate_refusal(arch)
    if why:
        raise EngineError(why)
    if isinstance(target, numbers.Real) or (hasattr(target, "ndim") and target.ndim == 0):
        target = [float(target)] * B
    elif hasattr(target, "ndim"):
        if target.ndim != 1:
            raise EngineError(f"target_snr_db must be one value or a sequence / 1-D tensor of one per row, got shape {tuple(target.shape)}")
        target = target.tolist()
    target = list(target)
    if len(target) != B:
        raise EngineError(f"target_snr_db must hold one entry per row ({B}), got {len(target)}")
    out = []
    for b, v in enumerate(target):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or v != v:
            raise EngineError(f"row {b}: target_snr_db is a number of dB (not NaN), got {v!r}")
        v = float(v)
        out.append(0.0 if v == float("inf") else float("inf") if v == float("-inf") else float(np.float64(10.0) ** np.float64(-v / 10.0)))
    return out


def rate_min_nq(arch, min_n_q, cap: Optional[int] = None, rows=None, floor: int = 1) -> int:
    """A checked ``min_n_q``: an integer in [floor, cap] (cap: ``num_quantizers`` unless given) and no larger than any per-row cap.
    floor: 1 for the row rule; 0 for frame mode (``per_frame=True``), where a frame may take no stage at all."""
    cap = arch.num_quantizers if cap is None else int(cap)
    if isinstance(min_n_q, bool) or not isinstance(min_n_q, numbers.Integral) or not floor <= int(min_n_q) <= cap:
        raise EngineError(f"min_n_q lies in [{floor}, {cap}]{'' if floor else ' with per_frame'}, got {min_n_q!r}")
    if rows is not None:
        for b, k in enumerate(rows):
            if int(min_n_q) > k:
                raise EngineError(f"min_n_q = {int(min_n_q)} lies above the cap of row {b} ({k} stages)")
    return int(min_n_q)


def rate_min_nq_frames(arch, min_n_q, cap: Optional[int] = None, rows=None) -> int:
    """A checked ``min_n_q`` of frame mode (``per_frame=True``): an integer in [0, cap] (cap: ``num_quantizers`` unless given) and no
    larger than any per-row cap -- a frame may take no stage at all."""
    return rate_min_nq(arch, min_n_q, cap, rows, floor=0)


def _pick_scan(e, lo: int, cap: int, meets) -> int:
    """The scan of both picks: the smallest k in [lo, cap] with meets(e[k]); no such k: the k in that range with the smallest e[k], first
    on ties."""
    best = lo
    for k in range(lo, cap + 1):
        if meets(e[k]):
            return k
        if e[k] < e[best]:
            best = k
    return best


def rate_pick(E, ratio: float, min_n_q: int, cap: int) -> int:
    """The stage count of one row (csrc/rvq_rate_kernels.h, include/funcodec_amd.h), a pure function of its float64 row errors
    E[0 .. cap] (E[0]: the input energy), its ratio 10^(-target / 10), the floor and the cap:
      - energies that are not all finite: cap (what the plain call gives the row);
      - E[0] == 0 (digital silence): min_n_q;
      - the smallest k in [min_n_q, cap] with E[k] <= E[0] * ratio;
      - no such k: the k in that range with the smallest E[k], first on ties."""
    E = [float(v) for v in E[:cap + 1]]
    lo = min(max(int(min_n_q), 1), cap)
    if not all(np.isfinite(v) for v in E):
        return cap
    if E[0] == 0.0:
        return lo
    thr = float(np.float64(E[0]) * np.float64(ratio))
    return _pick_scan(E, lo, cap, lambda v: v <= thr)


def floor_refusal(arch) -> Optional[str]:
    """Why a model of this architecture takes no stage count per push by a noise floor (``noise_floor_db``), or None.  The configuration
    key is named, as ``rate_refusal`` does."""
    if arch.segment_length is not None:
        return "noise_floor_db is not available with model_conf.segment_dur (segments are extra batch rows of the engine call)"
    if arch.bypass_quantizer:
        return "noise_floor_db is not available with model_conf.bypass_quantizer (the quantiser's result is dropped)"
    if arch.q0_ds_ratio > 1:
        return ("noise_floor_db is not available for quantizer_conf.q0_ds_ratio > 1 (stage 0 quantises another frame's row, so a frame's "
                "residual is not its input minus its codes)")
    return None


def floor_value(arch, db, what: str = "noise_floor_db") -> float:
    """floor = D * 10^(db / 10) of one ``noise_floor_db`` (D: the quantiser's input width; the floor reads as mean-square residual per
    element, in dB re 1), as a Python float (float64: the device multiplies the same double); -inf is 0 ("the best k"), +inf is +inf
    ("always min_n_q"); NaN, or anything that is not a number, raises."""
    if isinstance(db, bool) or not isinstance(db, numbers.Real) or db != db:
        raise EngineError(f"{what} is a number of dB (not NaN), got {db!r}")
    db = float(db)
    if db == float("-inf"):
        return 0.0
    if db == float("inf"):
        return float("inf")
    return float(np.float64(arch.codebook_dim) * np.float64(10.0) ** np.float64(db / 10.0))


def floor_values(arch, db, B: int) -> list:
    """The floors of a ``noise_floor_db`` that is one value or B of them, as B Python floats; raises before any engine call."""
    why = floor_refusal(arch)
    if why:
        raise EngineError(why)
    if isinstance(db, numbers.Real) or (hasattr(db, "ndim") and db.ndim == 0):
        db = [float(db)] * B
    elif hasattr(db, "ndim"):
        if db.ndim != 1:
            raise EngineError(f"noise_floor_db must be one value or a sequence / 1-D tensor of one per row, got shape {tuple(db.shape)}")
        db = db.tolist()
    db = list(db)
    if len(db) != B:
        raise EngineError(f"noise_floor_db must hold one entry per row ({B}), got {len(db)}")
    return [floor_value(arch, v, f"row {b}: noise_floor_db") for b, v in enumerate(db)]


def floor_pick(row_err, frames, floor, min_n_q: int, caps):
    """The push rule (csrc/rvq_rate_kernels.h, include/funcodec_amd.h) in float64 numpy: the stage counts of the B rows of one push, a pure
    function of their float64 row errors row_err [B, n_q + 1] (row_err[b, 0]: the input energy of the row's frames of the push), the frames
    every row has in the push (one int or B), the floors D * 10^(noise_floor_db / 10) (one float or B), min_n_q and the caps (one int or B):
      - a row without frames: -1 (the device leaves its entry alone);
      - energies E[0 .. cap] that are not all finite: cap;
      - E[0] <= thr = floor * float64(frames): min_n_q (the input is already at or below the floor);
      - the smallest k in [min_n_q, cap] with E[k] <= thr;
      - no such k: the k in that range with the smallest E[k], first on ties.
    Returns int32 [B]."""
    row_err = np.asarray(row_err, dtype=np.float64)
    if row_err.ndim == 1:
        row_err = row_err[None]
    B = row_err.shape[0]
    each = lambda v: list(np.broadcast_to(np.asarray(v), (B,)))
    out = np.full((B,), -1, dtype=np.int32)
    for b, (F, fl, cap) in enumerate(zip(each(frames), each(floor), each(caps))):
        F, cap = int(F), int(cap)
        if F <= 0:
            continue
        if fl is None or fl < 0:        # a row switched off keeps its cap
            out[b] = cap
            continue
        E = [float(v) for v in row_err[b, :cap + 1]]
        lo = min(max(int(min_n_q), 1), cap)
        if not all(np.isfinite(v) for v in E):
            out[b] = cap
            continue
        thr = float(np.float64(fl) * np.float64(F))
        out[b] = lo if E[0] <= thr else _pick_scan(E, lo, cap, lambda v: v <= thr)
    return out


def floor_pick_frames(stage_err, frames, floor, min_n_q: int, caps):
    """The push frame rule (csrc/rvq_rate_kernels.h, include/funcodec_amd.h) in float64 numpy: a stage count per frame of one push, a pure
    function of the float32 stage errors stage_err [n_q + 1, B, F] (stage_err[k, b, t]: frame t's residual energy after k stages), the
    frames every row has in the push (one int or B), the floors D * 10^(noise_floor_db / 10) (one float or B; None or negative: the row is
    switched off), min_n_q (0 allowed) and the caps (one int or B).  Row b, frame t < frames_b:
      - a row switched off: cap;
      - errors e[0 .. cap] that are not all finite: cap;
      - float64(e[0]) <= floor: lo = min_n_q clamped to [0, cap];
      - the smallest k in [lo, cap] with float64(e[k]) <= floor -- comparisons only;
      - no such k: the k in that range with the smallest e[k], first on ties.
    Frames t >= frames_b take 0; a row without frames: -1 in every frame (the device leaves its row alone).  Returns int32 [B, F]."""
    err = np.asarray(stage_err, dtype=np.float32)
    if err.ndim == 2:
        err = err[:, None]
    _, B, F = err.shape
    each = lambda v: list(np.broadcast_to(np.asarray(v, dtype=object), (B,)))
    out = np.zeros((B, F), dtype=np.int32)
    for b, (Fb, fl, cap) in enumerate(zip(each(frames), each(floor), each(caps))):
        Fb, cap = int(Fb), int(cap)
        if Fb <= 0:
            out[b] = -1
            continue
        lo = min(max(int(min_n_q), 0), cap)
        for t in range(min(Fb, F)):
            if fl is None or fl < 0:
                out[b, t] = cap
                continue
            e = [float(np.float64(v)) for v in err[:cap + 1, b, t]]
            if not all(np.isfinite(v) for v in e):
                out[b, t] = cap
            elif e[0] <= float(fl):
                out[b, t] = lo
            else:
                out[b, t] = _pick_scan(e, lo, cap, lambda v: v <= float(fl))
    return out


def rate_pick_frames(err, E, ratio: float, min_n_q: int, cap: int, frames: Optional[int] = None):
    """The stage counts of one row's frames (csrc/rvq_rate_kernels.h, include/funcodec_amd.h), a pure function of its float32
    stage errors err[0 .. cap][t] (err[k][t]: frame t's residual energy after k stages), its float64 row errors E[0 .. cap], its ratio
    10^(-target / 10), the floor in [0, cap], the cap and its own frame count (default: all of err's):
      - row energies that are not all finite: every frame takes cap;
      - E[0] == 0 (digital silence): every frame takes the floor;
      - else frame t takes the smallest k in [floor, cap] with float64(err[k][t]) * float64(frames) <= E[0] * ratio;
      - no such k: the k in that range with the smallest err[k][t], first on ties;
      - frames behind the row's frames take 0.
    Returns int32 [Tf] (Tf = err.shape[1])."""
    err = np.asarray(err, dtype=np.float32)
    Tf = err.shape[1]
    F = Tf if frames is None else min(int(frames), Tf)
    out = np.zeros((Tf,), dtype=np.int32)
    Ev = [float(v) for v in np.asarray(E, dtype=np.float64)[:cap + 1]]
    lo = min(max(int(min_n_q), 0), cap)
    if not all(np.isfinite(v) for v in Ev):
        out[:F] = cap
        return out
    if Ev[0] == 0.0:
        out[:F] = lo
        return out
    thr = np.float64(Ev[0]) * np.float64(ratio)
    for t in range(F):
        out[t] = _pick_scan(err[:, t], lo, cap, lambda v: np.float64(v) * np.float64(F) <= thr)
    return out


def row_nq_list(arch, rows, B: int, cap: Optional[int] = None) -> list:
    """The per-row stage counts of a call as a list of B ints in [1, cap] (cap: ``num_quantizers`` unless given); raises before any
    engine call -- a bad count or a list of the wrong length refuses the call as a whole."""
    why = row_nq_refusal(arch)
    if why:
        raise EngineError(why)
    cap = arch.num_quantizers if cap is None else int(cap)
    if hasattr(rows, "ndim"):                          # a tensor or an array
        if rows.ndim != 1:
            raise EngineError(f"per-row stage counts must be a sequence or 1-D tensor, got shape {tuple(rows.shape)}")
        rows = rows.tolist()
    rows = list(rows)
    if len(rows) != B:
        raise EngineError(f"per-row stage counts must hold one entry per row ({B}), got {len(rows)}")
    out = []
    for b, v in enumerate(rows):
        if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= cap:
            raise EngineError(f"row {b}: a stage count lies in [1, {cap}], got {v!r}")
        out.append(int(v))
    return out


class _Ratios(list):
    """checked ratios 10^(-target / 10) on their way through the micro-batches of a call (CodecEngine._rate_in)"""
    def __getitem__(self, i):
        r = super().__getitem__(i)
        return _Ratios(r) if isinstance(i, slice) else r


class CodecEngine:
    """One engine per (device, checkpoint).  Calls on one engine are serialised by the caller,
    like a torch module's forward."""

    #: utterances processed per engine call.  Every op of the path is per-utterance, so results do not depend on it
    #: (tests/test_gpu_parity.py::test_full_size_determinism_and_batch_independence); it bounds the workspace
    #: (~0.57 GB per 10 s utterance for ds640) and keeps the persistent LSTM kernel (B <= 32) on its fast path.
    micro_batch = 16

    def __init__(self, arch: ArchSpec, device: "torch.device | str | int" = "cuda:0"):
        self.lib = _lib.load()
        self.arch = arch
        if arch.lstm_layers > 0 and arch.seq_model == "lstm" and arch.bottleneck_channels == 512:
            # H = 512: the persistent LSTM advances two 16-utterance batch tiles side by side (128 workgroups each), so 32 utterances
            # per call cost the recurrence what 16 do
            self.micro_batch = 32
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if dev.type != "cuda":
            raise EngineError(
                f"funcodec_amd runs on MI355X (gfx950) only; device={device!r} has no implementation "
                "(there is deliberately no CPU fallback)")
        self.device = torch.device("cuda", dev.index if dev.index is not None else 0)
        a = _lib.FcArch()
        a.abi_version = _lib.FC_ABI_VERSION
        a.sample_rate = arch.sample_rate
        a.audio_normalize = int(arch.audio_normalize)
        a.n_filters = arch.n_filters
        a.dimension = arch.dimension
        a.n_ratios = len(arch.ratios)
        for i, r in enumerate(arch.ratios):
            a.ratios[i] = int(r)
        a.kernel_size = arch.kernel_size
        a.last_kernel_size = arch.last_kernel_size
        a.residual_kernel_size = arch.residual_kernel_size
        a.compress = arch.compress
        a.lstm_layers = arch.lstm_layers
        a.lstm_skip = int(arch.lstm_skip)
        a.elu_alpha = arch.elu_alpha
        a.gn_eps = arch.gn_eps
        a.codebook_size = arch.codebook_size
        a.num_quantizers = arch.num_quantizers
        a.norm_type = {"time_group_norm": 0, "weight_norm": 1, "none": 2}[arch.norm]
        a.causal = int(arch.causal)
        a.n_residual_layers = arch.n_residual_layers
        a.dilation_base = arch.dilation_base
        a.model_type = {"encodec": 0, "freq_codec": 1}[arch.model_type]
        a.input_channels = arch.input_channels
        # audio channels of the time-domain codec (stereo: wav / recon tensors are [B,2,T]); FreqCodec is mono
        self.channels = 2 if (arch.model_type == "encodec" and arch.input_channels == 2) else 1
        a.n_fft = arch.n_fft
        a.stft_hop = arch.stft_hop
        for i, r in enumerate(arch.ratios_f):
            a.ratios_f[i] = int(r)
        a.enc_conv_group_ratio, a.dec_conv_group_ratio = arch.enc_conv_group_ratio, arch.dec_conv_group_ratio
        a.dec_tr_conv_group_ratio = arch.dec_tr_conv_group_ratio
        a.codec_dim = arch.codebook_dim if arch.codebook_dim != arch.dimension else 0
        a.codec_range = float(arch.codec_range or 0.0)
        a.q0_ds_ratio = int(arch.q0_ds_ratio)
        a.seq_model = {"lstm": 0, "transformer": 1}[arch.seq_model]
        a.seq_heads, a.seq_ff = SEQ_HEADS, SEQ_FF
        h = C.c_void_p()
        self._check(self.lib.fc_engine_create(C.byref(a), self.device.index, C.byref(h)))
        self._h = h
        self._ws: Optional[torch.Tensor] = None
        self._ws_need: Dict[tuple, int] = {}
        self._finalized = False

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(self.lib.fc_last_error().decode("utf-8", "replace"))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.lib.fc_engine_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def expected_tensors(self) -> Dict[str, tuple]:
        out = {}
        name = C.c_char_p()
        dims = (C.c_int64 * 4)()
        for i in range(self.lib.fc_engine_num_weights(self._h)):
            nd = self.lib.fc_engine_weight_info(self._h, i, C.byref(name), dims)
            out[name.value.decode()] = tuple(int(dims[j]) for j in range(nd))
        return out

    # -- checkpoint ----------------------------------------------------------------------------
    @_on_device
    def load_state_dict(self, state: Dict[str, "torch.Tensor | np.ndarray"]) -> None:
        """Tolerant load, like the reference's filter_state_dict
        (funcodec/torch_utils/load_pretrained_model.py:12-43): unknown keys (discriminator.*,
        mel_spec_transforms.*, EMA buffers) are skipped; a MISSING hot-path tensor is an error
        because, unlike the reference, we cannot run on random init silently."""
        want = self.expected_tensors()
        state = dict(state)
        # `use_ddp: false` checkpoints store one codebook per layer (core_vq.py:147-150)
        if "quantizer.rq.model.embed" not in state:
            per = []
            i = 0
            while f"quantizer.rq.model.layers.{i}._codebook.embed" in state:
                per.append(torch.as_tensor(state[f"quantizer.rq.model.layers.{i}._codebook.embed"]))
                i += 1
            if per:
                state["quantizer.rq.model.embed"] = torch.stack(per)
        inited = state.get("quantizer.rq.model.inited", None)
        if inited is not None and not bool(torch.as_tensor(inited).bool().all()):
            raise EngineError("checkpoint has un-initialised codebooks (quantizer.rq.model.inited == 0); the reference "
                              "would run k-means on the first batch (ddp_core_vq.py:149-159), which is training behaviour")
        for key, shape in want.items():
            if key not in state:
                raise EngineError(f"checkpoint is missing tensor {key} {shape}")
            t = torch.as_tensor(state[key]).detach().to("cpu", torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise EngineError(f"shape mismatch for {key}: checkpoint {tuple(t.shape)} vs architecture {shape}")
            dims = (C.c_int64 * 4)(*t.shape)
            self._check(self.lib.fc_engine_set_weight(self._h, key.encode(), C.c_void_p(t.data_ptr()), dims, t.dim()))
        skipped = [k for k in state if k not in want]
        if skipped:
            logging.info("funcodec_amd: skipped %d checkpoint tensors outside the hot path (e.g. %s)", len(skipped), skipped[0])
        self._check(self.lib.fc_engine_finalize(self._h))
        self._finalized = True

    # -- sizes ---------------------------------------------------------------------------------
    @property
    def hop_length(self) -> int:
        return self.lib.fc_engine_hop_length(self._h)

    def frames(self, n_samples: int) -> int:
        return self.lib.fc_engine_frames(self._h, n_samples)

    def decoded_samples(self, n_frames: int) -> int:
        """Samples the decoder emits for n_frames frames (n_frames * hop; stft_hop * (2-D time frames - 1) for freq_codec)."""
        return self.lib.fc_engine_decoded_samples(self._h, n_frames)

    def _workspace(self, B: int, T: int, ragged: bool = False) -> torch.Tensor:
        key = (B, T, "ragged") if ragged else (B, T)
        need = self._ws_need.get(key)
        if need is None:
            size = self.lib.fc_ragged_workspace_bytes if ragged else self.lib.fc_engine_workspace_bytes
            need = self._ws_need[key] = int(size(self._h, B, T))
            if ragged and need == 0:
                raise EngineError(ragged_refusal(self.arch) or "this engine has no length-aware calls")
        return self._scratch(need)

    def _scratch(self, nbytes: int) -> torch.Tensor:
        """the engine's one scratch buffer, grown to nbytes: calls and sessions keep nothing in it between calls"""
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None                   # the old buffer goes before the new one comes
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def work(self, B: int, T: int, n_q: int) -> Dict[str, float]:
        w = _lib.FcWork()
        self._check(self.lib.fc_engine_work(self._h, B, T, n_q, C.byref(w)))
        return {f: getattr(w, f) for f, _ in _lib.FcWork._fields_}

    def set_profiling(self, on: bool) -> None:
        self._check(self.lib.fc_engine_profile(self._h, int(on)))

    @_on_device
    def read_profile(self):
        """Per-kernel-class totals since the last read (synchronises on the last recorded event)."""
        arr = (_lib.FcProf * _lib.FC_PROF_CLASSES)()
        self._check(self.lib.fc_engine_profile_read(self._h, arr))
        return [dict(kernel=p.kernel.decode(), total_ms=p.total_ms, flops=p.flops, bytes=p.bytes, launches=p.launches)
                for p in arr]

    def _dev(self, t: torch.Tensor, dtype) -> torch.Tensor:
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _wav_in(self, wav: torch.Tensor) -> torch.Tensor:
        """[B,T] (mono engines) or [B,C,T] with C = the model's audio channels, on the device, contiguous fp32."""
        wav = self._dev(wav, torch.float32)
        if wav.dim() == 2 and self.channels == 1:
            return wav
        if wav.dim() != 3 or wav.shape[1] != self.channels:
            raise EngineError(f"wav must be [B,{self.channels},T]" + (" or [B,T]" if self.channels == 1 else "") + f", got {tuple(wav.shape)}")
        return wav

    def _lengths_in(self, lengths, B: int) -> torch.Tensor:
        """speech_lengths / token_lengths [B] of a length-aware call as device int32.  The range [1, Tmax] is checked on the device
        (clamped and reported through check_status), so no host round trip is made here."""
        why = ragged_refusal(self.arch)
        if why:
            raise EngineError(why)
        lengths = torch.as_tensor(lengths).reshape(-1)
        if lengths.numel() != B:
            raise EngineError(f"lengths must hold one entry per row ({B}), got {lengths.numel()}")
        return self._dev(lengths, torch.int32)

    @contextlib.contextmanager
    def _row_nq(self, rows):
        """The engine's per-row stage counts (fc_engine_set_row_nq) for the calls made inside; cleared on the way out, whatever
        happened, so a later plain call on this engine is untouched.  rows: None (nothing is set) or a checked list (row_nq_list)."""
        if rows is None:
            yield
            return
        self._check(self.lib.fc_engine_set_row_nq(self._h, (C.c_int32 * len(rows))(*rows), len(rows), self._stream()))
        try:
            yield
        finally:
            self.lib.fc_engine_set_row_nq(self._h, None, 0, None)

    @contextlib.contextmanager
    def _rate(self, ratios, min_n_q: int, n_q: int, Tf: int, want_stage_errors: bool = False, per_frame: bool = False):
        """The engine's rate (fc_engine_set_rate) for the offline call made inside: a stage count per row chosen on the device; cleared on
        the way out, whatever happened, as _row_nq does.  ratios: None (nothing is set, None is yielded) or a checked list (rate_targets).
        Yields dict(n_q_rows [B] i32, row_errors [B, n_q + 1] f64, stage_errors [n_q + 1, B, Tf] f32 | None): device tensors the call
        fills; nothing is read back.  per_frame (fc_engine_set_rate_frames; min_n_q may then be 0): also n_q_frames [B, Tf] i32, n_codes_rows
        [B] i32 and achieved_errors [B] f64; n_q_rows is then every row's largest frame count."""
        if ratios is None:
            yield None
            return
        B = len(ratios)
        out = dict(n_q_rows=torch.empty((B,), dtype=torch.int32, device=self.device),
                   row_errors=torch.empty((B, n_q + 1), dtype=torch.float64, device=self.device),
                   stage_errors=torch.empty((n_q + 1, B, Tf), dtype=torch.float32, device=self.device) if want_stage_errors else None)
        self._check(self.lib.fc_engine_set_rate(self._h, (C.c_double * B)(*ratios), B, max(int(min_n_q), 1), _ptr(out["n_q_rows"]),
                                                _ptr(out["row_errors"]), _ptr(out["stage_errors"]), self._stream()))
        try:
            if per_frame:
                out.update(n_q_frames=torch.empty((B, Tf), dtype=torch.int32, device=self.device),
                           n_codes_rows=torch.empty((B,), dtype=torch.int32, device=self.device),
                           achieved_errors=torch.empty((B,), dtype=torch.float64, device=self.device))
                self._check(self.lib.fc_engine_set_rate_frames(self._h, int(min_n_q), _ptr(out["n_q_frames"]), _ptr(out["n_codes_rows"]),
                                                               _ptr(out["achieved_errors"]), self._stream()))
            yield out
        finally:
            self.lib.fc_engine_set_rate(self._h, None, 0, 1, None, None, None, None)

    @contextlib.contextmanager
    def _floor(self, floors, min_n_q: int, n_q_out: Optional[torch.Tensor], fused: bool = True, row_errors: Optional[torch.Tensor] = None,
               stage_errors: Optional[torch.Tensor] = None, sub_quants: Optional[torch.Tensor] = None,
               n_q_frames_out: Optional[torch.Tensor] = None):
        # an entry None of floors: the row is switched off (it keeps its cap)
        """The engine's noise floor (fc_engine_set_floor) for the session push or the per-op hook made inside: a stage count per row chosen
        on the device from the frames of that push; cleared on the way out, whatever happened, as _row_nq does.  floors: None (nothing is
        set) or a checked list (floor_values); n_q_out: the device int32 [B] that receives the counts.  fused=False (or outputs given):
        fc_engine_set_floor_form.  n_q_frames_out (device int32 [B][frames of the push], dense): frame mode (fc_engine_set_floor_frames,
        the push frame rule): a count per frame, min_n_q may be 0, and n_q_out is not written."""
        if floors is None:
            yield
            return
        B = len(floors)
        off = [int(v is None) for v in floors]
        self._check(self.lib.fc_engine_set_floor(self._h, (C.c_double * B)(*[0.0 if v is None else v for v in floors]), B,
                                                 max(int(min_n_q), 1) if n_q_frames_out is not None else int(min_n_q), _ptr(n_q_out), self._stream()))
        try:
            if n_q_frames_out is not None:
                self._check(self.lib.fc_engine_set_floor_frames(self._h, int(min_n_q), _ptr(n_q_frames_out), self._stream()))
            if not fused or row_errors is not None or stage_errors is not None or sub_quants is not None or any(off):
                self._check(self.lib.fc_engine_set_floor_form(self._h, int(not fused), _ptr(row_errors), _ptr(stage_errors), _ptr(sub_quants),
                                                              (C.c_int32 * B)(*off) if any(off) else None, self._stream()))
            yield
        finally:
            self.lib.fc_engine_set_floor(self._h, None, 0, 1, None, None)

    @contextlib.contextmanager
    def _push_frame_nq(self, table: Optional[torch.Tensor]):
        """The engine's stage count per frame (fc_engine_set_push_frame_nq) for the session decode push made inside: table, device int32
        [B, Tfc], dense and borrowed; cleared on the way out, whatever happened.  None: nothing is set."""
        if table is None:
            yield
            return
        if table.dtype != torch.int32 or table.dim() != 2 or not table.is_contiguous():
            raise EngineError(f"a stage count per frame of a push is a dense int32 [B, Tfc] tensor, got {table.dtype} {tuple(table.shape)}")
        self._check(self.lib.fc_engine_set_push_frame_nq(self._h, _ptr(table), table.shape[0], table.shape[1], self._stream()))
        try:
            yield
        finally:
            self.lib.fc_engine_set_push_frame_nq(self._h, None, 0, 0, None)

    def _rate_in(self, target_snr_db, min_n_q, B: int, n_q: int, n_q_rows, per_frame: bool = False):
        """(ratios or None, min_n_q) of a call's target_snr_db / min_n_q, checked before anything reaches the device; a list of floats
        that _rate_in made itself (a micro-batch's slice) passes through.  per_frame: the floor lies in [0, cap]; without a target it is
        refused."""
        if target_snr_db is None:
            if per_frame:
                raise EngineError("per_frame chooses a stage count per frame by target_snr_db: give a target")
            return None, 1
        if isinstance(target_snr_db, _Ratios):
            return target_snr_db, min_n_q
        floor = rate_min_nq(self.arch, min_n_q, n_q, n_q_rows, floor=0 if per_frame else 1)
        return _Ratios(rate_targets(self.arch, target_snr_db, B)), floor

    @contextlib.contextmanager
    def _frame_nq(self, table, B: int, Tf: int):
        """A stage count per frame (fc_engine_set_frame_nq) for the decode_codes call made inside: a device int32 [B, Tf] the engine
        borrows; cleared on the way out, whatever happened.  table: None (nothing is set) or anything [B, Tf]; a device tensor stays on
        the device (the kernel clamps to [0, n_q])."""
        if table is None:
            yield
            return
        t = torch.as_tensor(table)
        if tuple(t.shape) != (B, Tf):
            raise EngineError(f"n_q_frames must be [B, Tf] = [{B}, {Tf}], got {tuple(t.shape)}")
        t = self._dev(t, torch.int32)
        self._check(self.lib.fc_engine_set_frame_nq(self._h, _ptr(t), B, Tf, self._stream()))
        try:
            yield
        finally:
            self.lib.fc_engine_set_frame_nq(self._h, None, 0, 0, None)

    @_on_device
    def set_rvq_beam(self, width) -> None:
        """Width of the quantiser's search over the stages (fc_engine_set_rvq_beam) for every call that follows on this engine -- offline,
        length-aware, session pushes; 1 (or None) clears it: the greedy quantiser, launching exactly what it always did."""
        width = rvq_beam_width(self.arch, width)
        self._check(self.lib.fc_engine_set_rvq_beam(self._h, width, self._stream()))

    @contextlib.contextmanager
    def _rvq_beam(self, width):
        """set_rvq_beam for the calls made inside; cleared on the way out, whatever happened, as _row_nq does.  width: checked
        (rvq_beam_width); 1 sets nothing."""
        if width is None or width == 1:
            yield
            return
        self.set_rvq_beam(width)
        try:
            yield
        finally:
            self.lib.fc_engine_set_rvq_beam(self._h, 1, None)

    # -- hot path ------------------------------------------------------------------------------
    # n_q_rows (encode, encode_decode, decode_codes; optional): a stage count per row, each <= n_q (decode_codes: the tokens' last
    # dimension).  Row b is then what the call with n_q = n_q_rows[b] gives it; codes and sub_quants of its later stages are 0, and a
    # decode does not read them.
    # Every call below takes an optional `lengths` [B]: without it the offline call over the whole batch width, as ever; with it the
    # length-aware (ragged) sibling, whose row b is what the call gives row b alone cut at lengths[b], zeros behind (fc_*_ragged).
    @staticmethod
    def _cat(parts, dims):
        """Concatenate per-micro-batch result dicts along each tensor's batch dimension."""
        out = {}
        for k, dim in dims.items():
            vals = [p[k] for p in parts]
            out[k] = None if vals[0] is None else torch.cat(vals, dim)
        return out

    @staticmethod
    def _rate_dims(ratios, per_frame: bool = False):
        """the batch dimensions of the outputs a rate adds, for _cat"""
        if ratios is None:
            return {}
        return dict(n_q_rows=0, row_errors=0, stage_errors=1, **(dict(n_q_frames=0, n_codes_rows=0, achieved_errors=0) if per_frame else {}))

    def _encode(self, decode: bool, wav, n_q, use_scale, want_sub_quants, want_enc_out, lengths, n_q_rows, target_snr_db, min_n_q,
                want_stage_errors, per_frame):
        """encode (fc_encode / fc_encode_ragged; the dict holds enc_out) or, with decode, encode_decode (fc_encode_decode / its ragged
        sibling; the dict holds recon)."""
        if n_q_rows is not None:                       # refused as a whole before anything reaches the device
            n_q_rows = row_nq_list(self.arch, n_q_rows, wav.shape[0], n_q)
        ratios, min_n_q = self._rate_in(target_snr_db, min_n_q, wav.shape[0], n_q, n_q_rows, per_frame)
        wav = self._wav_in(wav)
        B, T = wav.shape[0], wav.shape[-1]
        if lengths is not None:
            lengths = self._lengths_in(lengths, B)
        last = "recon" if decode else "enc_out"
        if B > self.micro_batch:
            parts = [self._encode(decode, wav[i:i + self.micro_batch], n_q, use_scale, want_sub_quants, want_enc_out,
                                  None if lengths is None else lengths[i:i + self.micro_batch],
                                  None if n_q_rows is None else n_q_rows[i:i + self.micro_batch],
                                  None if ratios is None else ratios[i:i + self.micro_batch], min_n_q, want_stage_errors, per_frame)
                     for i in range(0, B, self.micro_batch)]
            return self._cat(parts, dict(codes=1, quantized=0, sub_quants=1, scale=0, **{last: 0}, **self._rate_dims(ratios, per_frame)))
        Tf, D = self.frames(T), self.arch.dimension
        dev = self.device
        codes = torch.empty((n_q, B, Tf), dtype=torch.int64, device=dev)
        quant = torch.empty((B, Tf, D), dtype=torch.float32, device=dev)
        subq = torch.empty((n_q, B, self.arch.codebook_dim, Tf), dtype=torch.float32, device=dev) if want_sub_quants else None
        scale = torch.empty((B,), dtype=torch.float32, device=dev) if self.arch.audio_normalize else None
        if decode:
            out = torch.empty((B, self.channels, min(T, self.decoded_samples(Tf))), dtype=torch.float32, device=dev)   # like recon[:, :, :T] of the reference
        else:
            out = torch.empty((B, Tf, D), dtype=torch.float32, device=dev) if want_enc_out else None
        ws = self._workspace(B, T, lengths is not None)
        fn = getattr(self.lib, ("fc_encode_decode" if decode else "fc_encode") + ("_ragged" if lengths is not None else ""))
        args = [_ptr(wav)] + ([_ptr(lengths)] if lengths is not None else []) + [B, T, n_q] + ([int(use_scale)] if decode else [])
        with self._row_nq(n_q_rows), self._rate(ratios, min_n_q, n_q, Tf, want_stage_errors, per_frame) as rate:
            self._check(fn(self._h, *args, _ptr(codes), _ptr(quant), _ptr(subq), _ptr(scale), _ptr(out), _ptr(ws), ws.numel(), self._stream()))
        return dict(codes=codes, quantized=quant, sub_quants=subq, scale=None if scale is None else scale.view(B, 1), **{last: out},
                    **(rate or {}))

    @_on_device
    def encode(self, wav: torch.Tensor, n_q: int, want_sub_quants: bool = True, want_enc_out: bool = False, lengths=None, n_q_rows=None,
               target_snr_db=None, min_n_q: int = 1, want_stage_errors: bool = False, per_frame: bool = False):
        """wav [B,T] (or [B,C,T]) -> dict(codes [n_q,B,Tf] i64, quantized [B,Tf,D], sub_quants [n_q,B,D,Tf], scale [B,1]|None).
        target_snr_db (one value or B; optional): every row takes the smallest stage count in [min_n_q, its cap] whose quantiser-domain SNR
        reaches its target (rate_pick; the cap: n_q_rows[b], else n_q), chosen on the device inside the call.  The dict then also holds
        n_q_rows [B] i32, row_errors [B, n_q + 1] f64 and stage_errors [n_q + 1, B, Tf] f32 (None unless want_stage_errors), all on the device.
        per_frame (with target_snr_db): a count per FRAME (rate_pick_frames; min_n_q in [0, cap]): frame (b, t) is what the call
        with n_q = n_q_frames[b, t] gives it; the dict also holds n_q_frames [B, Tf] i32, n_codes_rows [B] i32 and achieved_errors [B] f64,
        and n_q_rows is every row's largest frame count."""
        return self._encode(False, wav, n_q, True, want_sub_quants, want_enc_out, lengths, n_q_rows, target_snr_db, min_n_q, want_stage_errors,
                            per_frame)

    @_on_device
    def encode_decode(self, wav: torch.Tensor, n_q: int, use_scale: bool = True, want_sub_quants: bool = True, lengths=None, n_q_rows=None,
                      target_snr_db=None, min_n_q: int = 1, want_stage_errors: bool = False, per_frame: bool = False):
        """encode + decode in one enqueue; target_snr_db, min_n_q, want_stage_errors, per_frame: as for encode (the reconstruction is made
        from the chosen counts)."""
        return self._encode(True, wav, n_q, use_scale, want_sub_quants, False, lengths, n_q_rows, target_snr_db, min_n_q, want_stage_errors,
                            per_frame)

    @_on_device
    def decode_codes(self, tokens: torch.Tensor, lengths=None, n_q_rows=None, n_q_frames=None):
        """tokens [B,Tf,n_q] i64 -> (wav [B,1,Tf*hop], emb [B,Tf,D]).  lengths: frames per row.  n_q_frames [B,Tf] (optional; a device
        tensor stays there): a stage count per frame, clamped to [0, n_q] on the device; the codes behind it are not read."""
        if n_q_rows is not None and n_q_frames is not None:
            raise EngineError("decode_codes: n_q_rows and n_q_frames are a count per row and a count per frame: give one of them")
        if n_q_rows is not None:                       # refused as a whole before anything reaches the device
            n_q_rows = row_nq_list(self.arch, n_q_rows, tokens.shape[0], tokens.shape[-1])
        tokens = self._dev(tokens, torch.int64)
        B, Tf, n_q = tokens.shape
        if lengths is not None:
            lengths = self._lengths_in(lengths, B)
        if B > self.micro_batch:
            parts = [self.decode_codes(tokens[i:i + self.micro_batch], None if lengths is None else lengths[i:i + self.micro_batch],
                                       None if n_q_rows is None else n_q_rows[i:i + self.micro_batch],
                                       None if n_q_frames is None else n_q_frames[i:i + self.micro_batch])
                     for i in range(0, B, self.micro_batch)]
            return torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)
        L = self.decoded_samples(Tf)
        wav = torch.empty((B, self.channels, L), dtype=torch.float32, device=self.device)
        emb = torch.empty((B, Tf, self.arch.dimension), dtype=torch.float32, device=self.device)
        ws = self._workspace(B, Tf * self.hop_length, lengths is not None)
        with self._row_nq(n_q_rows), self._frame_nq(n_q_frames, B, Tf):
            if lengths is not None:
                self._check(self.lib.fc_decode_codes_ragged(self._h, _ptr(tokens), _ptr(lengths), B, Tf, n_q, L, _ptr(wav), _ptr(emb), _ptr(ws),
                                                            ws.numel(), self._stream()))
            else:
                self._check(self.lib.fc_decode_codes(self._h, _ptr(tokens), B, Tf, n_q, L, _ptr(wav), _ptr(emb), _ptr(ws), ws.numel(),
                                                     self._stream()))
        return wav, emb

    @_on_device
    def decode_emb(self, emb: torch.Tensor, scale: Optional[torch.Tensor] = None, out_len: Optional[int] = None, lengths=None):
        """emb [B,Tf,D] -> wav [B,1,out_len or Tf*hop].  lengths: frames per row."""
        emb = self._dev(emb, torch.float32)
        B, Tf, D = emb.shape
        if D != self.arch.dimension:
            raise EngineError(f"embedding dim {D} != {self.arch.dimension}")
        if lengths is not None:
            lengths = self._lengths_in(lengths, B)
        if B > self.micro_batch:
            return torch.cat([self.decode_emb(emb[i:i + self.micro_batch],
                                              None if scale is None else scale.reshape(-1)[i:i + self.micro_batch], out_len,
                                              None if lengths is None else lengths[i:i + self.micro_batch])
                              for i in range(0, B, self.micro_batch)], 0)
        L = self.decoded_samples(Tf)
        out_len = L if out_len is None else int(out_len)
        sc = None if scale is None else self._dev(scale.reshape(-1), torch.float32)
        wav = torch.empty((B, self.channels, out_len), dtype=torch.float32, device=self.device)
        ws = self._workspace(B, Tf * self.hop_length, lengths is not None)
        if lengths is not None:
            self._check(self.lib.fc_decode_emb_ragged(self._h, _ptr(emb), _ptr(sc), _ptr(lengths), B, Tf, out_len, _ptr(wav), _ptr(ws),
                                                      ws.numel(), self._stream()))
        else:
            self._check(self.lib.fc_decode_emb(self._h, _ptr(emb), _ptr(sc), B, Tf, out_len, _ptr(wav), _ptr(ws), ws.numel(),
                                               self._stream()))
        return wav

    @_on_device
    def overlap_add(self, frames, stride: int, out_len: Optional[int] = None) -> torch.Tensor:
        """_linear_overlap_add (codec_basic.py:77-116) of decoded segments: frames = list of [B,1,L_f] device tensors
        (frame f starts at f*stride) -> [B,1,out_len or total]."""
        shape = tuple(frames[0].shape[:-1]) if frames[0].dim() == 3 else (frames[0].shape[0], 1)      # [B,C]: every channel row is overlap-added alone
        frames = [self._dev(f.reshape(-1, f.shape[-1]), torch.float32) for f in frames]
        B = frames[0].shape[0]
        lens = [int(f.shape[1]) for f in frames]
        total = stride * (len(frames) - 1) + lens[-1]
        out_len = total if out_len is None else min(int(out_len), total)
        ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64).to(self.device)     # plumbing: one small H2D
        lens_d = torch.tensor(lens, dtype=torch.int32).to(self.device)
        out = torch.empty((B, 1, out_len), dtype=torch.float32, device=self.device)
        self._check(self.lib.fc_overlap_add(_ptr(ptrs), _ptr(lens_d), len(frames), B, lens[0], int(stride), out_len, _ptr(out),
                                            self._stream()))
        return out.view(*shape, out_len)

    def debug_freq_features(self, buf: Optional[torch.Tensor], mode: int) -> None:
        """Test hook (fc_debug_freq_features): the next encode / encode_decode call of this thread hands its STFT-domain feature tensor
        [B, input_channels, n_fft / 2 + 1, frames] to `buf` (mode 1) or takes it from there (mode 2); mode 0 disarms."""
        if buf is not None and (buf.device != self.device or buf.dtype != torch.float32 or not buf.is_contiguous()):
            raise EngineError("debug_freq_features: a contiguous float32 tensor on the engine's device")
        self._check(self.lib.fc_debug_freq_features(_ptr(buf), 0 if buf is None else buf.numel() * 4, int(mode)))
        # the library keeps a RAW device pointer until the next encode call of this thread returns: keep the tensor alive at least that long
        # (the reference is replaced by the next hook and dropped with the engine)
        self._feat_hook_ref = buf if mode else None

    def check_status(self, sync: bool = True) -> None:
        """Raise if a kernel of an earlier call recorded a failure (persistent-LSTM barrier timeout, out-of-range code
        index).  With sync=True the engine's stream is synchronised first, so every call enqueued so far is covered."""
        if sync and torch.cuda.is_available():
            torch.cuda.current_stream(self.device).synchronize()
        self._check(self.lib.fc_engine_status(self._h, None))

    # -- the bit stream (csrc/code_pack_kernels.h states the packet; funcodec_amd/io.py restates it on the host) ----------------
    @property
    def code_bits(self) -> int:
        """bits per code in a packet: ceil(log2(codebook_size))"""
        from .io import code_bits
        return code_bits(self.arch.codebook_size)

    def _rows_i32(self, rows, B: int, what: str) -> Optional[torch.Tensor]:
        """frames or stage counts per row as device int32 [B]; a device tensor stays on the device (nothing is read back: the kernel clamps)"""
        if rows is None:
            return None
        rows = torch.as_tensor(rows).reshape(-1)
        if rows.numel() != B:
            raise EngineError(f"{what} must hold one entry per row ({B}), got {rows.numel()}")
        return self._dev(rows, torch.int32)

    @_on_device
    def pack_codes(self, codes: torch.Tensor, frames_rows=None, n_q_rows=None, n_q_frames=None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """codes [n_q,B,Tf] i64 -> packets uint8 [B, pitch] on the device (fc_codes_pack), one packet per row with zeros behind it.
        frames_rows, n_q_rows [B] (optional; lists, or tensors on any device -- ``n_q_rows`` of a ``target_snr_db`` call goes in as it
        is): the row's frames and stage count, clamped on the device to [0, Tf] and [1, n_q]; nothing behind them is read.
        n_q_frames [B,Tf] (optional; ``n_q_frames`` of a ``per_frame`` call goes in as it is): packets of mode 1, a count per frame
        (fc_codes_pack_frames), clamped on the device to [0, n_q]; n_q_rows is then not needed (the header's kmax is made on the device)."""
        codes = self._dev(codes, torch.int64)
        if codes.dim() != 3:
            raise EngineError(f"pack_codes: codes must be [n_q,B,Tf], got {tuple(codes.shape)}")
        n_q, B, Tf = codes.shape
        fr, nq = self._rows_i32(frames_rows, B, "frames_rows"), self._rows_i32(n_q_rows, B, "n_q_rows")
        bits = self.code_bits
        if n_q_frames is not None:
            kf = torch.as_tensor(n_q_frames)
            if tuple(kf.shape) != (B, Tf):
                raise EngineError(f"pack_codes: n_q_frames must be [B, Tf] = [{B}, {Tf}], got {tuple(kf.shape)}")
            kf = self._dev(kf, torch.int32)
            pitch = int(self.lib.fc_frame_packet_pitch(Tf, n_q, bits))
            packets = torch.empty((B, pitch), dtype=torch.uint8, device=self.device)
            need = int(self.lib.fc_frame_pack_workspace_bytes(B, Tf))     # the scan's workspace: the caller's (a session's fixed buffer), or one made here
            if ws is None or ws.numel() < need:
                ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
            self._check(self.lib.fc_codes_pack_frames(_ptr(codes), B, Tf, n_q, bits, _ptr(fr), _ptr(kf), _ptr(packets), pitch, _ptr(ws), ws.numel(),
                                                      self._stream()))
            return packets
        pitch = int(self.lib.fc_code_packet_pitch(Tf, n_q, bits))
        packets = torch.empty((B, pitch), dtype=torch.uint8, device=self.device)
        self._check(self.lib.fc_codes_pack(_ptr(codes), B, Tf, n_q, bits, _ptr(fr), _ptr(nq), _ptr(packets), pitch, self._stream()))
        return packets

    @_on_device
    def unpack_codes(self, packets: torch.Tensor, Tf: int, n_q: Optional[int] = None) -> torch.Tensor:
        """packets uint8 [B, pitch] -> tokens [B,Tf,n_q] i64 (fc_codes_unpack), the layout the decode calls take: zeros at the stages
        behind a row's count and the frames behind its frames.  n_q: the tokens' last dimension (default: the model's num_quantizers)."""
        packets = self._dev(packets, torch.uint8)
        if packets.dim() != 2:
            raise EngineError(f"unpack_codes: packets must be [B, pitch], got {tuple(packets.shape)}")
        n_q = self.arch.num_quantizers if n_q is None else int(n_q)
        B, pitch = packets.shape
        tokens = torch.empty((B, int(Tf), n_q), dtype=torch.int64, device=self.device)
        self._check(self.lib.fc_codes_unpack(_ptr(packets), pitch, B, int(Tf), n_q, self.code_bits, _ptr(tokens), self._stream()))
        return tokens

    @_on_device
    def unpack_frame_codes(self, packets: torch.Tensor, Tf: int, n_q: Optional[int] = None):
        """packets uint8 [B, pitch], every row of mode 0 or mode 1 -> (tokens [B,Tf,n_q] i64, n_q_frames [B,Tf] i32) on the device
        (fc_codes_unpack_frames): zeros behind every frame's count and every row's frames; a mode-0 row counts its k in every frame.
        Both go to decode_codes(tokens, n_q_frames=...) as they are: packets to waveform without a read-back."""
        packets = self._dev(packets, torch.uint8)
        if packets.dim() != 2:
            raise EngineError(f"unpack_frame_codes: packets must be [B, pitch], got {tuple(packets.shape)}")
        n_q = self.arch.num_quantizers if n_q is None else int(n_q)
        B, pitch = packets.shape
        Tf = int(Tf)
        tokens = torch.empty((B, Tf, n_q), dtype=torch.int64, device=self.device)
        kf = torch.empty((B, Tf), dtype=torch.int32, device=self.device)
        ws = torch.empty((int(self.lib.fc_frame_pack_workspace_bytes(B, Tf)),), dtype=torch.uint8, device=self.device)
        self._check(self.lib.fc_codes_unpack_frames(_ptr(packets), pitch, B, Tf, n_q, self.code_bits, _ptr(tokens), _ptr(kf), _ptr(ws), ws.numel(),
                                                    self._stream()))
        return tokens, kf

    def _parse_packets_any(self, rows, exact):
        """(modes, frames, counts, lengths) of host packets of either mode, every header checked (bits, mode, k <= num_quantizers, a
        mode-1 packet's counts, length); a bad one raises EngineError naming the row and the field.  counts: k, or a mode-1 packet's
        largest count.  exact=None: the rows are headers alone (lengths are then None)."""
        from .io import PacketError, parse_any_packet
        modes, frames, counts, lengths = [], [], [], []
        for b, p in enumerate(rows):
            try:
                mode, f, k, _, _, need = parse_any_packet(p, self.arch.num_quantizers, self.code_bits, exact=exact)
            except PacketError as err:
                raise EngineError(f"row {b}: packet field {err}") from None
            modes.append(mode)
            frames.append(f)
            counts.append(k)
            lengths.append(need)
        return modes, frames, counts, lengths

    def _parse_packets(self, rows, exact):
        """(frames, counts) of host packets, checked as _parse_packets_any checks them"""
        return self._parse_packets_any(rows, exact)[1:3]

    def packets_to_host(self, packets: torch.Tensor):
        """packets uint8 [B, pitch] -> list of B bytes: ONE copy to the host, every row cut at its own packet length (a mode-1 row's
        length comes from its counts section, which the host then holds)"""
        host = packets.cpu().numpy()
        rows = [host[b].tobytes() for b in range(host.shape[0])]
        lengths = self._parse_packets_any(rows, exact=False)[3]
        return [r[:n] for r, n in zip(rows, lengths)]

    def packets_from_host(self, packets, n_q: Optional[int] = None):
        """list of B bytes -> (packets uint8 [B, pitch] on the device, Tf, counts): every header is validated first (bits, mode,
        k <= n_q, and a length of exactly fc_code_packet_bytes); Tf is the largest frame count, the pitch that of (Tf, n_q) with n_q the
        largest count unless given.  Packets of mode 1 (a count per frame) pass too: counts then holds the packet's largest count, the
        pitch is the mode-1 pitch, and ``packets_modes(packets)`` tells which unpack call the buffer needs."""
        from .io import frame_packet_pitch, packet_pitch
        packets = [bytes(p) for p in packets]
        if not packets:
            raise EngineError("packets_from_host: no packets")
        modes, frames, counts, _ = self._parse_packets_any(packets, exact=True)
        pitch_of = frame_packet_pitch if any(modes) else packet_pitch      # a buffer that holds a mode-1 row has the mode-1 pitch
        if n_q is not None:
            for b, k in enumerate(counts):
                if k > n_q:
                    raise EngineError(f"row {b}: packet field k: {k} stages, more than the {n_q} of this call")
        Tf = max(max(frames), 1)
        pitch = pitch_of(Tf, max(counts) if n_q is None else int(n_q), self.code_bits)
        host = np.zeros((len(packets), pitch), dtype=np.uint8)
        for b, p in enumerate(packets):
            host[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        return torch.from_numpy(host).to(self.device), Tf, counts

    @staticmethod
    def packets_modes(packets) -> list:
        """the mode (0: one count per packet, 1: a count per frame) of every host packet"""
        from .io import packet_mode
        return [packet_mode(bytes(p)) for p in packets]

    # -- per-op entry points (tests) -----------------------------------------------------------
    @_on_device
    def rvq_encode(self, x: torch.Tensor, n_q: int, n_q_rows=None, beam: int = 1, return_paths: bool = False, target_snr_db=None,
                   min_n_q: int = 1, per_frame: bool = False, noise_floor_db=None, fused: bool = True):
        """x [N,D] -> (codes [n_q,N], quantized [N,D]).  target_snr_db (a list of B, or with n_q_rows one value or B; fc_rvq_encode_rate):
        the N rows are B utterances of N / B frames each, every one takes the stage count the rule picks (rate_pick; n_q_rows are the caps)
        -> (codes, quantized, dict(n_q_rows [B] i32, row_errors [B, n_q + 1] f64, stage_errors [n_q + 1, B, N / B] f32)).  n_q_rows (B entries): the N rows are B utterances of N / B frames each, utterance b
        with n_q_rows[b] stages.  beam (2, 4, 8): the search over the stages (fc_rvq_encode_beam) instead of the greedy quantiser;
        return_paths: also (paths [beam,n_q,N] i64, errors [beam,N]), every slot's final path and its fixed-order residual energy.
        per_frame (with target_snr_db): a count per frame (rate_pick_frames; min_n_q in [0, cap]); the dict also holds n_q_frames
        [B, N / B] i32, n_codes_rows [B] i32 and achieved_errors [B] f64.
        noise_floor_db (a list of B, or with n_q_rows one value or B): the push rule instead (floor_pick; fc_engine_set_floor): the N rows
        are ONE push of B rows of N / B frames each -> (codes, quantized, dict(n_q_rows, row_errors, stage_errors)) as for target_snr_db,
        plus sub_quants [n_q, B, D, N / B] in the dict.
        fused=False runs the four-launch chain in place of the one fused launch (a push wider than 256 frames always does): same bits.
        noise_floor_db with per_frame: the push frame rule (floor_pick_frames; fc_engine_set_floor_frames; min_n_q in [0, cap]): a count
        per frame -> dict(n_q_frames [B, N / B] i32, stage_errors, sub_quants); one launch at any width, or the chain with fused=False."""
        beam = rvq_beam_width(self.arch, beam)
        if noise_floor_db is not None:
            if target_snr_db is not None:
                raise EngineError("rvq_encode: noise_floor_db and target_snr_db are two rules (a floor per push, a rate per call): give one")
            if return_paths:
                raise EngineError("rvq_encode: return_paths and noise_floor_db are two hooks (fc_rvq_encode_beam, fc_rvq_encode_rate)")
            rows_b = len(n_q_rows) if n_q_rows is not None else (1 if isinstance(noise_floor_db, numbers.Real) else len(noise_floor_db))
            floors = floor_values(self.arch, noise_floor_db, rows_b)
            if n_q_rows is not None:
                n_q_rows = row_nq_list(self.arch, n_q_rows, rows_b, n_q)
            min_n_q = rate_min_nq(self.arch, min_n_q, n_q, n_q_rows, floor=0 if per_frame else 1)
            x = self._dev(x, torch.float32)
            N, D = x.shape
            if D != self.arch.codebook_dim:
                raise EngineError(f"rvq_encode: rows must have {self.arch.codebook_dim} dims, got {D}")
            if N % rows_b != 0:
                raise EngineError(f"rvq_encode: {N} rows are not {rows_b} utterances of equal length")
            codes = torch.empty((n_q, N), dtype=torch.int64, device=self.device)
            quant = torch.empty((N, D), dtype=torch.float32, device=self.device)
            out = dict(n_q_rows=torch.empty((rows_b,), dtype=torch.int32, device=self.device),
                       row_errors=torch.empty((rows_b, n_q + 1), dtype=torch.float64, device=self.device),
                       stage_errors=torch.empty((n_q + 1, rows_b, N // rows_b), dtype=torch.float32, device=self.device),
                       sub_quants=torch.empty((n_q, rows_b, D, N // rows_b), dtype=torch.float32, device=self.device))
            if per_frame:       # the push frame rule: no row sums; n_q_rows is not written
                out["n_q_frames"] = torch.empty((rows_b, N // rows_b), dtype=torch.int32, device=self.device)
                del out["row_errors"]
            with self._row_nq(n_q_rows), self._floor(floors, min_n_q, out["n_q_rows"], fused, out.get("row_errors"), out["stage_errors"],
                                                     out["sub_quants"], out.get("n_q_frames")):
                self._check(self.lib.fc_rvq_encode_rate(self._h, _ptr(x), N, n_q, beam, _ptr(codes), _ptr(quant), self._stream()))
            if per_frame:
                del out["n_q_rows"]
            return codes, quant, out
        if per_frame and target_snr_db is None:
            raise EngineError("rvq_encode: per_frame chooses a stage count per frame by target_snr_db: give a target")
        if return_paths and beam == 1:
            raise EngineError("rvq_encode: return_paths needs rvq_beam above 1 (the paths are those of a search)")
        if n_q_rows is not None:
            n_q_rows = row_nq_list(self.arch, n_q_rows, len(n_q_rows), n_q)
            if x.shape[0] % len(n_q_rows) != 0:
                raise EngineError(f"rvq_encode: {x.shape[0]} rows are not {len(n_q_rows)} utterances of equal length")
        ratios = None
        if target_snr_db is not None:
            if return_paths:
                raise EngineError("rvq_encode: return_paths and target_snr_db are two hooks (fc_rvq_encode_beam, fc_rvq_encode_rate)")
            rows_b = len(n_q_rows) if n_q_rows is not None else (1 if isinstance(target_snr_db, numbers.Real) else len(target_snr_db))
            ratios, min_n_q = self._rate_in(target_snr_db, min_n_q, rows_b, n_q, n_q_rows, per_frame)
            if x.shape[0] % rows_b != 0:
                raise EngineError(f"rvq_encode: {x.shape[0]} rows are not {rows_b} utterances of equal length")
        x = self._dev(x, torch.float32)
        N, D = x.shape
        if D != self.arch.codebook_dim:
            raise EngineError(f"rvq_encode: rows must have {self.arch.codebook_dim} dims, got {D}")
        codes = torch.empty((n_q, N), dtype=torch.int64, device=self.device)
        quant = torch.empty((N, D), dtype=torch.float32, device=self.device)
        if ratios is not None:
            with self._row_nq(n_q_rows), self._rate(ratios, min_n_q, n_q, N // len(ratios), True, per_frame) as rate:
                self._check(self.lib.fc_rvq_encode_rate(self._h, _ptr(x), N, n_q, beam, _ptr(codes), _ptr(quant), self._stream()))
            return codes, quant, rate
        if beam > 1:
            paths = torch.empty((beam, n_q, N), dtype=torch.int64, device=self.device) if return_paths else None
            errors = torch.empty((beam, N), dtype=torch.float32, device=self.device) if return_paths else None
            with self._row_nq(n_q_rows):
                self._check(self.lib.fc_rvq_encode_beam(self._h, _ptr(x), N, n_q, beam, _ptr(codes), _ptr(quant), _ptr(paths), _ptr(errors),
                                                        self._stream()))
            return (codes, quant, paths, errors) if return_paths else (codes, quant)
        ws = torch.empty(N, dtype=torch.int32, device=self.device) if self.arch.q0_ds_ratio > 1 else None     # stage-0 source-row table
        with self._row_nq(n_q_rows):
            self._check(self.lib.fc_rvq_encode(self._h, _ptr(x), N, n_q, _ptr(codes), _ptr(quant), _ptr(ws) if ws is not None else None,
                                               0 if ws is None else 4 * N, self._stream()))
        return codes, quant

    def _sources(self, what: str, shape, aff0, x1, aff1):
        """(x1, aff0, aff1) of a per-layer call on the device, checked against the layer's input shape [B, C, T]."""
        B, Cin = shape[0], shape[1]
        if x1 is None and aff1 is not None:
            raise EngineError(f"{what}: aff1 without x1")
        if x1 is not None:
            x1 = self._dev(x1, torch.float32)
            if tuple(x1.shape) != tuple(shape):
                raise EngineError(f"{what}: x1 must be [B,C,T] = {tuple(shape)}, got {tuple(x1.shape)}")
        affs = []
        for a in (aff0, aff1):
            if a is not None:
                a = self._dev(a, torch.float32)
                if tuple(a.shape) != (B, Cin, 2):
                    raise EngineError(f"{what}: an affine must be [B,C,2] = {(B, Cin, 2)}, got {tuple(a.shape)}")
            affs.append(a)
        return x1, affs[0], affs[1]

    @_on_device
    def layer_forward(self, prefix: str, x: torch.Tensor, apply_elu: bool = False, *, aff0: Optional[torch.Tensor] = None,
                      div: Optional[torch.Tensor] = None, x1: Optional[torch.Tensor] = None, aff1: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One 1-D layer (fc_layer_forward / fc_layer_forward_src) on act(aff0(x / div) + aff1(x1)): x, x1 [B,C,T], pending GroupNorm
        affines aff0, aff1 [B,C,2] (scale, shift), div [B] (the encoder's first conv only), act = ELU when apply_elu -> the layer's output
        [B, Cout, Tout], GroupNorm'd (raw for weight_norm nets)."""
        x = self._dev(x, torch.float32)
        B, Cin, T = x.shape
        Tout = self.lib.fc_layer_out_len(self._h, prefix.encode(), T)
        if Tout < 0:
            if self.arch.model_type == "freq_codec" and prefix + ".conv.bias" in self.expected_tensors():
                raise EngineError(f"layer {prefix} is a 2-D layer of the STFT-domain codec: use layer2d_forward")
            raise EngineError(f"unknown layer {prefix}")
        exp = self.expected_tensors()
        tr = prefix.endswith("convtr")
        inner = ".convtr" if tr else ".conv"
        cout = exp[prefix + inner + ".bias"][0]
        wshape = exp.get(prefix + inner + ".weight", exp.get(prefix + inner + ".weight_v"))
        cin = wshape[0] if tr else wshape[1]
        if Cin != cin:
            raise EngineError(f"layer {prefix}: expected input [B, {cin}, T], got {tuple(x.shape)}")
        x1, aff0, aff1 = self._sources(f"layer {prefix}", x.shape, aff0, x1, aff1)
        if div is not None:
            div = self._dev(div.reshape(-1), torch.float32)
            if div.numel() != B:
                raise EngineError(f"layer {prefix}: div must hold one scale per utterance ({B}), got {div.numel()}")
        y = torch.empty((B, cout, Tout), dtype=torch.float32, device=self.device)
        self._workspace(B, max(T, Tout) * 4 + 4096)
        # the layer's output + statistics, and a materialised (activated, summed) input for layers with >= 3 row tiles
        ws = self._scratch((B * cout * (Tout + 64) * 4) * 2 + B * cin * (T + 2048) * 4 + (1 << 20))
        if aff0 is None and div is None and x1 is None:
            rc = self.lib.fc_layer_forward(self._h, prefix.encode(), _ptr(x), B, T, int(apply_elu), _ptr(y), _ptr(ws), ws.numel(), self._stream())
        else:
            rc = self.lib.fc_layer_forward_src(self._h, prefix.encode(), _ptr(x), _ptr(aff0), _ptr(div), _ptr(x1), _ptr(aff1), B, T,
                                               int(apply_elu), _ptr(y), _ptr(ws), ws.numel(), self._stream())
        self._check(rc)
        return y

    @_on_device
    def layer2d_forward(self, prefix: str, x0: torch.Tensor, aff0: Optional[torch.Tensor] = None, x1: Optional[torch.Tensor] = None,
                        aff1: Optional[torch.Tensor] = None, apply_elu: bool = False, out_halo: int = 0) -> torch.Tensor:
        """One 2-D layer of the STFT-domain codec (fc_layer2d_forward): x0, x1 [B,C,F,T] and pending affines aff0, aff1 [B,C,2]
        (scale, shift) -> the layer's output [B, Cout, Fo + 2 out_halo, Tout], GroupNorm'd (raw for weight_norm nets), halo rows included."""
        x0 = self._dev(x0, torch.float32)
        if x0.dim() != 4:
            raise EngineError(f"layer2d_forward: x0 must be [B,C,F,T], got {tuple(x0.shape)}")
        B, Cin, Fq, T = x0.shape
        dims = (C.c_int64 * 5)()
        self._check(self.lib.fc_layer2d_out_shape(self._h, prefix.encode(), B, Fq, T, int(out_halo), dims))
        if Cin != int(dims[4]):
            raise EngineError(f"layer {prefix}: expected input [B, {int(dims[4])}, F, T], got {tuple(x0.shape)}")
        srcs = [(x0, aff0)] + ([(x1, aff1)] if x1 is not None else [])
        if x1 is None and aff1 is not None:
            raise EngineError("layer2d_forward: aff1 without x1")
        conv = []
        for x, a in srcs:
            x = self._dev(x, torch.float32)
            if tuple(x.shape) != (B, Cin, Fq, T):
                raise EngineError(f"layer2d_forward: every source must be [B,C,F,T] = {(B, Cin, Fq, T)}, got {tuple(x.shape)}")
            if a is not None:
                a = self._dev(a, torch.float32)
                if tuple(a.shape) != (B, Cin, 2):
                    raise EngineError(f"layer2d_forward: an affine must be [B,C,2] = {(B, Cin, 2)}, got {tuple(a.shape)}")
            conv.append((x, a))
        y = torch.empty((B, int(dims[0]), int(dims[1]), int(dims[2])), dtype=torch.float32, device=self.device)
        need = int(dims[3])
        ws = self._scratch(need)
        (s0, a0), (s1, a1) = conv[0], (conv[1] if len(conv) > 1 else (None, None))
        self._check(self.lib.fc_layer2d_forward(self._h, prefix.encode(), _ptr(s0), _ptr(a0), _ptr(s1), _ptr(a1), B, Fq, T, int(apply_elu),
                                                int(out_halo), _ptr(y), _ptr(ws), ws.numel(), self._stream()))
        return y

    @_on_device
    def freq_synthesis(self, dec: torch.Tensor, aff: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                       out_len: Optional[int] = None, want_spec: bool = False):
        """The back end of the STFT-domain codec behind the 2-D decoder (fc_freq_synthesis): dec [B,C,F,Tp] (the decoder's last conv, raw),
        its pending GroupNorm affine aff [B,C,2] (scale, shift), scale [B] -> wav [B, out_len] (default stft_hop * (Tp - 1)); with
        want_spec also the spectrum rows [B, 2 F, Tp] (real rows, then imaginary rows) the inverse-DFT GEMM reads."""
        dec = self._dev(dec, torch.float32)
        if dec.dim() != 4:
            raise EngineError(f"freq_synthesis: dec must be [B,C,F,Tp], got {tuple(dec.shape)}")
        B, Cc, Fq, Tp = dec.shape
        if out_len is None:
            out_len = self.arch.stft_hop * (Tp - 1)
        need = C.c_size_t()
        self._check(self.lib.fc_freq_synthesis_size(self._h, B, Cc, Fq, Tp, int(out_len), C.byref(need)))
        if aff is not None:
            aff = self._dev(aff, torch.float32)
            if tuple(aff.shape) != (B, Cc, 2):
                raise EngineError(f"freq_synthesis: the affine must be [B,C,2] = {(B, Cc, 2)}, got {tuple(aff.shape)}")
        if scale is not None:
            scale = self._dev(scale.reshape(-1), torch.float32)
            if scale.numel() != B:
                raise EngineError(f"freq_synthesis: scale must hold one value per utterance ({B}), got {scale.numel()}")
        wav = torch.empty((B, int(out_len)), dtype=torch.float32, device=self.device)
        spec = torch.empty((B, 2 * Fq, Tp), dtype=torch.float32, device=self.device) if want_spec else None
        ws = self._scratch(need.value)
        self._check(self.lib.fc_freq_synthesis(self._h, _ptr(dec), _ptr(aff), _ptr(scale), B, Cc, Fq, Tp, int(out_len), _ptr(wav), _ptr(spec),
                                               _ptr(ws), ws.numel(), self._stream()))
        return (wav, spec) if want_spec else wav

    def freq_halo(self) -> int:
        """Frequency halo rows of the engine's 2-D activations (the out_halo layer2d_forward accepts besides 0)."""
        dims = (C.c_int64 * 5)()
        for k in self.expected_tensors():
            if k.endswith(".conv.bias") and k.startswith("encoder.model.0."):
                self._check(self.lib.fc_layer2d_out_shape(self._h, k[:-len(".conv.bias")].encode(), 1, 1, 1, -1, dims))
                return int(dims[0])
        raise EngineError("freq_halo: not an STFT-domain codec")

    @_on_device
    def resblock_forward(self, prefix: str, x: torch.Tensor, *, aff0: Optional[torch.Tensor] = None, x1: Optional[torch.Tensor] = None,
                         aff1: Optional[torch.Tensor] = None) -> torch.Tensor:
        """SEANetResnetBlock.forward of the block at Sequential prefix `prefix` (e.g. "encoder.model.1") on aff0(x) + aff1(x1)
        (fc_resblock_forward / fc_resblock_forward_src; affines [B,C,2] (scale, shift)): [B,C,T] -> [B,C,T]."""
        x = self._dev(x, torch.float32)
        B, Cc, T = x.shape
        x1, aff0, aff1 = self._sources(f"block {prefix}", x.shape, aff0, x1, aff1)
        y = torch.empty_like(x)
        need = B * Cc * (T + 64) * 4 * 6 + (4 << 20)      # both branches, the hidden one, and up to two materialised inputs
        ws = self._scratch(need)
        if aff0 is None and x1 is None:
            rc = self.lib.fc_resblock_forward(self._h, prefix.encode(), _ptr(x), B, T, _ptr(y), _ptr(ws), ws.numel(), self._stream())
        else:
            rc = self.lib.fc_resblock_forward_src(self._h, prefix.encode(), _ptr(x), _ptr(aff0), _ptr(x1), _ptr(aff1), B, T, _ptr(y), _ptr(ws),
                                                  ws.numel(), self._stream())
        self._check(rc)
        return y

    @_on_device
    def lstm_forward(self, prefix: str, x: torch.Tensor) -> torch.Tensor:
        x = self._dev(x, torch.float32)
        B, H, T = x.shape
        want = self.expected_tensors().get(prefix + ".weight_hh_l0")
        if want is None or want[1] != H:
            raise EngineError(f"lstm {prefix!r}: expected input [B, {want[1] if want else '?'}, T], got {tuple(x.shape)}")
        y = torch.empty_like(x)
        need = (T * B * 4 * H + 3 * B * H + B * H * T + (2 * T + 1) * 16 * ((B + 15) // 16) * H) * 4 * self.arch.lstm_layers + (1 << 20)
        ws = self._scratch(need)
        self._check(self.lib.fc_lstm_forward(self._h, prefix.encode(), _ptr(x), B, T, _ptr(y), _ptr(ws), ws.numel(), self._stream()))
        return y

    @_on_device
    def seq_forward(self, prefix: str, x: torch.Tensor) -> torch.Tensor:
        """TransformerEncoder.forward of the bottleneck transformer at Sequential prefix `prefix` (e.g. "encoder.model.16"): all blocks,
        after_norm and the res_seq skip, [B,C,T] -> [B,C,T]."""
        x = self._dev(x, torch.float32)
        B, Cc, T = x.shape
        want = self.expected_tensors().get(prefix + ".after_norm.weight")
        if want is None or want[0] != Cc:
            raise EngineError(f"transformer {prefix!r}: expected input [B, {want[0] if want else '?'}, T], got {tuple(x.shape)}")
        y = torch.empty_like(x)
        # residual stream, LayerNorm out, branch out, attention out, result: 5 x [B,C,T]; q|k|v [B,3C,T]; feed-forward hidden [B,ff,T]
        need = 4 * B * T * (8 * Cc + SEQ_FF) + (1 << 20)
        ws = self._scratch(need)
        self._check(self.lib.fc_seq_forward(self._h, prefix.encode(), _ptr(x), B, T, _ptr(y), _ptr(ws), ws.numel(), self._stream()))
        return y

    @_on_device
    def stream_seq_forward(self, session, x: torch.Tensor, decoder: bool = False) -> torch.Tensor:
        """Test hook (fc_seqstream_forward): the transformer stage of a push alone, without the res_seq skip, on the key / value cache
        of the encoder / decoder side of `session` (a CodecStream opened with max_frames): x [B,C,T] -> [B,C,T].  It advances that
        side's frame count, so consecutive calls continue one utterance."""
        x = self._dev(x, torch.float32)
        B, Cc, T = x.shape
        if B != session.batch or Cc != self.arch.bottleneck_channels:
            raise EngineError(f"stream_seq_forward: x must be [{session.batch},{self.arch.bottleneck_channels},T], got {tuple(x.shape)}")
        y = torch.empty_like(x)
        # fc_seq_forward's buffers for the chunk, and the partials of the cached attention's key split: 16 units x 16 queries x (DK + 2) per head
        need = 4 * B * T * (8 * Cc + SEQ_FF) + 4 * B * 256 * (Cc + 2 * SEQ_HEADS) + (1 << 20)
        ws = self._scratch(need)
        self._check(self.lib.fc_seqstream_forward(session._h, int(decoder), _ptr(x), T, _ptr(y), _ptr(ws), ws.numel(), self._stream()))
        return y
