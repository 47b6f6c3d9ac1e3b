"""ctypes binding of include/funcodec_amd.h (the C ABI of the gfx950 engine)."""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

FC_MAX_RATIOS = 8
FC_ABI_VERSION = 7


class FcArch(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("sample_rate", C.c_int32), ("audio_normalize", C.c_int32),
        ("n_filters", C.c_int32), ("dimension", C.c_int32), ("n_ratios", C.c_int32),
        ("ratios", C.c_int32 * FC_MAX_RATIOS),
        ("kernel_size", C.c_int32), ("last_kernel_size", C.c_int32), ("residual_kernel_size", C.c_int32),
        ("compress", C.c_int32), ("lstm_layers", C.c_int32), ("lstm_skip", C.c_int32),
        ("elu_alpha", C.c_float), ("gn_eps", C.c_float),
        ("codebook_size", C.c_int32), ("num_quantizers", C.c_int32),
        ("norm_type", C.c_int32), ("causal", C.c_int32), ("n_residual_layers", C.c_int32), ("dilation_base", C.c_int32),
        ("model_type", C.c_int32), ("input_channels", C.c_int32), ("n_fft", C.c_int32), ("stft_hop", C.c_int32),
        ("ratios_f", C.c_int32 * FC_MAX_RATIOS),
        ("enc_conv_group_ratio", C.c_int32), ("dec_conv_group_ratio", C.c_int32), ("dec_tr_conv_group_ratio", C.c_int32),
        ("codec_dim", C.c_int32), ("codec_range", C.c_float),
        ("q0_ds_ratio", C.c_int32),
        ("seq_model", C.c_int32), ("seq_heads", C.c_int32), ("seq_ff", C.c_int32),
    ]


class FcWork(C.Structure):
    _fields_ = [("total_flops", C.c_double), ("total_bytes", C.c_double), ("conv_flops", C.c_double),
                ("conv_bytes", C.c_double), ("lstm_flops", C.c_double), ("rvq_flops", C.c_double),
                ("conv_launches", C.c_int32), ("total_launches", C.c_int32)]


class FcProf(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("total_ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double),
                ("launches", C.c_int32), ("reserved", C.c_int32)]


FC_PROF_CLASSES = 48


class FcLauraStack(C.Structure):
    _fields_ = [("idim", C.c_int32), ("d_model", C.c_int32), ("heads", C.c_int32), ("ff", C.c_int32), ("layers", C.c_int32),
                ("act", C.c_int32), ("embed_relu", C.c_int32), ("norm_style", C.c_int32)]


class FcLauraArch(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("input_size", C.c_int32), ("vocab_size", C.c_int32), ("codebook_size", C.c_int32),
                ("codebook_dim", C.c_int32), ("num_quantizers", C.c_int32), ("predict_nq", C.c_int32), ("pos_emb_split", C.c_int32),
                ("bidirectional_inputs", C.c_int32), ("max_positions", C.c_int32),
                ("text_encoder", FcLauraStack), ("codec_lm", FcLauraStack), ("codec_encoder", FcLauraStack)]


class FcSlotMeta(C.Structure):
    """fc_slot_meta: the host part of a slot record (phases: 0 idle, 1 running, 2 ended)"""
    _fields_ = [("layout", C.c_uint32), ("enc_phase", C.c_int32), ("dec_phase", C.c_int32), ("enc_frames", C.c_int32), ("dec_frames", C.c_int32)]


class FcLauraSampleRow(C.Structure):
    """fc_laura_sample_row: one row of the sampling table of fc_laura_sample's table form"""
    _fields_ = [("mode", C.c_int32), ("k", C.c_int32), ("p", C.c_float), ("max_steps", C.c_int32), ("seed", C.c_uint64),
                ("forced_on", C.c_int32), ("rng_row", C.c_uint32), ("temperature", C.c_float), ("min_length", C.c_int32),
                ("top_p", C.c_float), ("repeat_window", C.c_int32), ("repeat_count", C.c_int32)]


class FcLauraSampleIo(C.Structure):
    """fc_laura_sample_io: the buffers and parameters of fc_laura_sample"""
    _fields_ = [("logits", C.c_void_p), ("step", C.POINTER(C.c_int32)), ("n_gen", C.POINTER(C.c_int32)), ("done", C.POINTER(C.c_int32)),
                ("pos", C.POINTER(C.c_int32)), ("tok_off", C.POINTER(C.c_int32)), ("n_done", C.POINTER(C.c_int32)),
                ("tokens", C.c_void_p), ("forced", C.c_void_p), ("logp", C.c_void_p), ("score", C.c_void_p), ("next_emb", C.c_void_p),
                ("xs", C.c_void_p), ("rows", C.POINTER(FcLauraSampleRow)), ("B", C.c_int32), ("R", C.c_int32), ("mode", C.c_int32),
                ("k", C.c_int32), ("p", C.c_float), ("seed", C.c_uint64), ("max_steps", C.c_int32), ("row0", C.c_int32),
                ("nrows", C.c_int32)]


# every symbol include/funcodec_amd.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "fc_abi_version": (C.c_int, []),
    "fc_last_error": (C.c_char_p, []),
    "fc_engine_create": (C.c_int, [C.POINTER(FcArch), C.c_int, C.POINTER(_P)]),
    "fc_engine_destroy": (None, [_P]),
    "fc_engine_num_weights": (C.c_int, [_P]),
    "fc_engine_weight_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]),
    "fc_engine_set_weight": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int]),
    "fc_engine_finalize": (C.c_int, [_P]),
    "fc_engine_hop_length": (C.c_int, [_P]),
    "fc_engine_frames": (C.c_int, [_P, C.c_int]),
    "fc_engine_decoded_samples": (C.c_int, [_P, C.c_int]),
    "fc_engine_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int]),
    "fc_encode": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "fc_decode_emb": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_decode_codes": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "fc_encode_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    # length-aware (ragged) batches: the offline signatures plus the device lengths
    "fc_ragged_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int]),
    "fc_encode_ragged": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "fc_decode_emb_ragged": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_decode_codes_ragged": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "fc_encode_decode_ragged": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    # per-row stage counts of the calls that follow (host int32 [B], or None to clear)
    "fc_engine_set_row_nq": (C.c_int, [_P, _P, C.c_int, _P]),
    "fc_engine_set_rvq_beam": (C.c_int, [_P, C.c_int, _P]),
    "fc_rvq_encode_beam": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    # a stage count per row by target SNR: host float64 ratios [B] (None clears), min_nq, device outputs n_q_rows / row_errors / stage_errors
    "fc_engine_set_rate": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "fc_rvq_encode_rate": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    # the bit stream (csrc/code_pack_kernels.h): pitch and packet length (host arithmetic), pack and unpack on the device; engine-free
    "fc_code_packet_pitch": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "fc_code_packet_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "fc_codes_pack": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "fc_codes_unpack": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    # a stage count per frame (csrc/rvq_rate_kernels.h): frame mode of the rate (min_nq, device outputs n_q_frames / n_codes_rows /
    # achieved), and a borrowed device table [B][Tf] for the decode_codes calls
    "fc_engine_set_rate_frames": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "fc_engine_set_frame_nq": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    # a stage count per push of a session by a noise floor (the push rule of csrc/rvq_rate_kernels.h): host float64 floors [B] (None
    # clears), min_nq, the device count table [B]; then the form (chain, device outputs row_errors / stage_errors / sub_quants, host i32 [B] rows off)
    "fc_engine_set_floor": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "fc_engine_set_floor_form": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    # the same per frame of a push (the push frame rule): min_nq, the device count table [B][Tf of the push]; and a borrowed device table
    # [B][Tfc] for the decode_codes pushes of sessions
    "fc_engine_set_floor_frames": (C.c_int, [_P, C.c_int, _P, _P]),
    "fc_engine_set_push_frame_nq": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    # the bit stream's mode 1 (csrc/code_pack_kernels.h): a count per frame; engine-free
    "fc_frame_packet_pitch": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "fc_frame_packet_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_longlong, C.c_int]),
    "fc_frame_pack_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "fc_codes_pack_frames": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P, C.c_size_t, _P]),
    "fc_codes_unpack_frames": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "fc_rvq_encode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "fc_q0_source_frames": (C.c_int, [C.c_int, _P]),
    "fc_layer_forward": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_layer_forward_src": (C.c_int, [_P, C.c_char_p, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_layer_out_len": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "fc_layer2d_forward": (C.c_int, [_P, C.c_char_p, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_layer2d_out_shape": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "fc_freq_synthesis": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "fc_freq_synthesis_size": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fc_lstm_forward": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_seq_forward": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_resblock_forward": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_resblock_forward_src": (C.c_int, [_P, C.c_char_p, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_engine_work": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(FcWork)]),
    "fc_engine_profile": (C.c_int, [_P, C.c_int]),
    "fc_engine_profile_read": (C.c_int, [_P, C.POINTER(FcProf)]),
    "fc_debug_timeline": (C.c_int, [_P]),
    "fc_debug_conv_layout": (C.c_int, [C.c_int] * 7 + [_P, _P, C.c_size_t, _P, C.c_size_t]),
    "fc_debug_freq_features": (C.c_int, [_P, C.c_size_t, C.c_int]),
    "fc_codec_json_bound": (C.c_size_t, [C.c_int, C.c_int]),
    "fc_format_codec_json": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "fc_write_wav_pcm16": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int, C.c_int]),
    "fc_overlap_add": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "fc_engine_status": (C.c_int, [_P, C.POINTER(C.c_uint)]),
    # streaming session of a causal time-domain engine
    "fc_stream_state_bytes": (C.c_size_t, [_P, C.c_int]),
    "fc_stream_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(_P)]),
    "fc_stream_destroy": (None, [_P]),
    "fc_stream_min_first": (C.c_int, [_P, C.c_int]),
    "fc_stream_workspace_bytes": (C.c_size_t, [_P]),
    "fc_stream_reset": (C.c_int, [_P, _P, _P]),
    "fc_stream_encode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(C.c_int), _P, C.c_size_t, _P]),
    "fc_stream_decode_codes": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "fc_stream_decode_emb": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_stream_lstm_forward": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    # a streaming session of a causal transformer net: an fc_stream with a key / value cache of max_frames frames per side
    "fc_seqstream_state_bytes": (C.c_size_t, [_P, C.c_int, C.c_int]),
    "fc_seqstream_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(_P)]),
    "fc_seqstream_forward": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    # slot session: S slots that start, push and end independently in one batch (counts and flags: host int32 [S])
    "fc_slots_state_bytes": (C.c_size_t, [_P, C.c_int]),
    "fc_slots_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(_P)]),
    "fc_slots_destroy": (None, [_P]),
    "fc_slots_min_first": (C.c_int, [_P, C.c_int]),
    "fc_slots_workspace_bytes": (C.c_size_t, [_P]),
    "fc_slots_encode": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "fc_slots_decode_codes": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "fc_slots_decode_emb": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_slots_lstm_forward": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    # a slot session of a causal transformer net: an fc_slots with a key / value cache and a position per slot
    "fc_seqslots_state_bytes": (C.c_size_t, [_P, C.c_int, C.c_int]),
    "fc_seqslots_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(_P)]),
    "fc_seqslots_forward": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    # graph replay of a session's pushes (opt-in per session; counts: int64 [4] = replays, captures, evictions, fallbacks)
    "fc_graphstream_set": (C.c_int, [_P, C.c_int]),
    "fc_graphstream_enabled": (C.c_int, [_P]),
    "fc_graphstream_counts": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "fc_graphslots_set": (C.c_int, [_P, C.c_int]),
    "fc_graphslots_enabled": (C.c_int, [_P]),
    "fc_graphslots_counts": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    # the slot record (csrc/slots_kernels.h): export n running calls of a session, import them in another (slots host int32 [n], records
    # dev f32 [n][pitch], meta host fc_slot_meta [n]); _export_stream: rows of a lock-step session as slot records
    "fc_slotrec_floats": (C.c_size_t, [_P, C.c_int, C.c_int]),
    "fc_slotrec_export": (C.c_int, [_P, C.c_int, _P, _P, C.c_size_t, C.POINTER(FcSlotMeta), _P]),
    "fc_slotrec_import": (C.c_int, [_P, C.c_int, _P, _P, C.c_size_t, C.POINTER(FcSlotMeta), _P]),
    "fc_slotrec_export_stream": (C.c_int, [_P, C.c_int, _P, _P, C.c_size_t, C.POINTER(FcSlotMeta), _P]),
    # LauraTTS generation (ABI version 5)
    "fc_laura_create": (C.c_int, [C.POINTER(FcLauraArch), C.c_int, C.POINTER(_P)]),
    "fc_laura_destroy": (None, [_P]),
    "fc_laura_num_weights": (C.c_int, [_P]),
    "fc_laura_weight_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]),
    "fc_laura_set_weight": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int]),
    "fc_laura_finalize": (C.c_int, [_P]),
    "fc_laura_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fc_laura_encode": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_laura_lm_logprobs": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, _P, C.c_size_t, _P]),
    "fc_laura_decode_codec": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                        C.c_uint64, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "fc_laura_codec_emb": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_laura_linear": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_laura_debug_probe": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "fc_laura_attention": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "fc_laura_step_block": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "fc_laura_sample": (C.c_int, [_P, C.POINTER(FcLauraSampleIo), _P, C.c_size_t, _P]),
    "fc_laura_set_persistent_step": (C.c_int, [_P, C.c_int]),
    "fc_laura_persistent_step_fallbacks": (C.c_int, [_P]),
    # decoding session: S slots of decode_codec that start and end independently in one running batch
    "fc_laura_slots_state_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int]),
    "fc_laura_slots_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(_P)]),
    "fc_laura_slots_destroy": (None, [_P]),
    "fc_laura_slots_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int]),
    "fc_laura_slots_start": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, _P,
                                       _P, C.c_size_t, _P]),
    "fc_laura_slots_step": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "fc_laura_slots_take": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "fc_laura_slots_start_from": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, _P, _P]),
    "fc_laura_slots_fork": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, _P]),
    # a session that keeps the log-probability of every step's picks: one float per slot and step (terms: HOST float32 [cap])
    "fc_laura_slots_state_bytes_scored": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fc_laura_slots_create_scored": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(_P)]),
    "fc_laura_slots_score": (C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    # a slot's sampling rules (temperature, min_length, top_p, repeat_window, repeat_count): written by the next start / start_from / fork
    "fc_laura_slots_set_rules": (C.c_int, [_P, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int]),
    # n different prompts into n slots with one prefix pass (host arrays [n]: slots, lengths, per-row parameters)
    "fc_laura_slots_start_many_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int]),
    "fc_laura_slots_start_many": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    # start_from across two sessions of one engine (both driven on one stream)
    "fc_laura_slots_start_from_session": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, _P, _P]),
    # a session of up to 64 slots (the step's GEMV over column blocks of 16 rows); up to 16 it is the _scored pair
    "fc_laura_slots_state_bytes_wide": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fc_laura_slots_create_wide": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(_P)]),
    # a queued session: tickets wait on the device, ended slots retire into a result ring and free slots claim inside the captured step
    "fc_laura_slots_state_bytes_queued": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fc_laura_slots_create_queued": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, C.POINTER(_P)]),
    "fc_laura_slots_submit": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_float, C.c_int, C.c_float, C.c_int,
                                        C.c_int, C.POINTER(C.c_int32), _P]),
    "fc_laura_slots_queue_status": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64), _P]),
    "fc_laura_slots_collect": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int32)]),
    # an elastic session: a step as wide as the slots in use; slots moved to other rows in one launch
    "fc_laura_slots_set_elastic": (C.c_int, [_P, C.c_int]),
    "fc_laura_slots_step_blocks": (C.c_int, [_P]),
    "fc_laura_slots_move": (C.c_int, [_P, C.c_int, _P, _P, _P]),
}

_lib = None


def lib_path() -> str:
    # FC_LIB: tuning aid only (e.g. a profiling build made with FC_TIMELINE=1 next to the product library)
    return os.environ.get("FC_LIB") or _build.LIB_PATH


def load():
    """Load libfuncodec_amd.so (built in-tree).  There is no fallback: if the HIP library cannot be
    loaded the product path raises."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own HIP runtime (torch/lib/libamdhip64.so); it must be in the process BEFORE this
    # library is loaded so that both share ONE runtime -- two HIP runtimes in one process cannot both
    # see the device ("no HIP device visible").
    import torch  # noqa: F401
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -m funcodec_amd.build` (hipcc, gfx950). "
            "funcodec_amd has no CPU or PyTorch fallback path.")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError = ABI drift, loudly
        fn.restype = res
        fn.argtypes = args
    if lib.fc_abi_version() != FC_ABI_VERSION:
        raise RuntimeError("libfuncodec_amd.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def last_error() -> str:
    return load().fc_last_error().decode("utf-8", "replace")
