/*
 * funcodec_amd.h -- C ABI of the MI355X (gfx950) FunCodec encode/decode engine.
 *
 * The reference (modelscope/FunCodec, /root/reference) is 100 % Python on top of torch.nn; it has no
 * FFI layer.  Its operator boundary for this path is the set of Python callables listed next to each
 * entry point below; a maintainer binds this library with ctypes from
 * `funcodec/bin/codec_inference.py` (Speech2Token.__call__, :86-134).
 *
 * Conventions
 *   - plain C types only; every pointer argument marked "dev" is a DEVICE pointer (HBM) owned by the
 *     caller (e.g. `tensor.data_ptr()`), "host" pointers are ordinary host memory;
 *   - all tensors are dense, row-major, fp32 unless stated; code indices are int64 like the reference;
 *   - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it (no host sync);
 *   - return value: 0 = ok, non-zero = error, message via fc_last_error() (thread-local);
 *   - one engine per (device, checkpoint); calls on one engine must be serialised by the caller;
 *   - the engine never falls back to a CPU path: without a gfx950 device every compute call fails.
 */
#ifndef FUNCODEC_AMD_H
#define FUNCODEC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FC_MAX_RATIOS 8
#define FC_ABI_VERSION 7     /* layout of fc_arch / fc_laura_arch.  7: fc_arch.seq_model / seq_heads / seq_ff appended (the transformer
                              * bottleneck, seq_model: transformer) and fc_seq_forward added.
                              * 6 (round 4): fc_arch.q0_ds_ratio appended; fc_arch.input_channels = 2 with
                              * model_type 0 is the stereo time-domain codec.  (Round 4 also added entry points that changed no struct:
                              * fc_laura_set_persistent_step, fc_debug_freq_features, fc_q0_source_frames.) */

typedef struct fc_engine fc_engine;

/* Architecture, i.e. the subset of config.yaml the hot path depends on.
 * Replaces: GANSpeechCodecTask.build_model (funcodec/tasks/gan_speech_codec.py:300-343) +
 * SEANetEncoder.__init__ (funcodec/models/encoder/seanet_encoder.py:88-160) +
 * SEANetDecoder.__init__ (funcodec/models/decoder/seanet_decoder.py:88-164) +
 * CostumeQuantizer.__init__ (funcodec/models/quantizer/costume_quantizer.py:7-55). */
typedef struct fc_arch {
    int32_t abi_version;            /* FC_ABI_VERSION */
    int32_t sample_rate;
    int32_t audio_normalize;        /* model_conf.audio_normalize */
    int32_t n_filters;              /* 32 */
    int32_t dimension;              /* 128: encoder output / codebook dim */
    int32_t n_ratios;
    int32_t ratios[FC_MAX_RATIOS];  /* decoder order, e.g. {8,5,4,2,2}; encoder walks it reversed */
    int32_t kernel_size;            /* 7 */
    int32_t last_kernel_size;       /* 7 */
    int32_t residual_kernel_size;   /* 3 */
    int32_t compress;               /* 2 */
    int32_t lstm_layers;            /* 2 (0 = no sequence model) */
    int32_t lstm_skip;              /* res_seq */
    float   elu_alpha;              /* 1.0 */
    float   gn_eps;                 /* 1e-5 */
    int32_t codebook_size;          /* 1024 */
    int32_t num_quantizers;         /* 32 */
    /* conv wrapper flavour (funcodec/modules/normed_modules/conv.py:20-56,205-305), ABI version 2: */
    int32_t norm_type;              /* 0 = GroupNorm(1,C) after every conv ("time_group_norm"); 1 = weight_norm (checkpoint holds
                                       weight_g / weight_v, no output norm); 2 = none (plain weight, no output norm) */
    int32_t causal;                 /* 1: all conv padding on the left, transposed convs trimmed on the right only */
    int32_t n_residual_layers;      /* residual blocks per stage (1 in the encodec recipes, 3 in the SoundStream recipe) */
    int32_t dilation_base;          /* block j of a stage dilates its k=3 conv by dilation_base**j (seanet_encoder.py:127-133) */
    /* ABI version 4: the STFT-domain codec (FreqCodec, funcodec/models/codec_freq.py:123-210; SEANetEncoder2d / SEANetDecoder2d,
     * funcodec/models/encoder/seanet_encoder.py:252-363, decoder/seanet_decoder.py:244-360).  model_type 0 ignores the rest except input_channels. */
    int32_t model_type;             /* 0 = encodec (time domain), 1 = freq_codec (codec_domain [mag_phase, mag_phase] or [mag_angle, mag_angle]) */
    int32_t input_channels;         /* model_type 0: audio channels, 1 (0 reads as 1) or 2 = stereo (config input_size / decoder_conf.channels;
                                     * codec_basic.py:342-344,366: the volume scale is taken from the channel mean); wav buffers are [B][C][T].
                                     * model_type 1: encoder input / decoder output channels of the 2-D nets, which also names the codec_domain like the
                                     * reference's input_size does (codec_freq.py:356-379): 3 = mag_phase (log-magnitude, phase re, phase im),
                                     * 2 = mag_angle (log-magnitude, torch.angle) */
    int32_t n_fft;                  /* 512  (model_conf.domain_conf.n_fft) */
    int32_t stft_hop;               /* 160  (model_conf.domain_conf.hop_length) */
    int32_t ratios_f[FC_MAX_RATIOS];/* frequency ratios of the 2-D stages, decoder order (ratios[] holds the time ratios) */
    /* grouped 2-D convs (seanet_encoder.py:224,234,321; seanet_decoder.py:219,229,324): <= 0 = dense (the recipe), else the layer has
     * groups = min(in, out) / 2 / ratio (res-block convs), channels / 2 / ratio (shortcut, strided / transposed convs) */
    int32_t enc_conv_group_ratio;   /* encoder_conf.conv_group_ratio */
    int32_t dec_conv_group_ratio;   /* decoder_conf.conv_group_ratio */
    int32_t dec_tr_conv_group_ratio;/* decoder_conf.tr_conv_group_ratio */
    /* ABI version 5: CostumeQuantizer's optional projection / range (funcodec/models/quantizer/costume_quantizer.py:23-35,63-73,84-87) */
    int32_t codec_dim;              /* quantizer_conf.codec_dim: 0 (or = dimension) = none; else the codebooks live in codec_dim dims behind
                                       input_proj / output_proj Linears (checkpoint keys quantizer.input_proj.*, quantizer.output_proj.*) */
    float   codec_range;            /* quantizer_conf.codec_range: 0 = none; else the quantiser input is tanh(x) * codec_range */
    /* ABI version 6 */
    int32_t q0_ds_ratio;            /* quantizer_conf.q0_ds_ratio (funcodec/modules/quantization/ddp_core_vq.py:354-356,396-404): <= 1 = off;
                                       > 1: the FIRST quantiser stage sees the nearest-neighbour half-rate sequence (the reference halves
                                       whatever the value is) and its output / indices are repeated back to Tf frames */
    /* ABI version 7: the sequence model at the bottleneck (encoder_conf / decoder_conf seq_model; seanet_encoder.py:142-151,328-337,
     * seanet_decoder.py:116-125,297-306).  lstm_layers counts its layers / blocks and lstm_skip is its res_seq in both cases. */
    int32_t seq_model;              /* 0 = SLSTM with lstm_layers layers; 1 = TransformerEncoder (normed_modules/transformer.py:26-208) with
                                       lstm_layers pre-LayerNorm blocks, no positional encoding, causal when `causal` is set; the bottleneck
                                       width C = n_filters << n_ratios must be 64, 128, 256, 512 or 1024 (head size C / seq_heads in 16..256) */
    int32_t seq_heads;              /* attention heads of the transformer (4, the TransformerEncoder default) */
    int32_t seq_ff;                 /* feed-forward units of the transformer (2048, linear_units default) */
} fc_arch;

/* ---- lifetime ------------------------------------------------------------------------------------ */
int  fc_abi_version(void);
const char* fc_last_error(void);

/* Replaces build_model(): builds the layer plan; allocates nothing on the device yet. */
int  fc_engine_create(const fc_arch* arch, int device, fc_engine** out);
void fc_engine_destroy(fc_engine* e);

/* Checkpoint contract.  Replaces build_model_from_file / filter_state_dict
 * (funcodec/tasks/abs_task.py:1895-1947, funcodec/torch_utils/load_pretrained_model.py:12-43):
 * the host enumerates the state_dict keys the engine wants and hands each tensor over by name. */
int  fc_engine_num_weights(const fc_engine* e);
/* name/dims of expected tensor i (dims has room for 4 entries); returns ndim or <0. */
int  fc_engine_weight_info(const fc_engine* e, int i, const char** name, int64_t* dims);
/* host fp32 tensor in the reference's own layout (e.g. Conv1d [Cout,Cin,k], ConvTranspose1d [Cin,Cout,k],
 * LSTM weight_ih_l0 [4H,H], quantizer.rq.model.embed [n_q,K,D]).  Unknown names -> error code 2
 * (the host skips discriminator.* etc. itself).  Shape mismatch -> error. */
int  fc_engine_set_weight(fc_engine* e, const char* name, const float* host, const int64_t* dims, int ndim);
/* Folds / re-lays-out the weights into HBM.  Fails if a tensor is missing. */
int  fc_engine_finalize(fc_engine* e);

/* ---- sizes --------------------------------------------------------------------------------------- */
int    fc_engine_hop_length(const fc_engine* e);
/* frames emitted for n_samples: ceil at every encoder stride (SConv1d extra padding, conv.py:57-64). */
int    fc_engine_frames(const fc_engine* e, int n_samples);
/* samples the decoder emits for n_frames frames: n_frames * hop for the time-domain codec; stft_hop * (frames * time ratios - 1) for
 * the STFT-domain codec (torch.istft with center=True).  Upper bound of `out_len` of the decode entry points. */
int    fc_engine_decoded_samples(const fc_engine* e, int n_frames);
/* bytes of caller-provided device scratch needed by any call with batch B and T samples (or Tf*hop).  The figure INCLUDES 4 KiB of tail
 * slack that every entry point requires behind its last internal buffer (kernels with unclamped row-end loads and the DMA-staged conv
 * read a few bytes past a buffer's end): a workspace that ends exactly at the last buffer is refused ("workspace too small"), never
 * over-read.  The workspace pointer itself must be 256-byte aligned device memory. */
size_t fc_engine_workspace_bytes(const fc_engine* e, int B, int T);

/* ---- the hot path -------------------------------------------------------------------------------- */
/* Encodec.inference_encoding (funcodec/models/codec_basic.py:720-764) = _encode_frame (:361-380) +
 * SEANetEncoder.forward + CostumeQuantizer.inference -> DRVQ.forward (ddp_core_vq.py:367-418).
 *   wav        dev f32 [B,T]       ([B,2,T] for a stereo model, fc_arch.input_channels = 2 with model_type 0; B and T keep their meaning)
 *   n_q        number of quantizers to run (1..num_quantizers)
 *   codes      dev i64 [n_q,B,Tf]                         (code_indices[0])
 *   quantized  dev f32 [B,Tf,D]   or NULL                 (code_embeddings[0][0])
 *   sub_quants dev f32 [n_q,B,D,Tf] or NULL               (sub_quants[0])
 *   scale      dev f32 [B]        or NULL (1e-8+rms; written only if audio_normalize)
 *   enc_out    dev f32 [B,Tf,D]   or NULL (encoder output before quantisation) */
int fc_encode(fc_engine* e, const float* wav, int B, int T, int n_q,
              int64_t* codes, float* quantized, float* sub_quants, float* scale, float* enc_out,
              void* workspace, size_t workspace_bytes, void* stream);

/* Encodec.inference_decoding_emb (codec_basic.py:804-836) = _decode_frame (:398-408) + SEANetDecoder.forward.
 *   emb   dev f32 [B,Tf,D];  scale dev f32 [B] or NULL (multiplied in when non-NULL, :406-407)
 *   wav   dev f32 [B,out_len] ([B,2,out_len] for a stereo model), out_len <= fc_engine_decoded_samples(Tf) (the first out_len samples
 *         of every channel are written) */
int fc_decode_emb(fc_engine* e, const float* emb, const float* scale, int B, int Tf, int out_len,
                  float* wav, void* workspace, size_t workspace_bytes, void* stream);

/* Encodec.inference_decoding (codec_basic.py:766-802): DRVQ.decode (ddp_core_vq.py:442-453) + decoder.
 *   codes dev i64 [B,Tf,n_q] (the reference's token layout);  emb_out dev f32 [B,Tf,D] or NULL */
int fc_decode_codes(fc_engine* e, const int64_t* codes, int B, int Tf, int n_q, int out_len,
                    float* wav, float* emb_out, void* workspace, size_t workspace_bytes, void* stream);

/* Encodec.inference (codec_basic.py:670-718) / FreqCodec.inference (codec_freq.py): encode + decode in one enqueue;
 * recon [B, min(T, fc_engine_decoded_samples(frames))] (= the reference's recon[:, :, :T]; always T for model_type 0; [B,2,T] for a
 * stereo model). */
int fc_encode_decode(fc_engine* e, const float* wav, int B, int T, int n_q, int use_scale,
                     int64_t* codes, float* quantized, float* sub_quants, float* scale, float* recon,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- length-aware (ragged) batches ----------------------------------------------------------------
 * (entry points added without a struct change: FC_ABI_VERSION stays 7)
 * A batch [B,Tmax] whose rows have lengths of their own.  `lengths` dev i32 [B], 1 <= lengths[b] <= Tmax (samples for the encode calls,
 * frames for the decode calls).  Row b of every output equals what the offline callable named below returns for row b ALONE cut at its
 * length: its volume scale, the GroupNorm statistics of every conv, the reflection padding at its end and the extra_padding of every
 * strided conv are the row's own.  Row b has fc_engine_frames(lengths[b]) valid frames and lengths[b] (decode: frames * hop) valid samples;
 * everything behind a row's valid part is written as zero.  A row's valid outputs depend on nothing outside that row: not on the other rows,
 * not on Tmax, not on what lies behind lengths[b] in the caller's buffers (it is never read).  The output shapes are those of the offline
 * sibling for (B, Tmax).
 * Time-domain codec only; refused with the configuration key named: model freq_codec, seq_model: transformer,
 * quantizer_conf.q0_ds_ratio > 1 (fc_ragged_workspace_bytes returns 0 for these).  A length outside [1, Tmax] is clamped on the device and
 * reported like an out-of-range code: by the next compute call or fc_engine_status (FC_STATUS_FLAG_BAD_LENGTH). */
/* workspace of any ragged call with batch B and Tmax samples (or frames * hop); includes the 4 KiB tail slack like fc_engine_workspace_bytes */
size_t fc_ragged_workspace_bytes(const fc_engine* e, int B, int Tmax);
/* Encodec.inference_encoding (codec_basic.py:720-764) on wav[b, ..., :lengths[b]], per row; arguments as fc_encode */
int fc_encode_ragged(fc_engine* e, const float* wav, const int32_t* lengths /* dev [B] */, int B, int T, int n_q,
                     int64_t* codes, float* quantized, float* sub_quants, float* scale, float* enc_out,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Encodec.inference_decoding_emb (codec_basic.py:804-836) on emb[b, :lengths[b]], per row; arguments as fc_decode_emb */
int fc_decode_emb_ragged(fc_engine* e, const float* emb, const float* scale, const int32_t* lengths /* dev [B], frames */, int B, int Tf,
                         int out_len, float* wav, void* workspace, size_t workspace_bytes, void* stream);
/* Encodec.inference_decoding (codec_basic.py:766-802) on codes[b, :lengths[b]], per row; arguments as fc_decode_codes.  Tokens behind a
 * row's frames are not looked up (and never reported as out of range) */
int fc_decode_codes_ragged(fc_engine* e, const int64_t* codes, const int32_t* lengths /* dev [B], frames */, int B, int Tf, int n_q,
                           int out_len, float* wav, float* emb_out, void* workspace, size_t workspace_bytes, void* stream);
/* Encodec.inference (codec_basic.py:670-718) on wav[b, ..., :lengths[b]], per row; arguments as fc_encode_decode; recon [B,T] */
int fc_encode_decode_ragged(fc_engine* e, const float* wav, const int32_t* lengths /* dev [B] */, int B, int T, int n_q, int use_scale,
                            int64_t* codes, float* quantized, float* sub_quants, float* scale, float* recon,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- a bit rate per row ----------------------------------------------------------------------------
 * (an entry point added without a struct change: FC_ABI_VERSION stays 7)
 * A residual quantiser is a prefix code: stage i depends on the stages before it only, and nothing is carried from frame to frame.  So
 * every row of a batch, a streaming session or a slot session may run its own number of stages, and change it from one call to the next.
 *   n_q_rows   HOST i32 [B], each in [1, num_quantizers]: the stage counts of the calls that FOLLOW on this engine; NULL clears them
 *              (B is then ignored).  The engine keeps them in a small device table of its own; the copy is ordered on `stream`, the
 *              caller's array may go when the call returns.
 * While a table is set, every call that quantises or looks up codes -- fc_encode, fc_encode_decode, fc_decode_codes, their _ragged
 * siblings, the encode and decode_codes pushes of both session kinds, and the per-op hook for the quantiser -- must have batch width (or
 * slot count) B, and its n_q argument (a session's: the n_q of create) is the CAP: the first dimension of its codes, >= every entry.  A call
 * that breaks either rule is refused before its first launch and changes nothing.  The table is indexed by batch row (in a slot push: by
 * slot; the count of an idle slot is ignored).  Row b with count k:
 *   - codes[:k], and the quantised embeddings, their decoder input and the reconstruction, are bit for bit what the same call with
 *     n_q = k gives that row; codes[k:] and sub_quants[k:] of the row are 0 (behind a row's length of a ragged call: as ever);
 *   - a decode call sums the row's first k code vectors and does not read its codes[.., k:]: whatever they hold changes nothing and is
 *     never reported as out of range.
 * In the per-op hook the N rows are B utterances of N / B frames each (N a multiple of B).
 * The calls that take embeddings are not concerned.  With no table set every call launches exactly what it launched before.
 * Segmented mode (model_conf.segment_dur: segments are extra batch rows) and model_conf.bypass_quantizer are host-side matters -- fc_arch
 * has neither field -- so only the host wrappers can refuse them, and do. */
int fc_engine_set_row_nq(fc_engine* e, const int32_t* n_q_rows /* host [B] or NULL */, int B, void* stream);

/* ---- the quantiser's search over the stages (entry points added without a struct change: FC_ABI_VERSION stays) --------------
 * The reference's residual quantiser is greedy: stage i takes the nearest code to the residual and never looks back.  A width W in
 * {2, 4, 8} keeps W hypotheses per frame through the stages instead (csrc/rvq_beam_kernels.h states the search); the bit stream, the
 * decoder and every consumer of codes stay as they are.  Slot 0 is always the greedy path and the pick is by the explicitly recomputed
 * residual energy, ties to the lowest slot, so a frame is never coded worse than greedy under that formula; the greedy codes themselves
 * are computed by the same launch as ever.  Everything a call returns besides the codes (quantised embeddings, sub_quants, the
 * decoder's input, the reconstruction) is made from the final codes: `quantized` is bit for bit fc_decode_codes' emb_out of them.
 * The search is per frame: nothing is carried between frames, rows, pushes or batch neighbours.
 * fc_engine_set_rvq_beam sets the width for the calls that follow, as fc_engine_set_row_nq sets stage counts; 1 clears it.  Every call
 * that quantises honours it: fc_encode, fc_encode_decode, their _ragged siblings, the encode pushes of both session kinds (the width
 * is part of a captured push's key) and the 2-D (FreqCodec) encode.  With width 1 every call launches exactly what it launched before.
 * With per-row stage counts a row with count k runs the search over k stages, which is NOT a prefix of the search over more.
 * Refused before any launch, changing nothing: a width outside {1, 2, 4, 8} (names rvq_beam); quantizer_conf.q0_ds_ratio > 1 with a
 * width above 1 (stage 0 is shared by frame pairs there).  model_conf.bypass_quantizer is a host-side matter: the host wrappers refuse. */
int fc_engine_set_rvq_beam(fc_engine* e, int width, void* stream);
/* The per-op hook: x dev f32 [N,D]; codes dev i64 [n_q,N]; quantized dev f32 [N,D] or NULL; paths dev i64 [width,n_q,N] or NULL and
 * errors dev f32 [width,N] or NULL: every slot's final path and its fixed-order residual energy (both NULL with width 1).  Honours
 * fc_engine_set_row_nq as fc_rvq_encode does; ignores the width set on the engine. */
int fc_rvq_encode_beam(fc_engine* e, const float* x, int N, int n_q, int width, int64_t* codes, float* quantized, int64_t* paths,
                       float* errors, void* stream);

/* ---- a stage count per row chosen on the device by target SNR (entry points added without a struct change: FC_ABI_VERSION stays) ----
 * Each row of an offline call takes the smallest number of stages whose quantiser-domain SNR reaches its target, inside the one call:
 * nothing is read back, the chosen counts are an output on the device.  csrc/rvq_rate_kernels.h states the rule and
 * funcodec_amd/engine.py::rate_pick restates it on the host.  With x [N = B Tf, Dc] the quantiser's input rows and c [n_q, N] the codes
 * the call finds at the cap (greedy, or the search of fc_engine_set_rvq_beam at its full depth):
 *   stage errors [n_q + 1][B][Tf] f32:  r_0 = x[n], r_{i+1} = r_i - E_i[c_i[n]] element-wise in fp32, err[i][n] = |r_i|^2 in one fixed
 *       order (four chains over Dc / 4, squares rounded separately, (p0 + p1) + (p2 + p3)); err[0] is the input energy.  Made from the
 *       codes, whoever found them.  0 behind a row's cap and behind a row's frames of a ragged call;
 *   row errors [B][n_q + 1] f64:  E_b[i] = the sum of err[i][b, t] over the row's frames (a ragged call: its own fc_engine_frames(len_b)
 *       only), in an order that depends on the row's frame count alone -- never on B, Tmax or the neighbours;
 *   the pick:  rho_b = 10^(-target_b / 10), computed by the host in double and handed over as a double; the floor min_nq; the cap cap_b
 *       (the row's entry of fc_engine_set_row_nq if a table is set, else the call's n_q).  k_b = the smallest k in [min_nq, cap_b] with
 *       E_b[k] <= E_b[0] * rho_b.  If no k reaches the target: the k in that range with the smallest E_b[k], first on ties (the curve is
 *       not monotone on real codebooks: a missed target never costs more bits for a worse result; rho = 0 therefore means "the best k").
 *       A row with E_b[0] == 0 (digital silence) takes min_nq.  A row whose energies are not all finite takes cap_b, as the plain call would.
 * Row b of codes, quantized, sub_quants, the decoder's input and the reconstruction is then what the call with fc_engine_set_row_nq
 * count k_b returns: zeros in codes[k_b:] and sub_quants[k_b:].  Greedy: bit for bit that call.  With a search: the first k_b codes of
 * the full-depth path, which is NOT the search over k_b stages; quantized is fc_decode_codes' sum of those codes.  A decoder needs the
 * count (code 0 is a valid code): hand n_q_rows to fc_engine_set_row_nq for the decode call.
 *   ratio_rows        HOST f64 [B]; NULL clears the rate (the other arguments are then ignored).  The engine keeps a device copy of its own;
 *                     the copy is ordered on `stream`, the caller's array may go when the call returns
 *   n_q_rows_out      dev i32 [B]: the chosen counts (required)
 *   row_errors_out    dev f64 [B][n_q + 1] or NULL;  stage_errors_out  dev f32 [n_q + 1][B * Tf] or NULL: with n_q and Tf those of the call
 *                     that follows; the call's workspace holds whichever is NULL (fc_engine_workspace_bytes counts them)
 * It applies to the calls that follow, like fc_engine_set_row_nq, and is honoured by fc_encode, fc_encode_decode, their _ragged siblings
 * (the 2-D FreqCodec encode included) and the per-op hook fc_rvq_encode_rate.  With no rate set every call launches exactly what it
 * launched before.  Refused before the first launch, changing nothing: B other than the call's batch width; min_nq outside
 * [1, num_quantizers], above the call's n_q or above a row's cap; a ratio that is negative or NaN; quantizer_conf.q0_ds_ratio > 1 (stage 0
 * quantises another frame's row); any encode push of a stream or slot session while a rate is set (offline calls only).
 * model_conf.segment_dur and model_conf.bypass_quantizer are host-side matters: the host wrappers refuse. */
int fc_engine_set_rate(fc_engine* e, const double* ratio_rows /* host [B] or NULL */, int B, int min_nq, int32_t* n_q_rows_out /* dev [B] */,
                       double* row_errors_out /* dev [B][n_q+1] or NULL */, float* stage_errors_out /* dev [n_q+1][B*Tf] or NULL */, void* stream);
/* The per-op hook under the rate set on the engine (both optional outputs of fc_engine_set_rate must be given: the hook has no
 * workspace): x dev f32 [N,D], the N rows being B utterances of N / B frames; width 1 (greedy) or 2, 4, 8 (the search at full depth);
 * codes dev i64 [n_q,N]; quantized dev f32 [N,D] or NULL.  Honours fc_engine_set_row_nq as the caps. */
int fc_rvq_encode_rate(fc_engine* e, const float* x, int N, int n_q, int width, int64_t* codes, float* quantized, void* stream);

/* ---- a stage count per FRAME by target SNR (entry points added without a struct change: FC_ABI_VERSION stays 7) ----
 * csrc/rvq_rate_kernels.h states the frame rule and funcodec_amd/engine.py::rate_pick_frames restates it on the host: with the stage
 * errors and the fp64 row sums above, thr_b = E_b[0] * rho_b, and frame t of row b takes the smallest k in [min_nq, cap_b] with
 * (double)err[k][b,t] * (double)F_b <= thr_b (F_b: the row's own frame count), else the k with the smallest err[k][b,t], first on ties;
 * a row that is not finite takes cap_b in every frame, a silent row min_nq; frames behind a row's frames take 0.  Every frame is
 * quantised down to the row's constant noise floor thr_b / F_b (reverse water-filling).  Frame (b,t) of codes, quantized, sub_quants, the
 * decoder's input and the reconstruction is what the call with n_q = k_t gives that frame (greedy: bit for bit; with a search: the first
 * k_t codes of the full-depth path); codes[k_t:] and sub_quants[k_t:] of the frame are 0, and a frame with k_t = 0 has quantized 0. */
/* By the frame rule of csrc/rvq_rate_kernels.h: given AFTER fc_engine_set_rate, it turns the rate set there into frame mode for the
 * offline calls that follow (fc_encode, fc_encode_decode, their _ragged siblings, the 2-D FreqCodec encode, fc_rvq_encode_rate); cleared
 * with the rate (NULL ratios), and by every new fc_engine_set_rate.  min_nq in [0, num_quantizers] replaces the floor given there: a
 * frame may take no stage.  n_q_rows_out of fc_engine_set_rate then receives every row's LARGEST frame count.
 *   n_q_frames_out     dev i32 [B][Tf] (required, so no workspace size changes)
 *   n_codes_rows_out   dev i32 [B] or NULL: the sum of the row's frame counts
 *   achieved_out       dev f64 [B] or NULL: the sum over the row's frames of err[k_t][b,t], in the order E_b is summed
 * Refused before anything changes: no rate set, min_nq outside [0, num_quantizers], a null n_q_frames_out.  Every session push is refused
 * by name while it is set, as for the row rate. */
int fc_engine_set_rate_frames(fc_engine* e, int min_nq, int32_t* n_q_frames_out /* dev [B][Tf] */, int32_t* n_codes_rows_out /* dev [B] or NULL */,
                              double* achieved_out /* dev [B] or NULL */, void* stream);
/* By the count of csrc/rvq_rate_kernels.h (a count per frame): a stage count per frame for the fc_decode_codes and
 * fc_decode_codes_ragged calls that follow; frame (b,t) sums its first n_q_frames[b][t] codes (clamped to [0, n_q]); the codes behind a
 * frame's count are not read and never raise FC_STATUS_BAD_CODE.  The pointer is BORROWED: it is read by the launches of those calls and
 * must stay valid until they have run; NULL clears the table.  Refused: together with a row table (fc_engine_set_row_nq); a decode call
 * of another B or Tf, before its first launch; every decode push of a stream or slot session while a table is set. */
int fc_engine_set_frame_nq(fc_engine* e, const int32_t* n_q_frames /* DEV i32 [B][Tf] or NULL */, int B, int Tf, void* stream);

/* ---- a stage count per PUSH of a session, by a noise floor (entry points added without a struct change: FC_ABI_VERSION stays 7) ----
 * By the push rule of csrc/rvq_rate_kernels.h ("THE PUSH RULE"): every row of the encode pushes of both session kinds that follow
 * (fc_stream_encode, fc_slots_encode, sessions made by fc_seqstream_create / fc_seqslots_create included) takes the smallest stage count
 * in [min_nq, its cap] whose residual energy over the row's frames OF THAT PUSH lies at or below floor_b * frames_b; a row already at or
 * below its floor takes min_nq; a missed floor takes the best count; a row without a frame in the push (an idle slot) is neither read nor
 * written.  floor_rows [B] (host, copied): floor_b = D * 10^(noise_floor_db_b / 10), D the quantiser's input width, neither negative nor
 * NaN; +inf is "always min_nq", 0 "the best count".  The cap of row b is its entry of fc_engine_set_row_nq, else the session's n_q; the
 * width of fc_engine_set_rvq_beam composes (a row then keeps the first k_b codes of the full-depth path).  The rule is stateless: a
 * count depends on the row's frames of the push alone.  Row b of codes, quantized and enc_out is what the same push with a row count of
 * k_b gives (greedy: bit for bit, zeros in codes[k_b:]).  n_q_rows_out [B] (device, the caller's, valid until the floor is cleared)
 * receives k_b; fc_codes_pack reads it as it is.  A push of at most 256 frames per row adds ONE launch to the push; a wider one runs
 * four (the same device steps, the same bits).  Every launch reads frames, caps and floors from device memory, so a captured push
 * (fc_graphstream_set, fc_graphslots_set) replays without a new capture when the floors change.  NULL floors clear it; with no floor
 * set every call and push launches exactly what it launched before.
 * It also applies to the per-op hook fc_rvq_encode_rate, on B rows of N / B frames (fc_engine_set_floor_form then gives the hook's outputs).
 * Refused, before the first launch and changing nothing: an offline encode call while a floor is set (session pushes only); a floor
 * together with a rate (fc_engine_set_rate), by either setter; a push of another B; min_nq outside [1, num_quantizers], above the
 * session's n_q or above a row's cap; a NaN or negative floor; quantizer_conf.q0_ds_ratio > 1. */
int fc_engine_set_floor(fc_engine* e, const double* floor_rows /* host [B] or NULL */, int B, int min_nq, int32_t* n_q_rows_out /* dev [B] */,
                        void* stream);
/* Given AFTER fc_engine_set_floor; cleared with it and by every new fc_engine_set_floor.  chain != 0: the four-launch form at every
 * width (a measurement and test aid: same bits).  row_errors_out (dev f64 [B][n_q + 1]) and stage_errors_out (dev f32 [n_q + 1][B Tf]):
 * optional outputs of the pushes that follow; the hook fc_rvq_encode_rate needs both (it has no workspace of its own).  sub_quants_out
 * (dev f32 [n_q][B][D][Tf], optional): E_i[c_i] of every stage, 0 behind a row's count, from the hook alone.  off_rows (host
 * i32 [B] or NULL): a row with a non-zero entry is switched off -- it takes its cap, as without a floor, and n_q_rows_out receives that
 * (a slot without a floor beside slots that have one; device data, like the floors). */
int fc_engine_set_floor_form(fc_engine* e, int chain, double* row_errors_out, float* stage_errors_out, float* sub_quants_out,
                             const int32_t* off_rows /* host [B] or NULL */, void* stream);

/* ---- a stage count per FRAME of a session push, by a noise floor (entry points added without a struct change: FC_ABI_VERSION stays 7) ----
 * By the push frame rule of csrc/rvq_rate_kernels.h ("THE PUSH FRAME RULE"; funcodec_amd/engine.py::floor_pick_frames restates it on the
 * host): given AFTER fc_engine_set_floor, it turns the floor set there into frame mode for the encode pushes of both session kinds and
 * for the per-op hook fc_rvq_encode_rate; cleared with the floor (NULL floors), and by every new fc_engine_set_floor.  Frame t of row b
 * takes the smallest k in [min_nq, cap_b] with (double)err[k][b,t] <= floor_b -- comparisons only; a frame already at or below the floor
 * takes min_nq; a missed floor takes the frame's best k, first on ties; a frame that is not finite, and every frame of a row switched
 * off, takes cap_b; frames behind a row's frames in the push take 0; an idle row's counts are left unwritten.  min_nq in
 * [0, num_quantizers] replaces the one given to fc_engine_set_floor: a frame may take no stage.  A frame's count depends on that frame's
 * quantiser input alone, not on how the audio is cut into pushes.  Frame (b,t) of codes and quantized is what the same push with
 * n_q = k_t gives it (greedy: bit for bit, zeros in codes[k_t:]; with a search: the first k_t codes of the full-depth path).
 *   n_q_frames_out   dev i32 [B][Tf of the push], dense, required; n_q_rows_out of fc_engine_set_floor is then NOT written
 * ONE launch at every width (a workgroup per 16 frames of a row), or four with fc_engine_set_floor_form(chain = 1): the same bits on every
 * row that has frames.  row_errors_out of fc_engine_set_floor_form is not written in frame mode (there are no row sums); the hook needs
 * stage_errors_out alone.  A captured push is keyed by the table's address, min_nq and the mode, never by a floor.
 * Refused before anything changes: no floor set, min_nq outside [0, num_quantizers] or above a row's cap, a null n_q_frames_out. */
int fc_engine_set_floor_frames(fc_engine* e, int min_nq, int32_t* n_q_frames_out /* dev [B][Tf] */, void* stream);
/* By the count of csrc/rvq_rate_kernels.h (a count per frame): fc_engine_set_frame_nq for the decode pushes of sessions that follow
 * (fc_stream_decode_codes, fc_slots_decode_codes): frame (b,t) of the push sums its first n_q_frames[b][t] codes (clamped to [0, n_q]; 0
 * behind a slot's frames in the push).  The pointer is BORROWED; NULL clears the table.  Part of a captured push's key.  Refused:
 * together with a row table (fc_engine_set_row_nq); a decode push of another B or Tfc, before its first launch; every offline decode
 * call while it is set. */
int fc_engine_set_push_frame_nq(fc_engine* e, const int32_t* n_q_frames /* DEV i32 [B][Tfc] or NULL */, int B, int Tfc, void* stream);

/* ---- the bit stream: one self-describing packet per row (entry points added without a struct change: FC_ABI_VERSION stays 7) ----
 * csrc/code_pack_kernels.h states the packet rule (8-byte little-endian header: u32 frames, u8 k, u8 bits, u8 mode = 0, u8 0; payload
 * value t * k + i = codes[i][b][t] in `bits` bits each, LSB first, pad bits 0) and the device row (pitch = the largest packet rounded up
 * to 16, zeros behind the packet); funcodec_amd/io.py restates it on the host.  None of the four calls needs an engine.
 * There is no fused "decode from packets" call: decoding is fc_codes_unpack, then fc_engine_set_row_nq with the counts of the headers
 * (the host holds the bytes and therefore the headers), then the decode calls.  A call that asks for no packets launches what it did.
 * Not built: entropy coding, packets for quantizer_conf.q0_ds_ratio > 1 and for segmented mode (a count per frame, mode 1: below).
 * Measured 2026-10-21 on the MI355X (tools/code_pack.py, profiles/code_pack.txt; median of 24, every call synchronised): both launches
 * are bound by their launch -- 17.7 us to pack and 17.0 us to unpack 16 x 250 frames x 32 stages x 10 bits (1.02 MB of int64, 0.16 MB of
 * packets), 17.9 / 17.6 us for 32 x 1 x 32, 18.5 / 18.3 us for 1 x 7500 x 32; pack plus one copy of the packets 50.9 us against 59.8 us
 * for a copy of the int64 codes.  Packing does not pay in time: the feature is the bytes. */
/* By the packet rule of csrc/code_pack_kernels.h: the row pitch of a packet buffer for up to `frames` frames of n_q stages; host
 * arithmetic, works without a GPU.  0 for arguments outside the format (frames < 0, n_q outside 1..255, bits outside 1..16). */
size_t fc_code_packet_pitch(int frames, int n_q, int bits);
/* By the packet rule of csrc/code_pack_kernels.h: 8 + ceil(frames k bits / 8), the length of one packet; 0 as above. */
size_t fc_code_packet_bytes(int frames, int k, int bits);
/* By the packet rule of csrc/code_pack_kernels.h: codes dev i64 [n_q][B][Tf] -> packets dev u8 [B][pitch].  frames_rows, n_q_rows: dev
 * i32 [B] or NULL (all Tf / all n_q); both are read and clamped on the device (frames to [0, Tf], k to [1, n_q]), so n_q_rows_out of
 * fc_engine_set_rate feeds it directly; nothing behind a row's frames or k is read; a code is taken modulo 2^bits; every byte up to
 * the pitch is written.  Refused before any launch, naming the argument: bits outside 1..16, n_q outside 1..255, a pitch below
 * fc_code_packet_pitch(Tf, n_q, bits) (or no multiple of 4), null codes / packets. */
int fc_codes_pack(const int64_t* codes, int B, int Tf, int n_q, int bits, const int32_t* frames_rows, const int32_t* n_q_rows,
                  uint8_t* packets, size_t pitch, void* stream);
/* By the packet rule of csrc/code_pack_kernels.h: packets dev u8 [B][pitch] -> tokens dev i64 [B][Tf][n_q], the layout the decode
 * calls take, zeros at stages >= k and frames >= frames.  The headers' frames and k are clamped on the device to Tf and n_q; `bits` is
 * the call's.  Refusals as for fc_codes_pack. */
int fc_codes_unpack(const uint8_t* packets, size_t pitch, int B, int Tf, int n_q, int bits, int64_t* tokens, void* stream);

/* ---- the bit stream, mode 1: a stage count per frame (entry points added without a struct change: FC_ABI_VERSION stays 7) ----
 * csrc/code_pack_kernels.h states mode 1 (header: u32 frames, u8 kmax, u8 bits, u8 mode = 1, u8 0; a counts section of cbits = bit
 * length of kmax bits per frame, padded to a 32-bit word; a codes section of value S_t + i = codes[i][b][t], frame-major);
 * funcodec_amd/io.py restates it on the host.  None of the calls needs an engine.  Sessions opened per frame write and read mode 1
 * (fc_engine_set_floor_frames, fc_engine_set_push_frame_nq).  Not built: entropy coding, a fused decode from packets, frame mode by target
 * SNR in stream and slot sessions, a rule with memory over pushes. */
/* By the packet rule of csrc/code_pack_kernels.h (mode 1): the row pitch for up to `frames` frames of up to n_q stages each: the largest
 * packet (kmax = n_q, every count n_q) rounded up to 16; 0 for arguments outside the format. */
size_t fc_frame_packet_pitch(int frames, int n_q, int bits);
/* By the packet rule of csrc/code_pack_kernels.h (mode 1): 8 + 4 ceil(frames cbits / 32) + ceil(n_codes bits / 8); 0 for arguments
 * outside the format (n_codes outside 0 .. frames kmax included). */
size_t fc_frame_packet_bytes(int frames, int kmax, long long n_codes, int bits);
/* By the packet rule of csrc/code_pack_kernels.h (mode 1): bytes of the workspace both calls below take: one int32 table [B][Tf + 1], the
 * exclusive scan of the counts. */
size_t fc_frame_pack_workspace_bytes(int B, int Tf);
/* By the packet rule of csrc/code_pack_kernels.h (mode 1): codes dev i64 [n_q][B][Tf] and n_q_frames dev i32 [B][Tf] -> packets dev u8
 * [B][pitch].  frames_rows dev i32 [B] or NULL (all Tf).  Frames and counts are read and clamped on the device (frames to [0, Tf], a
 * count to [0, n_q], 0 behind the row's frames; kmax is the largest clamped count), so n_q_frames_out of fc_engine_set_rate_frames feeds
 * it directly; nothing behind a frame's count or a row's frames is read; every byte up to the pitch is written.  Refused before any
 * launch, naming the argument: as fc_codes_pack (the pitch against fc_frame_packet_pitch), a null n_q_frames, a workspace that is null or
 * smaller than fc_frame_pack_workspace_bytes, and a Tf * n_q that an int32 scan cannot hold. */
int fc_codes_pack_frames(const int64_t* codes, int B, int Tf, int n_q, int bits, const int32_t* frames_rows, const int32_t* n_q_frames,
                         uint8_t* packets, size_t pitch, void* workspace, size_t workspace_bytes, void* stream);
/* By the packet rule of csrc/code_pack_kernels.h (mode 1): packets dev u8 [B][pitch], every row of mode 1 or mode 0 -> tokens dev i64
 * [B][Tf][n_q] (zeros behind counts and frames) and n_q_frames dev i32 [B][Tf] (a mode-0 row: its k inside its frames), which
 * fc_engine_set_frame_nq takes as it is: packets to waveform without a read-back.  Header and counts are clamped on the device and every
 * read stays inside the row's pitch.  Refusals as for fc_codes_pack_frames, the pitch against fc_code_packet_pitch. */
int fc_codes_unpack_frames(const uint8_t* packets, size_t pitch, int B, int Tf, int n_q, int bits, int64_t* tokens, int32_t* n_q_frames,
                           void* workspace, size_t workspace_bytes, void* stream);

/* _linear_overlap_add (funcodec/models/codec_basic.py:77-116), the tail of Encodec._decode (:382-396) when
 * model_conf.segment_dur is set: triangle-weighted overlap-add of the decoded segments, products accumulated in
 * frame order and divided once by the summed weights, exactly as the reference orders it.
 *   frames      dev array of n_frames dev pointers, frame f = f32 [B, lens[f]] (decoded, UNTRIMMED segment f, which
 *               starts at sample f*stride); lens dev i32 [n_frames]; frame0_len = lens[0] (sizes the window, host copy)
 *   out         dev f32 [B, out_len]: the first out_len samples of the sum (Encodec.inference trims to the input, :711)
 * Rows are independent: a stereo model passes B * 2 rows. */
int fc_overlap_add(const float* const* frames, const int* lens, int n_frames, int B, int frame0_len, int stride,
                   int out_len, float* out, void* stream);

/* ---- streaming session (causal time-domain nets: norm weight_norm, causal true) ----------------------------------------
 * The reference has no streaming implementation (`streaming=` of bin/codec_inference.py selects a data iterator), so the
 * specification is the offline callable itself: the pushes of one utterance add up to Encodec.inference_encoding
 * (codec_basic.py:720-764) of their concatenation for fc_stream_encode, and to Encodec.inference_decoding /
 * inference_decoding_emb (:766-836) of the concatenated codes / embeddings for the two decode calls.
 *   - every push but the final one is a positive multiple of the hop; the final one (final = 1) has any length >= 1 and takes
 *     the reference's extra_padding (conv.py:57-64) at every layer; a push that breaks the rule fails, it is never padded;
 *   - the offline call pads every causal conv on the left by REFLECTION (pad1d, conv.py:82-99,251-253), i.e. with columns
 *     1..padding_total of the layer's own input: the first push of an utterance must therefore hold fc_stream_min_first
 *     samples (encode) / frames (decode); from then on a frame's codes and samples depend on nothing that comes later;
 *   - the volume scale of audio_normalize (codec_basic.py:366-371) is a function of the whole utterance, which no stream
 *     knows: the session takes one scale per utterance at reset (NULL = 1), encode divides by it, decode multiplies by it
 *     when use_scale is set (:406-407);
 *   - everything carried between pushes (per conv the last padding_total input columns, one input column per transposed
 *     conv, the LSTMs' (h, c), the scale) lives in ONE caller-owned device buffer of fc_stream_state_bytes bytes, 16-byte
 *     aligned; nothing is allocated per push; encoder and decoder state are separate, so one session may do both;
 *   - refused at create, the key named in the message: non-causal nets, seq_model transformer (fc_stream_create has no bound for
 *     its key / value cache: fc_seqstream_create below opens such a net), model freq_codec, quantizer_conf.q0_ds_ratio > 1.  Segmented mode (model_conf.segment_dur) is not a property of the engine -- fc_arch has no
 *     such field, the segments are a host-side loop over offline calls -- so only the host session can refuse it, and does.
 * Calls on one engine, its sessions included, are serialised by the caller; sessions do not disturb each other or the
 * offline calls. */
typedef struct fc_stream fc_stream;
size_t fc_stream_state_bytes(const fc_engine* e, int B);       /* 0: this engine cannot stream */
int  fc_stream_create(fc_engine* e, int B, int max_chunk_samples, int n_q, void* state /* dev */, size_t state_bytes, fc_stream** out);
void fc_stream_destroy(fc_stream* s);
/* shortest first push of an utterance: samples, a multiple of the hop (decode = 0) or frames (decode = 1) */
int  fc_stream_min_first(const fc_stream* s, int decode);
/* device scratch of any push of this session (tail slack included, as fc_engine_workspace_bytes) */
size_t fc_stream_workspace_bytes(const fc_stream* s);
/* starts an utterance: clears the state; scale dev f32 [B] or NULL.  Required before the first push. */
int  fc_stream_reset(fc_stream* s, const float* scale, void* stream);
/*   wav dev f32 [B][C][Tc];  codes dev i64 [n_q][B][*n_frames];  quantized, enc_out dev f32 [B][*n_frames][D] or NULL
 *   *n_frames (host) = Tc / hop, or ceil at every encoder stride for the final push (= fc_engine_frames(Tc)) */
int  fc_stream_encode(fc_stream* s, const float* wav, int Tc, int final, int64_t* codes, float* quantized, float* enc_out, int* n_frames,
                      void* workspace, size_t workspace_bytes, void* stream);
/*   codes dev i64 [B][Tfc][n_q] (n_q of create);  emb dev f32 [B][Tfc][D];  wav dev f32 [B][C][Tfc * hop];  emb_out as fc_decode_codes */
int  fc_stream_decode_codes(fc_stream* s, const int64_t* codes, int Tfc, int use_scale, float* wav, float* emb_out,
                            void* workspace, size_t workspace_bytes, void* stream);
int  fc_stream_decode_emb(fc_stream* s, const float* emb, int Tfc, int use_scale, float* wav,
                          void* workspace, size_t workspace_bytes, void* stream);

/* A push that fails after it has begun (workspace too small, a launch error) leaves carries half written: every later call of
 * the session fails with a message until fc_stream_reset.  Size the workspace with fc_stream_workspace_bytes to rule the first out.
 * Test hook: the SLSTM stage of a push alone (lstm.py:22-28 without the res_seq skip) on the session's encoder (decoder = 0) or
 * decoder (decoder = 1) LSTM state: x, y dev f32 [B][H][T]; consecutive calls continue one recurrence, as consecutive pushes do. */
int  fc_stream_lstm_forward(fc_stream* s, int decoder, const float* x, int T, float* y, void* workspace, size_t workspace_bytes, void* stream);

/* ---- streaming a causal net whose bottleneck is the TransformerEncoder (seq_model: transformer, causal: true) -------------
 * (entry points added without a struct change: FC_ABI_VERSION stays 7)
 * Causal attention sees every earlier frame, so a session keeps the keys and values of every block of both bottlenecks, and a cache
 * needs a size: max_frames, the most frames one utterance may hold per side (encoder / decoder), given at create.  The session is an
 * ordinary fc_stream: every fc_stream_* call works on it and the semantics are those above.  At the bottleneck of either side, with
 * pos the frames the side has taken since fc_stream_reset: a push of n frames appends its K and V to every block's cache at
 * [pos, pos + n), and query i of the push sees keys 0 .. pos + i (transformer.py:172-177), inside the first push too; LayerNorm, the
 * Linears and the feed-forward are per frame.  The caches lie behind what fc_stream_state_bytes lays out: per side, per block,
 * K [B][C][F] then V [B][C][F] floats, F = max_frames rounded up to 16, the first cache at a multiple of 256 bytes.
 *   - a push that would take a side past max_frames is refused before its first launch and changes nothing (the message names
 *     max_frames); the session goes on, fc_stream_reset starts the next utterance.  reset does not clear the caches: a frame is
 *     written before it is read, and no key behind pos + n reaches a result;
 *   - refused at create: max_frames < 1 or below the first push (fc_stream_min_first), a net without a transformer bottleneck
 *     (the message names max_frames), and whatever fc_stream_create refuses for other reasons;
 *   - fc_slots_create refuses these nets as fc_stream_create does; fc_seqslots_create below opens their slot session. */
size_t fc_seqstream_state_bytes(const fc_engine* e, int B, int max_frames);       /* 0: this engine cannot stream this way */
int  fc_seqstream_create(fc_engine* e, int B, int max_chunk_samples, int n_q, int max_frames, void* state /* dev */, size_t state_bytes,
                         fc_stream** out);
/* Test hook, the sibling of fc_stream_lstm_forward: the transformer stage of a push alone (all blocks and after_norm, without the
 * res_seq skip) on the session's encoder (decoder = 0) or decoder (decoder = 1) cache: x, y dev f32 [B][C][T]; it advances that
 * side's frame count, so consecutive calls continue one utterance, as consecutive pushes do. */
int  fc_seqstream_forward(fc_stream* s, int decoder, const float* x, int T, float* y, void* workspace, size_t workspace_bytes, void* stream);

/* ---- slot session: S slots that start, push and end independently in ONE batch ------------------------------------------
 * A streaming push is bound by its launches, so S independent callers cost about what one costs when they share a push.  A slot
 * session has S slots, each one utterance at a time; the specification is the streaming session's: the pushes of one utterance
 * add up to the offline call on that utterance alone, whatever the other slots do (they may hold NaN: nothing behind a row's
 * count is read).  The state is the streaming session's for B = S (one caller-owned buffer, nothing allocated per push), the
 * refusals at create are the same, and so is the start-up rule (fc_slots_min_first).
 *
 * A push is [S][..][width] with, per slot, a count (samples for encode, frames for decode) and flags, both HOST int32 [S]:
 *   count 0                 the slot sits idle in this push (flags must be 0); its state is carried over untouched
 *   FC_SLOT_START           the push begins an utterance: left context by reflection, LSTM state cleared, and (encode) the slot's
 *                           volume scale set from scale[slot] (dev f32 [S]; NULL = 1).  scale is read for START rows only;
 *                           decode multiplies by the slot's current scale when use_scale is set.  START on a slot whose utterance
 *                           is still running abandons that utterance (allowed)
 * The slots' scales are the first S floats of the state buffer.  fc_slots_create writes 1 into them (a synchronous copy: the
 * buffer must be allocated and not in use by then), so a slot whose encoder never started decodes with scale 1; a caller that
 * only decodes may write a slot's scale there itself, on the stream of its pushes, before the slot's decode START.
 *   FC_SLOT_FINAL           the push ends the utterance (with START: a whole utterance in one push): an encode row takes the
 *                           reference's extra_padding at every layer and may have any count >= 1; a decode row changes no sample
 * The rules, checked for every slot BEFORE the first launch -- a refused push changes nothing, the message names the slot and the rule:
 *   - 1 <= width <= max_chunk_samples (decode: / hop, rounded up); every count in [0, width]; at least one slot active;
 *   - a push without START needs a running utterance in that slot (one that has STARTed and not taken its FINAL push);
 *   - a push without FINAL is a positive multiple of the hop (encode); it is never padded silently;
 *   - a START push holds at least fc_slots_min_first samples / frames.
 * Encoder and decoder phases of a slot are separate.  Outputs are laid out as in the streaming calls over the common width; behind
 * a row's valid part (ceil(count / hop) frames, count * hop samples) every output is zero.
 * A push that fails after its first launch (workspace too small, a launch error) leaves carries half written: every slot then
 * refuses to continue until it is restarted with START, on either side.
 * Calls on one engine, its sessions included, are serialised by the caller. */
#define FC_SLOT_START 1
#define FC_SLOT_FINAL 2
typedef struct fc_slots fc_slots;
size_t fc_slots_state_bytes(const fc_engine* e, int S);        /* 0: this engine cannot stream */
int  fc_slots_create(fc_engine* e, int S, int max_chunk_samples, int n_q, void* state /* dev */, size_t state_bytes, fc_slots** out);
void fc_slots_destroy(fc_slots* s);
int  fc_slots_min_first(const fc_slots* s, int decode);
size_t fc_slots_workspace_bytes(const fc_slots* s);
/*   wav dev f32 [S][C][Tc];  codes dev i64 [n_q][S][fc_engine_frames(Tc)];  quantized, enc_out dev f32 [S][frames][D] or NULL */
int  fc_slots_encode(fc_slots* s, const float* wav, int Tc, const int32_t* samples, const int32_t* flags, const float* scale, int64_t* codes,
                     float* quantized, float* enc_out, void* workspace, size_t workspace_bytes, void* stream);
/*   codes dev i64 [S][Tfc][n_q];  emb dev f32 [S][Tfc][D];  wav dev f32 [S][C][Tfc * hop];  emb_out as fc_decode_codes */
int  fc_slots_decode_codes(fc_slots* s, const int64_t* codes, int Tfc, const int32_t* frames, const int32_t* flags, int use_scale, float* wav,
                           float* emb_out, void* workspace, size_t workspace_bytes, void* stream);
int  fc_slots_decode_emb(fc_slots* s, const float* emb, int Tfc, const int32_t* frames, const int32_t* flags, int use_scale, float* wav,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Test hook: the SLSTM stage of a slot push alone on the session's encoder / decoder LSTM state: x, y dev f32 [S][H][T]; row b takes
 * steps[b] <= T steps (a step beyond leaves its (h, c) as they were, y = 0 there) and begins from zeros where start[b] != 0; both host [S]. */
int  fc_slots_lstm_forward(fc_slots* s, int decoder, const float* x, int T, const int32_t* steps, const int32_t* start, float* y,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- slot session of a causal transformer net (seq_model: transformer, causal: true) ----------------------------------------
 * (entry points added without a struct change: FC_ABI_VERSION stays 7)
 * The slot session with the key / value cache of fc_seqstream_create: size and layout of the state are fc_seqstream_state_bytes(e, S,
 * max_frames)'s, and the session is an ordinary fc_slots for every fc_slots_* call above.  What a lock-step session keeps once, the
 * frames a side has taken since reset, a slot session keeps per slot and side, on the host: a START push sets the slot's count to 0
 * (the caches are not cleared: a frame is written before it is read), every enqueued push adds the row's frames.  At the bottleneck
 * row b of a push takes its own n_b frames (ceil(count / hop) of an encode push) at its own position pos_b: K and V go to
 * [pos_b, pos_b + n_b) of the slot's own cache rows and query i sees keys 0 .. pos_b + i, by the arithmetic and the split of the work
 * of a one-row lock-step push (n_b, pos_b); the positions travel to the device in the push's one copy of counts and flags.  A slot's
 * results therefore do not depend on S, on the push's width or on what the other slots do.
 *   - a push that would take ANY slot past max_frames is refused before its first launch, by the rules above: the message names the
 *     slot and max_frames, nothing changes for any slot, and a push with START begins the refused slot's next utterance;
 *   - refused at create: max_frames < 1 or below the START push (fc_slots_min_first), a net without a transformer bottleneck (the
 *     message names max_frames), and whatever fc_slots_create refuses for other reasons. */
size_t fc_seqslots_state_bytes(const fc_engine* e, int S, int max_frames);        /* 0: this engine cannot stream this way */
int  fc_seqslots_create(fc_engine* e, int S, int max_chunk_samples, int n_q, int max_frames, void* state /* dev */, size_t state_bytes,
                        fc_slots** out);
/* Test hook, the sibling of fc_seqstream_forward and fc_slots_lstm_forward: the transformer stage of a slot push alone on the
 * session's encoder / decoder cache: x, y dev f32 [S][C][T]; row b takes frames[b] <= T frames (y = 0 behind them) and begins at
 * position 0 where start[b] != 0; both host [S].  It advances the side's per-slot frame counts, refuses a row past max_frames before
 * anything is enqueued, and neither reads nor changes the slots' phases. */
int  fc_seqslots_forward(fc_slots* s, int decoder, const float* x, int T, const int32_t* frames, const int32_t* start, float* y,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- graph replay of a session's pushes (opt-in per session, off by default) ------------------------------------------------
 * (entry points added without a struct change: FC_ABI_VERSION stays 7; fc_graphstream_* take an fc_stream, fc_graphslots_* an fc_slots)
 * A push is some 60 small launches.  With graph replay on, a push is enqueued as ONE hipGraphLaunch of a graph captured from the very
 * launches the push makes without it (one stream, a linear chain); what is computed does not change.  Measured, replay saves the host's
 * time to enqueue (about 0.16 of 0.2 ms per push) and nothing else: the device runs the same kernels one after the other.
 * Every check of a push runs first, as ever: a refused push changes nothing.  Then the push's KEY is looked up among the session's
 * graphs.  The key holds every host value the enqueued work depends on: the call form (encode, decode_codes, decode_emb), the width
 * (Tc / Tfc), the parity of the side's push count, n_q, use_scale, EVERY POINTER ARGUMENT (inputs, outputs -- NULL for an absent one --,
 * scale, workspace and its size, the stream), the width of the quantiser's search (fc_engine_set_rvq_beam) and whether per-row stage counts are set (fc_engine_set_row_nq), with the table's
 * device address and width.  A hit replays; a miss captures (hipStreamCaptureModeThreadLocal on the caller's stream, which must
 * not be the null stream), instantiates, launches and stores the graph.  So a caller whose pointers repeat from push to push -- fixed
 * input, output and workspace buffers -- replays, two graphs per (side, form, width) in the steady state, one per parity; a caller
 * whose pointers move captures every time, which costs more than the eager push.
 *   - fc_stream: the first push of an utterance (reflection staging) and the final push are one-offs and run eagerly;
 *   - fc_slots: every push qualifies.  Its one copy of counts, flags and cache positions from host memory is issued in front of
 *     the replay, to the head of the workspace, where the captured kernels read it; with a key / value cache the attention's grid is
 *     sized by the bound that depends on the width alone, the rows' counts and positions are read on the device;
 *   - a session of fc_seqstream_create is REFUSED (its cache position is a launch argument that changes with every push; the message
 *     names max_frames and points to the slot session);
 *   - while engine profiling is live (fc_engine_profile) pushes run eagerly;
 *   - at most 16 graphs per session, the least recently used one is evicted; all go with the session or with fc_graph*_set(s, 0);
 *     fc_stream_reset and START keep them;
 *   - if the stream cannot be captured or the graph not instantiated, that push runs eagerly and `fallbacks` counts it.  A launch that
 *     fails while capturing, or a failing hipGraphLaunch, is a failed push as above (fc_stream_reset / START), and no graph is stored;
 *   - FC_SESSION_GRAPH=0 in the environment makes fc_graph*_set(s, 1) a no-op that returns 0 and leaves the session eager
 *     (fc_graph*_enabled then reports 0).
 * fc_graph*_set returns non-zero with fc_last_error set when refused.  counts: {replays, captures, evictions, fallbacks} since create. */
int  fc_graphstream_set(fc_stream* s, int on);
int  fc_graphstream_enabled(const fc_stream* s);
int  fc_graphstream_counts(const fc_stream* s, int64_t counts[4]);
int  fc_graphslots_set(fc_slots* s, int on);
int  fc_graphslots_enabled(const fc_slots* s);
int  fc_graphslots_counts(const fc_slots* s, int64_t counts[4]);

/* ---- the slot record: export a running call and import it in another session ----------------------------------------------------
 * (entry points added without a struct change: FC_ABI_VERSION stays 7)
 * A slot record is a copy of everything one utterance in flight owns: a flat run of floats in a fixed order -- the slot's scale, then
 * per side the read half of every conv's carry, (h, c) of every LSTM layer and, with a key / value cache, K and V of every block at
 * the pitch of the frames held.  funcodec_amd/csrc/slots_kernels.h is its specification.  The record is canonical: a pure function of
 * the utterance's pushes, whatever the session's S, the slot index, max_frames, max_chunk_samples, the parity of its push counters,
 * graph replay and the other slots.  Any session of the same architecture imports it, and the call goes on bit for bit as if it had
 * never moved.  fc_slot_meta is the host part: the phases (0 idle, 1 running, 2 ended) and cached frames of both sides, and `layout`,
 * a fingerprint of the segment list (kinds and lengths): it tells architectures apart, NOT checkpoints.  A side that is not running
 * contributes zeros and 0 frames.
 *   fc_slotrec_floats         the record's length for the given frame counts (both 0 in a session without a cache)
 *   fc_slotrec_export         records[i] = the record of slots[i], meta[i] its host part; the source is only read and goes on as before,
 *                             so export + import is also a fork of a call.  ONE launch for the n slots, on `stream`, between pushes.
 *   fc_slotrec_import         the inverse: slots[i] takes records[i] / meta[i].  It abandons whatever the slot held, as START does,
 *                             writes the DESTINATION's read halves and the destination's cache pitch, sets the slot's phases and frame
 *                             counts from meta and touches no other slot.  ONE launch.
 *   fc_slotrec_export_stream  row b of a lock-step session as a slot record (the same code: both kinds are one session layout).
 * slots, meta: host [n]; records: dev f32 [n][pitch_floats].  Refused before the first launch -- nothing changes, the message names the
 * slot and the rule: n outside [1, S], a slot out of range or named twice; pitch_floats below a record's length; export of a slot that
 * a failed push has invalidated or from a broken stream; import of another layout; frames past the destination's max_frames; frames
 * into a session without a cache, or a record without a cache into a session with one.  A refused call returns 1.  An import that
 * fails after its launch invalidates the slots it named, as a failed push does, and returns 2, so that a caller who keeps books of
 * its own tells the two apart without reading the message.
 * Cost at create: every fc_stream / fc_slots create (the fc_seq* ones included) now builds the segment table, one small hipMalloc
 * (freed at destroy) and one synchronous copy of a few KB, whether the session ever exports or not. */
typedef struct { uint32_t layout; int32_t enc_phase, dec_phase, enc_frames, dec_frames; } fc_slot_meta;
size_t fc_slotrec_floats(const fc_slots* s, int enc_frames, int dec_frames);
int  fc_slotrec_export(fc_slots* s, int n, const int32_t* slots, float* records /* dev [n][pitch] */, size_t pitch_floats,
                       fc_slot_meta* meta /* host [n] */, void* stream);
int  fc_slotrec_import(fc_slots* s, int n, const int32_t* slots, const float* records, size_t pitch_floats, const fc_slot_meta* meta, void* stream);
int  fc_slotrec_export_stream(fc_stream* s, int n, const int32_t* rows, float* records, size_t pitch_floats, fc_slot_meta* meta, void* stream);

/* Deferred device-side failures.  Kernels cannot return a status, so two conditions are recorded in host-visible
 * status words and reported by the NEXT fc_* compute call on the engine (non-zero return, message in fc_last_error(),
 * condition cleared) or by this call.  *flags (may be NULL) receives the conditions pending at entry:
 *   FC_STATUS_FLAG_LSTM_TIMEOUT  the persistent LSTM kernel's grid barrier timed out (workgroups not co-resident);
 *                                that call's outputs are NaN-poisoned; the engine falls back to per-step launches
 *   FC_STATUS_FLAG_BAD_CODE      fc_decode_codes saw an index outside [0, codebook_size) (F.embedding would raise)
 * Call it after synchronising the stream to learn about the calls enqueued so far. */
#define FC_STATUS_FLAG_LSTM_TIMEOUT 1u
#define FC_STATUS_FLAG_BAD_CODE 2u
#define FC_STATUS_FLAG_BAD_LENGTH 4u   /* a length-aware call saw a row length outside [1, Tmax] (clamped) */
int fc_engine_status(fc_engine* e, unsigned* flags);

/* ---- per-op entry points (so tests can pin each kernel against torch.nn.functional) -------------- */
/* DRVQ.forward on rows: x dev f32 [N,D], codebooks as loaded; codes dev i64 [n_q,N];
 * quantized dev f32 [N,D] or NULL.  With fc_arch.q0_ds_ratio > 1 the rows are ONE utterance of N >= 2 frames and
 * `workspace` must hold N * 4 bytes (the stage-0 source-row table); otherwise the workspace is unused. */
int fc_rvq_encode(fc_engine* e, const float* x, int N, int n_q, int64_t* codes, float* quantized,
                  void* workspace, size_t workspace_bytes, void* stream);

/* HOST function, no GPU: frames[t] = the frame whose stage-0 code frame t receives when quantizer_conf.q0_ds_ratio > 1, i.e. the
 * composition of the reference's two nearest-neighbour F.interpolate calls (ddp_core_vq.py:396-404: Tf -> Tf // 2 -> Tf) that the
 * kernels apply as a row table.  Exported so that the restatement of torch's index arithmetic is tested against torch itself. */
int fc_q0_source_frames(int Tf, int32_t* frames /* host, Tf entries */);

/* One SConv1d / SConvTranspose1d of the plan, addressed by its checkpoint prefix (e.g.
 * "encoder.model.3.conv", "decoder.model.3.convtr"): y = GroupNorm(conv(pad(act(x)))) as the reference
 * module computes it (conv.py:243-305), x dev f32 [B,Cin,T], y dev f32 [B,Cout,Tout] (trimmed for convtr).
 * apply_elu: apply ELU to x first (the nn.ELU that precedes the module in the Sequential). */
int fc_layer_forward(fc_engine* e, const char* prefix, const float* x, int B, int T, int apply_elu,
                     float* y, void* workspace, size_t workspace_bytes, void* stream);
/* The same layer in any call form the encode / decode drivers use (run_encoder / run_resblocks / run_decoder): the drivers' own run_conv
 * with the sources they hand over, so the kernel is the one the product picks for that layer, form and shape.
 *   x0, x1     dev f32 [B][Cin][T] (x1 NULL = one source)
 *   aff0, aff1 dev f32 [B][Cin][2] (scale, shift) pending GroupNorm affines, or NULL
 *   div0       dev f32 [B]: x0 is divided by div0[b] (the volume scale of the encoder's first conv), or NULL
 *   the layer's input is act(aff0(x0 / div0) + aff1(x1)), act = ELU when apply_elu; y as fc_layer_forward.
 * Refused on the host: a second source for a layer the plan gives one (its staging has no room for two), div0 on any layer but the
 * encoder's first conv, div0 together with aff0, a 2-D layer.  fc_layer_forward is this call with x0 alone.  A test hook. */
int fc_layer_forward_src(fc_engine* e, const char* prefix, const float* x0, const float* aff0, const float* div0, const float* x1,
                         const float* aff1, int B, int T, int apply_elu, float* y, void* workspace, size_t workspace_bytes, void* stream);
/* output length of that layer for input length T (-1: unknown prefix, or a 2-D layer) */
int fc_layer_out_len(const fc_engine* e, const char* prefix, int T);
/* fc_layer_forward refuses the 2-D layers of the STFT-domain codec (model_type 1) on the host, before any launch; they go through: */

/* One SConv2d / SConvTranspose2d of the 2-D nets (conv.py:342-447), addressed by its checkpoint prefix: an encoder or decoder "...conv"
 * of SEANetEncoder2d / SEANetDecoder2d or a decoder "...convtr" (whose last_out_padding, seanet_decoder.py:279, follows from the prefix:
 * the last decoder stage).  Runs the same run_conv2d / run_convtr2d the encode / decode drivers call, so the kernel branch is the
 * product's own for that shape; the inputs are first copied into workspace buffers in the engine's frequency-major layout with
 * reflected halo rows, as the drivers hand activations over.
 *   x0, x1     dev f32 [B][C][F][T] (the reference's layout; x1 NULL = one source)
 *   aff0, aff1 dev f32 [B][C][2] (scale, shift) pending GroupNorm affines, or NULL
 *   the layer's input is act(aff0(x0) + aff1(x1)), act = ELU when apply_elu (a convtr always has apply_elu = 1)
 *   y          dev f32 [B][Cout][Fo + 2 out_halo][Tout]: the GroupNorm'd output (raw for weight_norm nets) with the halo rows the
 *              engine hands to the next layer; out_halo is 0 or the engine's frequency halo.
 * A test hook: the drivers never call it. */
int fc_layer2d_forward(fc_engine* e, const char* prefix, const float* x0, const float* aff0, const float* x1, const float* aff1,
                       int B, int F, int T, int apply_elu, int out_halo, float* y, void* workspace, size_t workspace_bytes, void* stream);
/* dims[0] = Cout, dims[1] = Fo + 2 out_halo, dims[2] = Tout of that call for input [B][C][F][T]; dims[3] = workspace bytes it needs
 * (tail slack included); dims[4] = C, the layer's input channels.  Host only.  out_halo = -1 returns the engine's frequency halo in
 * dims[0] and nothing else. */
int fc_layer2d_out_shape(const fc_engine* e, const char* prefix, int B, int F, int T, int out_halo, int64_t* dims /* [5] */);

/* The back end of the STFT-domain codec behind the 2-D decoder (FreqCodec._decode_frame, codec_freq.py:419-448), through the very function
 * the decode driver calls after its last conv: softplus(magnitude) x phase (mag_phase, C = 3) or x (cos, sin)(sin(o1) pi) (mag_angle,
 * C = 2) -> inverse-DFT GEMM -> window-envelope division, centre trim, x scale[b], the first out_len samples.
 *   dec      dev f32 [B][C][F][Tp] (the reference's layout), C = input_channels, F = n_fft / 2 + 1; copied into a workspace buffer in the
 *            engine's frequency-major layout without halo rows, as the decoder's last conv leaves its output
 *   aff      dev f32 [B][C][2] (scale, shift): that conv's pending GroupNorm affine, or NULL (weight_norm nets)
 *   scale    dev f32 [B] or NULL
 *   wav      dev f32 [B][out_len], 1 <= out_len <= stft_hop * (Tp - 1)
 *   spec     dev f32 [B][2 F][Tp] or NULL: the spectrum rows the inverse-DFT GEMM reads (real rows, then imaginary rows)
 * Refused on the host, before any launch: a time-domain engine, C or F other than the engine's, Tp < 2, out_len outside its range.
 * A test hook: the drivers never call it. */
int fc_freq_synthesis(fc_engine* e, const float* dec, const float* aff, const float* scale, int B, int C, int F, int Tp, int out_len,
                      float* wav, float* spec, void* workspace, size_t workspace_bytes, void* stream);
/* the same refusals, and the workspace bytes of that call (tail slack included).  Host only. */
int fc_freq_synthesis_size(const fc_engine* e, int B, int C, int F, int Tp, int out_len, size_t* workspace_bytes);

/* SEANetResnetBlock.forward (seanet_encoder.py:44-61; decoder copy seanet_decoder.py:42-59) addressed by its Sequential
 * prefix ("encoder.model.1", "decoder.model.16"): y = shortcut(x) + block(x), each conv followed by its GroupNorm (when the
 * recipe has one); x, y dev f32 [B,C,T].  Exercises the fused shortcut + block.1 launch of the thin (C <= 64) blocks. */
int fc_resblock_forward(fc_engine* e, const char* prefix, const float* x, int B, int T,
                        float* y, void* workspace, size_t workspace_bytes, void* stream);
/* The same block on the input the drivers hand it: aff0(x0) + aff1(x1) (x1, aff1 NULL: one source; affines [B][C][2] as above), through
 * run_resblocks, so the thin blocks run reshead_kernel<C, k, DUAL> with one or two sources.  A second source is refused on the host for
 * a block the plan gives one (block 0 of a stage).  fc_resblock_forward is this call with x0 alone. */
int fc_resblock_forward_src(fc_engine* e, const char* prefix, const float* x0, const float* aff0, const float* x1, const float* aff1,
                            int B, int T, float* y, void* workspace, size_t workspace_bytes, void* stream);

/* SLSTM.forward (lstm.py:22-28) addressed by prefix ("encoder.model.16.lstm"): x,y dev f32 [B,C,T]. */
int fc_lstm_forward(fc_engine* e, const char* prefix, const float* x, int B, int T,
                    float* y, void* workspace, size_t workspace_bytes, void* stream);

/* TransformerEncoder.forward (normed_modules/transformer.py:150-208: blocks, after_norm, + x when res_seq) addressed by prefix
 * ("encoder.model.16"): x, y dev f32 [B,C,T]; the workspace of fc_engine_workspace_bytes for the same (B, T * hop) suffices. */
int fc_seq_forward(fc_engine* e, const char* prefix, const float* x, int B, int T,
                   float* y, void* workspace, size_t workspace_bytes, void* stream);

/* ---- profiling aid ------------------------------------------------------------------------------- */
/* Algorithmic work of one fc_encode_decode call: flops and bytes, total and for the
 * implicit-GEMM conv kernel family only. */
typedef struct fc_work {
    double total_flops, total_bytes;
    double conv_flops, conv_bytes;
    double lstm_flops, rvq_flops;
    int32_t conv_launches, total_launches;
} fc_work;
int fc_engine_work(const fc_engine* e, int B, int T, int n_q, fc_work* out);

/* Optional in-engine timing: when enabled, every conv launch (and each LSTM block / RVQ launch) is
 * bracketed by hipEventRecord on the caller's stream.  fc_engine_profile_read() synchronises on the
 * last event, returns per-kernel-class totals accumulated since the last read and resets them. */
typedef struct fc_prof {
    char    kernel[64];      /* named like rocprofv3 prints it, e.g. "conv_mfma_kernel<128, 128, 2, 2, 0, 8, false>",
                                "lstm_persist_kernel<NS> (...)" for the persistent recurrence */
    double  total_ms;        /* sum of event-to-event durations */
    double  flops, bytes;    /* algorithmic work of those launches */
    int32_t launches;
    int32_t reserved;
} fc_prof;
#define FC_PROF_CLASSES 48
int fc_engine_profile(fc_engine* e, int enable);
/* fills out[0..n) (n <= FC_PROF_CLASSES, returned through *n_out); unused entries have launches == 0 */
int fc_engine_profile_read(fc_engine* e, fc_prof* out /* [FC_PROF_CLASSES] */);

/* Kernel-phase timeline of the last conv launch, [2 roles][24 work items][8 stamps] of shader-clock ticks.
 * Only builds made with FC_TIMELINE=1 record anything (all zeros otherwise); a tuning aid, not part of the path. */
int fc_debug_timeline(unsigned long long* dst /* [2*24*8] */);

/* Host-side description of the implicit-GEMM conv kernel's operand layout for one chunk shape (k taps, CC channels per chunk, BM x BN tile);
 * no GPU work -- what the CPU tests check the weight packing and the B-operand offset table against.
 *   info[0] 1 = quad-k layout   info[1] floats per packed weight chunk   info[2] entries of the offset table   info[3] slab row stride
 *   info[4] columns per stride phase (PL)   info[5] slab width in input columns
 *   pack_index (optional) [k][CC][BM]: float index of W[row][chunk channel][tap] inside the packed chunk image
 *   koff (optional): the B-operand offset table (floats), one entry per half-quad (quad layout) or per k-step (round-4 layout) */
int fc_debug_conv_layout(int k, int stride, int dil, int CC, int BM, int BN, int row, int* info /* [6] */, int* pack_index, size_t pack_cap,
                         int* koff, size_t koff_cap);

/* Test hook for the STFT-domain codec (model_type 1): the NEXT fc_encode / fc_encode_decode call of this thread hands its feature tensor
 * (the 2-D encoder's input, codec_freq.py:356-379) to `dev_buf` (mode 1) or takes it from there (mode 2), in the reference's layout
 * [B][input_channels][n_fft / 2 + 1][1 + T / stft_hop] fp32; mode 0 disarms.  One shot.  Why it exists: torch.angle of a bin whose
 * imaginary part is rounding noise around a negative real part is +pi or -pi by the FFT's rounding, so for codec_domain mag_angle no
 * second STFT implementation reproduces the reference's feature tensor bin for bin; the parity tests compare the features modulo 2 pi
 * and pin the rest of the path from the reference's own features. */
int fc_debug_freq_features(void* dev_buf, size_t cap_bytes, int mode);

/* ---- host-side wire formats of the CLI (no GPU work) -------------------------------------------
 * The text form of one utterance's codes, byte for byte what funcodec/bin/codec_inference.py:295-299 writes with
 * json.dumps(indices[:, b, :len].tolist()) for the single frame of non-segmented inference: "[[[i, i, ...], [...], ...]]"
 * (n_q rows of `len` integers, ", " separators).
 *   codes   HOST i64 [n_q][B][T];  out: at least fc_codec_json_bound(n_q, len) bytes;  *written = bytes produced (no terminator) */
size_t fc_codec_json_bound(int n_q, int len);
int fc_format_codec_json(const int64_t* codes, int n_q, int B, int T, int b, int len, char* out, size_t cap, size_t* written);
/* save_audio (codec_inference.py:153-161): peak-rescale to 0.99 (rescale != 0; else clamp to +-0.99), round(x * 32768) clamped to
 * int16, mono 16-bit PCM RIFF file.   wav HOST f32 [n] */
int fc_write_wav_pcm16(const char* path, const float* wav, int n, int sample_rate, int rescale);

/* ======================================================================================================================
 * LauraTTS generation (ABI version 5; SURVEY.md §8f rank 3, BASELINE.json configs[4]): text -> conformer text encoder ->
 * decoder-only rel-pos transformer LM sampling the first `predict_nq` codec groups autoregressively -> non-autoregressive
 * conformer predicting the dense codec embedding -> fc_decode_emb of the codec engine above.
 * Replaces, for inference, funcodec/models/audio_generation/laura_model.py (LauraGenModel.encode :186-202, decode_codec :501-548,
 * cal_codec_emb :296-333 as syn_audio :550-567 calls it), funcodec/lm/transformer_lm.py (TransformerEmbedLM.score :266-313),
 * funcodec/models/encoder/conformer_encoder.py / transformer_encoder.py (the three rel-pos stacks) and
 * funcodec/modules/attention.py:212-308.  The reference re-scores the whole prefix for every token (no KV cache, batch 1, one
 * host round trip per token); this engine keeps a KV cache, decodes a batch of <= 16 prompts per call and samples on the device.
 * Same conventions as above: "dev" = device pointer, "host" = host pointer, fp32, int64 token ids, work enqueued on `stream`
 * (fc_laura_decode_codec additionally synchronises the stream, see there). */
typedef struct fc_laura fc_laura;

/* one rel-pos self-attention stack: ConformerEncoder without CNN / macaron modules (conformer_encoder.py:317-532) or
 * TransformerEncoder_s0 (transformer_encoder.py:424-654) */
typedef struct fc_laura_stack {
    int32_t idim, d_model, heads, ff, layers;
    int32_t act;          /* FFN activation: 1 = ReLU (TransformerEncoder_s0), 2 = Swish (conformer) */
    int32_t embed_relu;   /* ReLU after the input layer's LayerNorm (transformer_encoder.py:463-469) */
    int32_t norm_style;   /* state_dict names of the block norms: 0 = norm_mha / norm_ff, 1 = norm1 / norm2 */
} fc_laura_stack;

typedef struct fc_laura_arch {
    int32_t abi_version;            /* FC_ABI_VERSION */
    int32_t input_size;             /* width of the text embeddings (T5: 1536) or of token_embedding */
    int32_t vocab_size;             /* > 0: the checkpoint holds token_embedding [vocab_size][input_size] */
    int32_t codebook_size;          /* 1024 (the reference's index shift is hard-wired to it, laura_model.py:29) */
    int32_t codebook_dim;           /* 128 */
    int32_t num_quantizers;         /* rows of quantizer_codebook.embed */
    int32_t predict_nq;             /* codec groups the LM predicts per frame */
    int32_t pos_emb_split;          /* model_conf.pos_emb_type: 1 = "split" (abs. positional encoding per part, laura_model.py:312-317), 0 = "uni" */
    int32_t bidirectional_inputs;   /* codec_lm_conf.bidirectional_inputs (transformer_lm.py:286-288) */
    int32_t max_positions;          /* longest sequence any stack will see (sizes the relative-position tables; <= 2048) */
    fc_laura_stack text_encoder, codec_lm, codec_encoder;
} fc_laura_arch;

/* Text2AudioGenTask.build_model (funcodec/tasks/text2audio_generation.py:202-247) */
int  fc_laura_create(const fc_laura_arch* arch, int device, fc_laura** out);
void fc_laura_destroy(fc_laura* e);
/* checkpoint contract, as fc_engine_*: state_dict names of LauraGenModel (host fp32 tensors in the reference's layout) */
int  fc_laura_num_weights(const fc_laura* e);
int  fc_laura_weight_info(const fc_laura* e, int i, const char** name, int64_t* dims);
int  fc_laura_set_weight(fc_laura* e, const char* name, const float* host, const int64_t* dims, int ndim);
int  fc_laura_finalize(fc_laura* e);
/* device scratch for any call with B utterances, texts of <= L tokens, <= Cmax prompt / codec tokens and max_length new tokens */
size_t fc_laura_workspace_bytes(const fc_laura* e, int B, int L, int Cmax, int max_length);

/* LauraGenModel.encode (laura_model.py:186-202): text encoder + text_enc_out_layer.
 *   text_emb  dev f32 [B][L][input_size] or NULL;  text_ids dev i64 [B][L] or NULL (token_embedding lookup,
 *             bin/text2audio_inference.py:99-113; ids < 0 = padding): exactly one of the two
 *   text_lens host i32 [B];   text_outs dev f32 [B][L][codebook_dim] (rows >= text_lens[b] zero) */
int fc_laura_encode(fc_laura* e, const float* text_emb, const int64_t* text_ids, const int32_t* text_lens, int B, int L,
                    float* text_outs, void* workspace, size_t workspace_bytes, void* stream);

/* TransformerEmbedLM.score (transformer_lm.py:266-313) at EVERY position of [<sos>, text, <task>, codec...] in one pass
 * (teacher forcing): logp[b][t] = log_softmax of the decoder output at position t, i.e. what decode_codec samples token
 * t - text_lens[b] - 1 from.   codec dev i64 [B][Cmax][predict_nq] or NULL, codec_lens host i32 [B] or NULL;
 * logp dev f32 [B][Tseq][vocab], Tseq >= max_b(text_lens[b] + 2 + codec_lens[b]), vocab = predict_nq * (codebook_size + 1) */
int fc_laura_lm_logprobs(fc_laura* e, const float* text_outs, const int32_t* text_lens, int B, int L, const int64_t* codec,
                         const int32_t* codec_lens, int Cmax, float* logp, int Tseq, void* workspace, size_t workspace_bytes, void* stream);

/* LauraGenModel.decode_codec (laura_model.py:501-548) for a batch: prefix pass, then one KV-cached step per token, sampled on the device.
 *   continual  dev i64 [B][Cmax][predict_nq] or NULL, cont_lens host i32 [B] or NULL: prompt tokens (zero-shot continuation)
 *   sampling_mode 0 greedy (sampling=False) | 1 softmax (True) | 2 top-k (int, sampling_k) | 3 nucleus (float, sampling_p)
 *   seed       counter-based generator key; the same (seed, inputs) reproduce the same tokens
 *   forced     dev i64 [B][max_length][predict_nq] or NULL: teacher forcing (sampled ids are replaced by these)
 *   tokens     dev i64 [B][Cmax + max_length][predict_nq]: prompt tokens followed by the generated ones (<eos> step dropped)
 *   out_lens   host i32 [B]: valid rows of tokens[b] (filled after an internal stream synchronise, like the reference's .item())
 *   step_logp  dev f32 [B][max_length][vocab] or NULL: the log-probability vector every step sampled from
 * Utterances end at <eos> (any group) or after max_length steps; the call ends when all have. */
int fc_laura_decode_codec(fc_laura* e, const float* text_outs, const int32_t* text_lens, int B, int L, const int64_t* continual,
                          const int32_t* cont_lens, int Cmax, int max_length, int sampling_mode, int sampling_k, float sampling_p,
                          uint64_t seed, const int64_t* forced, int64_t* tokens, int32_t* out_lens, float* step_logp,
                          void* workspace, size_t workspace_bytes, void* stream);

/* LauraGenModel.cal_codec_emb (laura_model.py:296-333) on one-hot probabilities, as syn_audio (:550-567) calls it:
 *   codec dev i64 [B][Cmax][nq_cols] (the first predict_nq columns are used), codec_lens host i32 [B]
 *   emb   dev f32 [B][Cmax][codebook_dim] (rows >= codec_lens[b] zero): the input of fc_decode_emb */
int fc_laura_codec_emb(fc_laura* e, const float* text_outs, const int32_t* text_lens, int B, int L, const int64_t* codec, int nq_cols,
                       const int32_t* codec_lens, int Cmax, float* emb, void* workspace, size_t workspace_bytes, void* stream);

/* per-op entry point (tests pin each Linear against torch.nn.functional.linear): `name` = state_dict prefix of a Linear
 * ("codec_lm.encoder.encoders.3.feed_forward.w_1", "text_enc_out_layer", ...; "<block>.self_attn.linear_qkv" = the fused q/k/v).
 * x dev f32 [B][T][in], y dev f32 [B][T][out].  step_form != 0: through the decoding step's GEMV (LM layers only, B*T <= 64:
 * rows beyond 16 as further column blocks of 16, each the 16-row call on its own rows, bit for bit);
 * 1 = as the decoding step stages x, 2 = x in one LDS stage, 3 = x in at least two LDS windows (2 and 3 are test hooks). */
int fc_laura_linear(fc_laura* e, const char* name, const float* x, int B, int T, int step_form, float* y,
                    void* workspace, size_t workspace_bytes, void* stream);

/* per-op entry points of the two attention forms (tests pin them against a float64 restatement); both run the launch code of the path.
 *
 * Full-sequence rel-pos attention of block `layer` of a stack (0 text_encoder / 1 codec_lm / 2 codec_encoder) on the caller's q / k / v:
 *   qkv   dev f32 [B][T][3 d] token-major, q | k | v along the feature axis; transposed to the stack's feature-major layout at T padded
 *         to 4 with NO length masking (every value reaches the kernel: rows >= lens[b] must be finite)
 *   lens  host i32 [B] in [1, T]: keys >= lens[b] are masked;  bidir host i32 [B] or NULL: with causal, rows and keys < bidir[b] see each other
 *   ctx   dev f32 [B][T][d]: the attention context before linear_out (rows >= lens[b]: whatever the kernel leaves, finite) */
int fc_laura_attention(fc_laura* e, int stack, int layer, const float* qkv, const int32_t* lens, const int32_t* bidir, int causal, int B,
                       int T, float* ctx, void* workspace, size_t workspace_bytes, void* stream);

/* One block of the LM as the kernel chain's decoding step runs it, on 1 <= B <= 64 rows: QKV GEMV (LayerNorm prologue, cache scatter at
 * pos[b]), step attention over keys 0 .. pos[b], linear_out GEMV (combines the key-range partials while staging) + residual, the two
 * feed-forward GEMVs + residual.
 *   x        dev f32 [B][d]: the residual stream, replaced by the block's output
 *   k_cache  dev f32 [B][d][Tcap], v_cache dev f32 [B][Tcap][d]: this block's caches in the engine's layouts, column pos[b] is written
 *   pos      host i32 [B] in [0, min(Tcap, max_positions))
 *   key_ranges 1 .. 8 key ranges per (row, head); a decoding step of B rows takes 256 / (B * heads) clamped to 1 .. 8
 *   wide     != 0 with B <= 16: the GEMV instantiations over column blocks (what an elastic session's cut launch runs)
 *   q_out    dev f32 [B][d];  part_out dev f32 [B][heads][key_ranges][dk + 2]: per range the unnormalised context, running max, sum */
int fc_laura_step_block(fc_laura* e, int layer, float* x, float* k_cache, float* v_cache, const int32_t* pos, int B, int Tcap,
                        int key_ranges, int wide, float* q_out, float* part_out, void* workspace, size_t workspace_bytes, void* stream);

/* per-op entry point of the device sampler (tests pin every draw against a float64 restatement and a host Philox): the engine's own
 * sampler launch on the caller's logits and state, 1 <= B <= 64 rows, with the model's side of the launch (group layout, codebook table,
 * the LM's fused input layer) stated where a decoding step states it.  Two forms of the sampling parameters, the two the library launches:
 *   call form   rows == NULL: mode / k / p / seed / max_steps below for every row, neutral rules, Philox row word = the batch row
 *               (what fc_laura_decode_codec launches); forced / logp / score hold max_steps steps per row
 *   table form  rows host [B]: a row of the sampling table per row (what a decoding session launches); forced / logp / score hold R
 *               steps per row
 * Refused with a message: B, row0 / nrows, a mode, rule or max_steps out of range, state that would reach outside the R token rows
 * (tok_off + n_gen > R, tok_off + max_steps > R), a forced id outside 0 .. codebook_size.  Logits must be finite.  Synchronises the stream. */
typedef struct fc_laura_sample_row {
    int32_t mode, k;            /* 0 greedy, 1 softmax, 2 top-k (k), 3 nucleus (p) */
    float p;
    int32_t max_steps;          /* 1 .. R */
    uint64_t seed;
    int32_t forced_on;          /* 0: the row samples even when `forced` is given */
    uint32_t rng_row;           /* second word of the row's Philox counter */
    float temperature;          /* the five rules of fc_laura_slots_set_rules; 1, 0, 0, 0, 1 are the neutral ones */
    int32_t min_length;
    float top_p;
    int32_t repeat_window, repeat_count;
} fc_laura_sample_row;
typedef struct fc_laura_sample_io {
    const float* logits;        /* dev f32 [B][V], V = predict_nq * (codebook_size + 1) */
    int32_t *step, *n_gen, *done, *pos;     /* host i32 [B], in and out: samples drawn, tokens generated, ended, cache position */
    const int32_t* tok_off;     /* host i32 [B]: generated token g of row b is token row tok_off[b] + g */
    int32_t* n_done;            /* host i32 [1], in and out: the count of ended rows */
    int64_t* tokens;            /* dev i64 [B][R][predict_nq], in (the repeat rule's history) and out */
    const int64_t* forced;      /* dev i64 [B][steps][predict_nq] or NULL */
    float* logp;                /* dev f32 [B][steps][V] or NULL: row n_gen of a running row = log-softmax of its raw logits */
    float* score;               /* dev f32 [B][steps] or NULL: entry n_gen of a running row = the step's score term */
    float* next_emb;            /* dev f32 [B][codebook_dim]: written for rows that append a token */
    float* xs;                  /* dev f32 [B][LM width]: likewise, the LM's fused input layer of next_emb */
    const fc_laura_sample_row* rows;        /* host [B], or NULL: call form */
    int32_t B, R;
    int32_t mode, k;            /* call form */
    float p;
    uint64_t seed;
    int32_t max_steps;
    int32_t row0, nrows;        /* rows row0 .. row0 + nrows - 1 only (nrows 0: all B); the other rows' state and buffers are untouched */
} fc_laura_sample_io;
int fc_laura_sample(fc_laura* e, const fc_laura_sample_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* debugging aid, not part of the path: the NEXT full-sequence stack runs of this thread copy one intermediate tensor (feature-major
 * [B][rows][T padded to 4]) to dev_dst.  stack 0 text_encoder / 1 codec_lm / 2 codec_encoder (-1 any); what 0 = stream after the input
 * layer, 1 = attention-norm output of block `layer`, 2 = its q/k/v, 3 = its attention context, 5 = residual stream at the entry of
 * block `layer` (layer = number of blocks: before after_norm).  dev_dst NULL switches it off. */
int fc_laura_debug_probe(void* dev_dst, size_t cap_bytes, int stack, int layer, int what);

/* How fc_laura_decode_codec runs a decoding step (no reference counterpart: the reference re-scores the whole prefix per token,
 * funcodec/models/audio_generation/laura_model.py:501-548).  on = 1 (default; FC_LAURA_PERSIST=0 in the environment changes the default):
 * ONE persistent launch per step whose workgroups hand the token vectors to each other through arrival counters (csrc/laura_persist.hip);
 * on = 0: the chain of one kernel per Linear / attention (csrc/laura_kernels.hip).  Same arithmetic, results agree to fp32 rounding.
 * Returns 1 if the persistent form is in effect afterwards, 0 if the chain is (switched off, or the model / device cannot run it at any batch
 * size), -1 on a null handle.  Batches whose step does not fit the persistent kernel's LDS (d_model 1024: B > 2) still run on the chain. */
int fc_laura_set_persistent_step(fc_laura* e, int on);
/* The persistent launch needs all its workgroups resident; it is not a cooperative launch, so CUs held by another stream or process can make
 * a hand-off time out (bounded spins, no hang).  fc_laura_decode_codec then runs THAT call again on the kernel chain and succeeds with the
 * chain's result (a generation is a function of its seed), and the engine stays on the chain until fc_laura_set_persistent_step(e, 1).
 * This counter says how many calls of this engine went that way (0 normally; -1 on a null handle): a fallback is reported, never silent. */
int fc_laura_persistent_step_fallbacks(const fc_laura* e);

/* ---- decoding session: prompts join and leave a running batch (continuous batching of LauraGenModel.decode_codec,
 * laura_model.py:501-548, which the reference runs for one utterance at a time) ------------------------------------------
 * S slots (1 .. 16), each holding one utterance at a time.  One step call advances every running slot by the same number of
 * decoding steps; a slot can be started while the others are in the middle of theirs, and a slot that ended (<eos>, or its own
 * max_length) is free for the next prompt.  A slot depends on nothing but its own prompt and parameters: its tokens, length and
 * per-step log-probabilities are the same bits alone or in a full session, in any slot, whatever starts and ends around it (its
 * Philox counter is (seed, step, 0, group): the slot index is not in it).  A session of one slot is fc_laura_decode_codec on that
 * prompt alone, bit for bit; a session of S slots computes a row as an S-row call does (same key ranges per head).
 * Everything that survives a call lies in ONE device allocation of the caller (`state`, zero-filled or not): the key / value caches
 * [layers][S][d][max_positions] and [layers][S][max_positions][d], positions, counters and the per-slot sampling table, the step's
 * token vectors and hand-off buffers, tokens and forced tokens [S][max_positions][predict_nq] and, with_logp != 0, the per-step
 * log-probabilities [S][max_positions][vocab].  max_positions: a multiple of 4 in [16, the engine's]. */
typedef struct fc_laura_slots fc_laura_slots;
size_t fc_laura_slots_state_bytes(const fc_laura* e, int slots, int max_positions, int with_logp);   /* 0: refused (see create) */
int  fc_laura_slots_create(fc_laura* e, int slots, int max_positions, int with_logp, void* state, size_t state_bytes, fc_laura_slots** out);
void fc_laura_slots_destroy(fc_laura_slots* s);
/* device scratch of fc_laura_slots_start for a text of <= L tokens and <= Cmax prompt tokens */
size_t fc_laura_slots_workspace_bytes(const fc_laura_slots* s, int L, int Cmax);
/* The head of decode_codec for ONE prompt into slot `slot`: prefix pass (B = 1) into the slot's cache rows and the first sample.
 *   text_outs dev f32 [text_len][codebook_dim];  continual dev i64 [cont_len][predict_nq] or NULL (cont_len 0)
 *   sampling_mode / sampling_k / sampling_p / seed / forced (dev i64 [max_length][predict_nq] or NULL, copied): as fc_laura_decode_codec
 * Refused before any launch, changing nothing for any slot: a slot outside 0 .. S - 1, bad sampling arguments,
 * text_len + 2 + cont_len + max_length > max_positions.  A running slot's utterance is abandoned.  Revives a failed slot. */
int fc_laura_slots_start(fc_laura_slots* s, int slot, const float* text_outs, int text_len, const int64_t* continual, int cont_len,
                         int max_length, int sampling_mode, int sampling_k, float sampling_p, uint64_t seed, const int64_t* forced,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The loop body of decode_codec, n_steps times for every running slot (one captured graph of the step, replayed), then ONE
 * stream-ordered read-back.  Returns at once when no slot is running.
 *   done_out  host i32 [S] or NULL: 0 free, 1 running, 2 ended (take it), 3 failed;   n_gen_out host i32 [S] or NULL: tokens generated
 * A hand-off of the persistent step that times out fails every slot that was running (the step updates its rows in place and
 * cannot be repeated); the session then stays on the kernel chain and fc_laura_persistent_step_fallbacks counts the event. */
int fc_laura_slots_step(fc_laura_slots* s, int n_steps, int32_t* done_out, int32_t* n_gen_out, void* stream);
/* The tail of decode_codec for an ended slot, which is free afterwards (refused for a slot that has not ended):
 *   tokens dev i64 [cap][predict_nq]: prompt tokens followed by the generated ones;  len_out host: their number
 *   logp_out dev f32 [max_length][vocab] or NULL: what every step sampled from (zero rows past the last step) */
int fc_laura_slots_take(fc_laura_slots* s, int slot, int64_t* tokens, int cap, int32_t* len_out, float* logp_out);
/* The head of decode_codec (laura_model.py:501-548) for the prompt that slot `src` already holds, into slot `dst`: no prefix pass.  One
 * device copy of the source's prefix -- its first text_len + 2 + cont_len key / value positions in every layer and the logits its own
 * prefix pass ended with, which the session keeps per slot -- then the first sample with `dst`'s own parameters.  The result is, bit
 * for bit, the slot that fc_laura_slots_start gives for the same text, prompt tokens and parameters; the source is not disturbed, may
 * be in the middle of its utterance or ended (not yet taken), and may itself have been started this way.  Several candidates of one
 * prompt thus cost one prefix pass.
 *   max_length / sampling_mode / sampling_k / sampling_p / seed / forced: `dst`'s own, as fc_laura_slots_start
 * Refused before any launch, changing nothing for any slot: `dst` or `src` outside 0 .. S - 1, dst == src, a source that holds no
 * utterance (free, never started, failed), bad sampling arguments, max_length < 1, the source's text_len + 2 + cont_len + max_length >
 * max_positions.  A running `dst`'s utterance is abandoned. */
int fc_laura_slots_start_from(fc_laura_slots* s, int dst, int src, int max_length, int sampling_mode, int sampling_k, float sampling_p,
                              uint64_t seed, const int64_t* forced, void* stream);
/* decode_codec (laura_model.py:501-548) taken up in the middle of its loop :519-546: slot `dst` holds the utterance of slot `src` as it
 * stood after its first `keep` generated tokens -- the prompt, those tokens, their log-probability rows and the forced tokens are the
 * source's -- and goes on from there with its OWN sampling mode, seed and max_length.  No prefix pass and no decoding step is run: one
 * device copy of the source's key / value positions [0, text_len + 2 + cont_len + keep - 1) and one launch that copies the token and
 * log-probability rows, sets the counters and runs the LM's input layer on token keep - 1, exactly as the sampler did.  dst == src rewinds
 * a slot in place (no copy at all); an ended slot runs again.  Sample j of an utterance depends on the logits of step j and (seed, j)
 * only, so with the source's own mode and seed the destination ends as the source does, bit for bit, and with any other its per-step
 * log-probabilities are those of fc_laura_slots_start with its final tokens forced.  The source is not disturbed; it may be running or
 * ended (by <eos> or by length, not yet taken) and may itself be the product of a fork or of fc_laura_slots_start_from.
 *   keep        0 .. the source's n_gen as fc_laura_slots_step last reported it; < 0: all of them.  keep = 0 is
 *               fc_laura_slots_start_from without forced tokens, through the same code
 *   max_length  `dst`'s own, > keep; < 1: the source's
 *   sampling_mode / sampling_k / sampling_p / seed: `dst`'s own, as fc_laura_slots_start
 * Refused before any launch, changing nothing for any slot: `dst` or `src` outside 0 .. S - 1, a source that holds no utterance (free,
 * never started, failed), keep above the source's n_gen, max_length <= keep, text_len + 2 + cont_len + max_length > max_positions, bad
 * sampling arguments, a source that follows forced tokens with a max_length beyond them.  A running `dst` != `src` is abandoned. */
int fc_laura_slots_fork(fc_laura_slots* s, int dst, int src, int keep, int max_length, int sampling_mode, int sampling_k, float sampling_p,
                        uint64_t seed, void* stream);
/* A session that scores its candidates (with_score != 0; 0 is fc_laura_slots_state_bytes / fc_laura_slots_create, bit for bit and launch
 * for launch): one fp32 term per slot and generated step, [S][max_positions] floats behind everything else in `state`,
 *     term[j] = sum over the predict_nq groups k, in k order, of  x_k[t_k] - max(x_k) - log(sum_v exp(x_k[v] - max(x_k)))
 * with x_k the group's codebook_size + 1 logits of step j and t_k the step's FINAL pick (a forced token counts as the pick): the log of
 * the probability LauraGenModel.sampling_ids (laura_model.py:466-499) gives the picks before any top-k / nucleus truncation.  It is a
 * function of the step's logits and picks only -- the same bits in every sampling mode and for forced tokens -- and is written for every
 * step the slot's sampler runs, the ending <eos> step included.  start / start_from zero the slot's row; fork copies terms [0, keep) from
 * the source and zeroes the rest of the row (in place: only the zeros), so a branched utterance has the score of its whole path.  Nothing
 * is summed on the device. */
size_t fc_laura_slots_state_bytes_scored(const fc_laura* e, int slots, int max_positions, int with_logp, int with_score);
int  fc_laura_slots_create_scored(fc_laura* e, int slots, int max_positions, int with_logp, int with_score, void* state, size_t state_bytes,
                                  fc_laura_slots** out);
/* A WIDE session: slots 1 .. 64, everything else as the _scored pair (which keeps refusing more than 16).  The step's weight-streaming
 * GEMV takes 16 rows per workgroup (the MFMA's 16 columns); rows beyond them are further COLUMN BLOCKS of 16, block j = slot / 16, each
 * computed by the 16-column kernel on its own rows: a slot's bits do not depend on its block or on what the other blocks hold.  Up to
 * 16 slots a wide session IS the _scored session (state layout, launches, bits).  Above 16 the step runs as the kernel chain (the
 * persistent launch is built for 16 rows), captured once per session as before, and the key ranges per head follow the same rule
 * (256 / (slots * heads), 1 .. 8).  Every per-slot call takes every slot; fc_laura_slots_start_many stays at min(16, slots) prompts per
 * call.  A slot costs its key / value rows (2 * layers * d_model * max_positions floats), its token and forced-token rows, its logits
 * rows and, with_logp != 0, max_positions * vocab floats of log-probabilities. */
size_t fc_laura_slots_state_bytes_wide(const fc_laura* e, int slots, int max_positions, int with_logp, int with_score);
int  fc_laura_slots_create_wide(fc_laura* e, int slots, int max_positions, int with_logp, int with_score, void* state, size_t state_bytes,
                                fc_laura_slots** out);
/* The score row of a slot that holds an utterance (running or ended; the slot keeps it: call this ahead of fc_laura_slots_take):
 *   terms      HOST f32 [cap], cap >= max_positions: the slot's whole row, zeros behind the terms written
 *   count_out  host: terms written as fc_laura_slots_step last reported -- n_gen, plus 1 for a slot that ended on <eos>
 *   end_out    host: 0 the slot is running, 1 it ended by length, 2 it ended on <eos> (ended with n_gen < max_length)
 * Refused, with the slot named: a session created without scores, a slot outside 0 .. S - 1, a free, never-started or failed slot. */
int fc_laura_slots_score(fc_laura_slots* s, int slot, float* terms, int cap, int32_t* count_out, int32_t* end_out);
/* The sampling rules of slot `slot`, kept on the host side of the session: every later fc_laura_slots_start, _start_from or _fork with
 * that slot as the DESTINATION (dst == src, a rewind, included) writes them into the slot's row of the device sampling table, beside the
 * mode, seed and max_length of that call.  They hold until set again; a session that never calls this has the neutral rules.  The step
 * is not captured again and nothing else in it changes.
 * For a running slot the sampler visits every group k of G = codebook_size + 1 logits x, <eos> at index G - 1; gen = the tokens the slot
 * has generated so far.
 *   1. temperature T (finite, > 0):  y[v] = x[v] / T, an IEEE fp32 division; T = 1 gives y = x bit for bit.
 *   2. min_length n (>= 0):  while gen < n, y[G - 1] = -inf in every group: the utterance cannot end before it has n generated
 *      tokens (a forced token still can); max_length still ends it.
 *   3. Everything behind these two sees y: the greedy arg-max (lowest index on ties), the softmax total, the top-k select, the nucleus
 *      walk, and the step's score term, which becomes sum over k of log softmax(y_k)[pick_k] -- the distribution the pick is drawn from
 *      before truncation.  The log-probability rows (fc_laura_slots_take's logp_out) stay the whole-vocabulary log-softmax of the raw
 *      logits.
 *   4. top_p p (0 < p <= 1; 0 = none), with top-k sampling (sampling_mode 2) only: the top-k candidates in their order (probability
 *      descending, index ascending) are cut to the shortest prefix whose mass reaches p x the sum over the whole group; the entry that
 *      crosses is kept and at least one entry stays -- mode 3's walk, stopped at k.
 *   5. repeat_window W (0 .. 256, 0 = off) and repeat_count r (1 .. W), in the drawing modes (1, 2, 3) only: after the draw of t in group
 *      k let c be the number of generated tokens j in [max(0, gen - W), gen) whose group-k id equals t (prompt tokens are not in the
 *      window).  If c >= r, t is drawn again, once, from softmax(y) over all G entries in index order, by the same inverse-CDF routine
 *      as the first draw; its uniform number is Philox of the step's counter with the group word 8 + k (first draws use k < 8), so it is
 *      a function of (seed, step, group) and not of the slot index.  A forced token replaces the pick after all of this.
 *   6. The neutral rules -- T = 1, min_length 0, top_p 0, W = 0 -- are the session without rules bit for bit: tokens, log-probability
 *      rows, scores and random-number stream.
 * Refused before anything changes, with the slot named: a slot outside 0 .. S - 1, a non-finite or non-positive temperature, a
 * negative min_length, top_p outside [0, 1], repeat_window outside 0 .. 256, repeat_count outside 1 .. repeat_window when the window is
 * on.  top_p without top-k sampling and a window with greedy are refused by the start / start_from / fork that follows, together with
 * its "bad sampling arguments", before it changes anything.  fc_laura_decode_codec has no rules. */
int fc_laura_slots_set_rules(fc_laura_slots* s, int slot, float temperature, int min_length, float top_p, int repeat_window, int repeat_count);
/* (entry points added without a struct change: FC_ABI_VERSION stays 7)
 * The head of decode_codec (laura_model.py:501-548) for n DIFFERENT prompts into n slots with ONE prefix pass: the LM stack runs once at
 * B = n over time axes padded to the longest prompt; the reset, the output layer on the last position, and the first sample stay one
 * launch per slot, exactly those of fc_laura_slots_start.  After the call every named slot holds what fc_laura_slots_start would have
 * left there for its prompt and parameters, BIT FOR BIT -- cache positions [0, P), logits, position, token / forced / log-probability /
 * score rows, its row of the sampling table, the first sample: a column of the full-sequence stack depends on its own row's columns
 * only, never on the batch size, the padded length or a neighbour (DESIGN.md section 9 gives the argument per kernel).  No other slot
 * changes; the persistent step's launch number and arrival counters are not touched and the captured step is not captured again.
 *   n           1 .. min(16, S);  slots host i32 [n]: distinct, any order
 *   text_outs   dev f32 [n][L][codebook_dim], rows >= text_lens[b] ignored;  text_lens host i32 [n], 1 .. L
 *   continual   dev i64 [n][Cmax][predict_nq] or NULL, rows >= cont_lens[b] ignored;  cont_lens host i32 [n] (NULL with continual NULL)
 *   max_lengths / sampling_modes / sampling_ks host i32 [n], sampling_ps host f32 [n], seeds host u64 [n]: per row, as fc_laura_slots_start
 * Forced tokens are not taken (fc_laura_slots_start forces).  A slot's rules are those of fc_laura_slots_set_rules.
 * Every rule is checked for every row before the first launch; a refused call changes nothing for any slot and names the slot: a slot
 * outside 0 .. S - 1 or named twice, n outside 1 .. min(16, S), text_len + 2 + cont_len + max_length > max_positions, bad sampling
 * arguments or rules that do not go with the row's mode.  A named slot that is running abandons its utterance. */
size_t fc_laura_slots_start_many_workspace_bytes(const fc_laura_slots* s, int n, int L, int Cmax);
int fc_laura_slots_start_many(fc_laura_slots* s, int n, const int32_t* slots, const float* text_outs, const int32_t* text_lens, int L,
                              const int64_t* continual, const int32_t* cont_lens, int Cmax, const int32_t* max_lengths,
                              const int32_t* sampling_modes, const int32_t* sampling_ks, const float* sampling_ps, const uint64_t* seeds,
                              void* workspace, size_t workspace_bytes, void* stream);
/* fc_laura_slots_start_from across two sessions of the SAME fc_laura: slot `dst` of `dst_session` from the prompt that slot `src` of
 * `src_session` holds.  The sessions may differ in their slot count, in max_positions (hence in the pitch of the key rows) and in whether
 * they keep log-probabilities or scores.  One device copy (K rows of pad4(P) floats from one pitch to the other, the first P * d floats
 * of V, the source's prefix logits, the position) and the first sample with `dst`'s own parameters: the slot that fc_laura_slots_start
 * gives on `dst_session` for the same prompt, bit for bit.  The source row is not disturbed and may be imported any number of times; a
 * session that is never stepped can so hold prompts, prefilled several per pass by fc_laura_slots_start_many, for the slots of another.
 * BOTH SESSIONS ARE DRIVEN ON ONE STREAM: the copy is ordered behind the source's prefix pass by `stream` alone.
 * Refused before any launch, changing nothing, with the slot named: sessions of different engines (or the same session), `dst` or
 * `src` outside its session, a source that is free, never started or failed, bad sampling arguments, the source's text_len + 2 +
 * cont_len + max_length > the DESTINATION's max_positions.  A running `dst` is abandoned. */
int fc_laura_slots_start_from_session(fc_laura_slots* dst_session, int dst, const fc_laura_slots* src_session, int src, int max_length,
                                      int sampling_mode, int sampling_k, float sampling_p, uint64_t seed, const int64_t* forced,
                                      void* stream);
/* (entry points added without a struct change: FC_ABI_VERSION stays 7)
 * A QUEUED session: its slots are fed by a queue of TICKETS on the device and by nothing else.  A ticket names a row of `source` -- a
 * session of the same fc_laura that holds prompts (fc_laura_slots_start_many), fixed here; slot count and max_positions may differ --
 * and its own max_length, sampling mode, seed and rules.  At the head of EVERY decoding step, inside the captured step and with no word
 * from the host, (1) every slot whose utterance has ended is retired: its token rows, generated count, <eos> flag and, with_score, its
 * score row go to the ticket's entry of a result ring in the session state, and the slot is free in the same step; (2) every free slot,
 * in ascending order, claims the oldest waiting ticket.  Any number up to `slots` claim in one step.  A claimed slot is the slot
 * fc_laura_slots_start_from_session gives for (row, max_length, mode, seed, rules), BIT FOR BIT -- prefix keys / values and logits,
 * position, token row (the row's continual prompt, zeros behind), score row, sampling-table row, first sample, random-number stream --
 * so a ticket's result is a function of its row and parameters only, never of its slot, the step it was claimed at, its neighbours or
 * the n of fc_laura_slots_step.  The phase is four launches that read everything from device memory (laura_kernels.hip: a one-wave
 * kernel that retires and claims, two copy kernels, the one-row sampler over the claim table); none waits on anything.
 *   queue       1 .. 65536 result entries: the tickets that may be waiting, running or uncollected at one time
 *   with_score  as fc_laura_slots_create_scored.  There are no per-step log-probability rows and no forced tokens per ticket.
 * slots 1 .. 64; above 16 the session is a wide one.  fc_laura_slots_start, _start_many, _start_from, _start_from_session, _fork, _take
 * and _score are refused on a queued session, naming the call, and change nothing.  `source` must outlive the session, is driven on
 * the same stream, and a row of it may be overwritten once every ticket that names it has been claimed. */
size_t fc_laura_slots_state_bytes_queued(const fc_laura* e, int slots, int max_positions, int with_score, int queue);
int fc_laura_slots_create_queued(fc_laura* e, int slots, int max_positions, int with_score, int queue, const fc_laura_slots* source,
                                 void* state, size_t state_bytes, fc_laura_slots** out);
/* A ticket into the queue: one small stream-ordered launch, no synchronisation.  *ticket_out = 0, 1, 2, ... in submit order, which is the
 * order of claiming.  The rules are the five of fc_laura_slots_set_rules (1, 0, 0, 0, 1: neutral).  Everything
 * fc_laura_slots_start_from_session checks is checked here, on the host: the row holds a prompt, its prefix + max_length fits THIS
 * session's max_positions, the sampling arguments, the rules and that they go with the mode.  Refused as well while `queue` tickets are
 * waiting, running or uncollected.  A refused submit names the ticket and the row, takes no ticket number and changes nothing. */
int fc_laura_slots_submit(fc_laura_slots* s, int row, int max_length, int sampling_mode, int sampling_k, float sampling_p, uint64_t seed,
                          float temperature, int min_length, float top_p, int repeat_window, int repeat_count, int32_t* ticket_out,
                          void* stream);
/* The queue as the last fc_laura_slots_step read it back (the same single read-back as the slots' states; no device access here):
 * tickets submitted (host count), claimed, finished, failed and collected so far -- all monotone -- and slot_tickets host i32 [slots],
 * the ticket each slot runs or -1.  Any pointer may be NULL.  fc_laura_slots_step on a queued session reports a slot as running or free;
 * it also retires what its last step ended before it reads back, so a finished ticket never waits for another call. */
int fc_laura_slots_queue_status(const fc_laura_slots* s, int64_t* submitted, int64_t* claimed, int64_t* finished, int64_t* failed,
                                int64_t* collected, int32_t* slot_tickets);
/* Up to `cap` results out of the ring, with ONE synchronisation for all of them, and their entries free: failed tickets first, then the
 * finished ones in the order they finished.
 *   tickets / states / lens / n_gens / ends   host i32 [cap]: the ticket; 2 finished, 3 failed; token rows (prompt + generated);
 *                                             generated tokens; 1 ended by length, 2 on <eos> (the score row then has n_gen + 1 terms)
 *   tokens      dev i64 [cap][max_positions][predict_nq]: row j's first lens[j] rows are written
 *   scores      HOST f32 [cap][max_positions] or NULL: the whole score rows (a session created with_score)
 * A ticket fails when a hand-off of the persistent step timed out in a call it ran in: it has no tokens (lens 0), the session goes on
 * over the kernel chain and the waiting tickets are claimed as before. */
int fc_laura_slots_collect(fc_laura_slots* s, int cap, int32_t* tickets, int32_t* states, int32_t* lens, int32_t* n_gens, int32_t* ends,
                           int64_t* tokens, float* scores, int32_t* n_out);
/* (entry points added without a struct change: FC_ABI_VERSION stays 7)
 * An ELASTIC session steps as wide as the slots in use.  With `on` != 0 every fc_laura_slots_step call takes hi, the highest slot that
 * is RUNNING at the call, from the library's host mirror of the slot states (free, failed and ended-not-taken slots do not count) and
 * launches the step over rows = min(slots, 16 * (hi / 16 + 1)): the GEMV's grid.y is the column blocks [0, rows / 16), the step attention
 * and the sampler run rows [0, rows), and nothing else differs from the full step -- the same kernel instantiations (those over column
 * blocks, also when one block is left), the same buffers, layer strides and key-range split.  No slot can start inside a call, so the
 * width holds for all its n_steps.  Every step kernel indexes per-row memory from row 0 and no row reads another's, so the rows stepped
 * hold the full step's bits; the rows above the cut are not touched (a running slot is never among them).  Up to 16 slots there is one
 * block and nothing changes, the persistent step included; above 16 the step stays the kernel chain at every width.  One captured graph
 * per distinct width (at most 4), captured on first use and never again; the first step of a session runs eagerly as ever.
 * Refused on a queued session: its slots are claimed on the device and the host cannot know the busy rows. */
int fc_laura_slots_set_elastic(fc_laura_slots* s, int on);
/* The column blocks the last fc_laura_slots_step call launched (ceil(slots / 16) without set_elastic); 0 when it had no running slot and
 * launched nothing.  For tests and tools. */
int fc_laura_slots_step_blocks(const fc_laura_slots* s);
/* n slots to other rows: after the call slot dst[i] IS slot src[i], and src[i] is free.  Everything the session keeps per slot moves in
 * ONE launch of a copy kernel driven by a device table of the n lines (written by a one-wave launch ahead of it): key / value positions
 * [0, pos] of every layer; position, generated count, done flag, sample counter, prompt length; the row of the sampling table; the token
 * and score rows, the forced-token row of a slot that follows one, the log-probability rows [0, max_length); the step's logits and the
 * kept prefix logits; the pending LM input row and next-embedding row; and the host mirror of the slot (state, prefix and continual
 * lengths, max_length, whether it follows forced tokens).  The rules of fc_laura_slots_set_rules belong to the row they were set for and
 * change places with the destination's.  Nothing is re-derived and no layer runs: a running slot goes on as if it had never moved, an
 * ended one is taken from dst, a later fc_laura_slots_start_from / _fork from dst is the one from src.  Stream-ordered, no
 * synchronisation.  Refused before any launch, changing nothing and naming the slot: n outside 1 .. slots, a slot outside
 * 0 .. slots - 1, a slot named twice or on both sides, a source that holds no utterance (free, never started, failed), a destination
 * that is not free, a queued session. */
int fc_laura_slots_move(fc_laura_slots* s, int n, const int32_t* src, const int32_t* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FUNCODEC_AMD_H */
