/* libstylish_hip.so -- C ABI of the MI355X (gfx950) acoustic hot path of stylish-tts.
 *
 * The reference has no FFI: its boundary is torch.nn.Module forward() signatures plus state_dict key
 * names.  This ABI sits directly underneath those modules: a model object is
 * created per reference module, its parameters are bound BY THE REFERENCE'S state_dict KEY, and one entry
 * point per reference forward() runs the whole module on the caller's HIP stream.  Plain pointers and
 * sizes only; no torch types.  All activations are fp32, contiguous, channel-major [B, C, T].
 *
 * Conventions
 *   - every function returns 0 on success or a negative sty_status; sty_last_error() gives the text.
 *   - all pointers are DEVICE pointers unless the name ends in _host.
 *   - every entry point is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default).
 *   - the caller owns inputs, outputs and the workspace; the library owns only the prepared (repacked)
 *     weight arena of each model, allocated once in sty_model_finalize().
 *   - there is NO CPU fallback: without a HIP device every compute entry point returns STY_EHIP.
 */
#ifndef STYLISH_HIP_H
#define STYLISH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  STY_OK = 0,
  STY_EINVAL = -1, /* bad argument / unknown key */
  STY_ESHAPE = -2, /* tensor shape does not match the module's manifest */
  STY_EHIP = -3,   /* HIP runtime error (incl. no device) */
  STY_ENOMEM = -4, /* workspace too small */
  STY_ESTATE = -5  /* call order violated (e.g. forward before finalize) */
} sty_status;

typedef struct sty_model sty_model;

int sty_version(void);
const char *sty_last_error(void);

/* ---- model objects -------------------------------------------------------------------------------
 * kind: "speech_predictor"   = train/models/speech_predictor.py:10-73 (text_encoder + decoder + generator)
 *       "mel_style_encoder"  = train/models/mel_style_encoder.py:121-152
 *       "text_aligner"       = train/models/text_aligner.py:33-45 (inference only, see sty_aligner_fwd)
 *       "text_aligner_train" = the same module with a training graph (see sty_aligner_fwd_train)
 *       "rmvpe"              = train/dataprep/rmvpe/model.py:49-86 E2E0 (inference only, see sty_rmvpe_fwd)
 *       "wavlm"              = transformers WavLMModel in eval mode (frozen, see sty_wavlm_fwd / sty_wavlm_bwd)
 * Dimensions are taken from the bound tensors' shapes (train/config/model.yml defaults are checked).   */
int sty_model_create(const char *kind, sty_model **out);
void sty_model_destroy(sty_model *m);
/* Bind one state_dict entry by its reference key, e.g.
 *   "generator.basegen.phase_convnext.3.pwconv1.weight"  (SURVEY.md Appendix B).
 * The pointer must stay valid and may be updated in place by the optimiser between calls.            */
int sty_model_bind(sty_model *m, const char *key, const float *ptr, int ndim, const int64_t *shape);
/* Check that every key of the module's manifest is bound, allocate the prepared-weight arena.        */
int sty_model_finalize(sty_model *m);
/* Number of keys the manifest expects / i-th key (for binding loops and for tests).                  */
int sty_model_num_keys(const sty_model *m);
const char *sty_model_key(const sty_model *m, int i);
/* Re-derive effective weights (weight_norm g*v/|v|, spectral_norm W/sigma, MFMA operand packing, folded
 * GRN beta) from the bound parameters.  Call after every optimiser step; once for inference.          */
int sty_model_prepare(sty_model *m, void *stream);
/* Tell the library that bound parameters / buffers were modified in place (optimizer step, load_state_dict into the
 * same storage, BatchNorm / spectral-norm buffer updates): the next inference entry point re-prepares.  The
 * *_fwd_train entry points prepare on every call and leave the model marked stale.                      */
int sty_model_invalidate(sty_model *m);

/* ---- vocoder: MultiGenerator.forward (train/models/generator.py:884-901) -------------------------
 * mel [B,128,T], style [B,64], pitch [B,T], voiced [B,T]  ->  audio [B,1,300*T].
 * noise [B,300*T,9] is SineGen's randn draw (generator.py:440-442), explicit for parity; if NULL a
 *   counter-based generator seeded with `seed` is used instead.
 * prior_override [B,300*T] (optional) replaces the harmonic source output (generator.py:722).        */
typedef struct {
  int B, T;
  const float *mel, *style, *pitch, *voiced, *noise, *prior_override;
  uint64_t seed;
  float *audio;
  /* optional taps for parity tests (NULL = not written) */
  float *tap_conformer_out; /* [B,256,T]   */
  float *tap_prior;         /* [B,300T]    */
  float *tap_har_spec;      /* [B,32,75T]  */
  float *tap_har_phase;     /* [B,32,75T]  */
  float *tap_logamp_prior;  /* [B,32,75T]  */
  float *tap_phase_prior;   /* [B,32,75T]  */
  float *tap_trunk;         /* [B,32,75T]  */
  float *tap_logamp;        /* [B,32,75T]  */
} sty_vocoder_io;
int sty_vocoder_workspace_bytes(const sty_model *m, int B, int T, size_t *bytes);
int sty_vocoder_fwd(sty_model *m, const sty_vocoder_io *io, void *workspace, size_t ws_bytes, void *stream);

/* ---- SpeechPredictor.forward (train/models/speech_predictor.py:47-73) ----------------------------
 * texts [B,L] int64, text_lengths [B] int64, alignment [B,L,T], pitch/energy/voiced [B,T], style [B,64].
 * denormal_pitch [B,T] feeds the harmonic source (speech_predictor.py:69).                           */
typedef struct {
  int B, L, T;
  const int64_t *texts, *text_lengths;
  const float *alignment, *pitch, *energy, *voiced, *style, *denormal_pitch, *noise, *prior_override;
  uint64_t seed;
  float *audio;
  float *tap_text_encoding; /* [B,128,L] */
  float *tap_decoder_out;   /* [B,128,T] */
  sty_vocoder_io voc_taps;  /* only the tap_* fields are read */
  void *style_stream;       /* sty_speech_fwd_train: HIP stream on which `style` is being produced (NULL: the call's own
                               stream).  The call waits for that stream's current position right before the first use
                               of style, i.e. after the text encoder: a style encoder on a second stream overlaps it. */
} sty_speech_io;
int sty_speech_workspace_bytes(const sty_model *m, int B, int L, int T, size_t *bytes);
int sty_speech_fwd(sty_model *m, const sty_speech_io *io, void *workspace, size_t ws_bytes, void *stream);

/* ---- MelStyleEncoder.forward (train/models/mel_style_encoder.py:147-152) -------------------------
 * mel [B,1,80,T] -> style [B,64]                                                                      */
int sty_style_workspace_bytes(const sty_model *m, int B, int T, size_t *bytes);
int sty_style_fwd(sty_model *m, int B, int T, const float *mel, float *style, void *workspace, size_t ws_bytes,
                  void *stream);

/* ---- front end: calculate_mel (train/utils.py:825-834) + log energy (utils.py:73-85) --------------
 * audio [B,N] -> mel [B,80,frames] with frames = even(N/hop + 1); energy [B,frames] (optional).
 * 80 HTK mel bins at 24 kHz (train/config/model.yml), window = periodic hann(win_length) centred in n_fft.  */
int sty_mel_workspace_bytes(int B, int N, int n_fft, int hop, size_t *bytes);
int sty_mel_fwd(int B, int N, const float *audio, int n_fft, int win_length, int hop, float mean, float std,
                float *mel, float *energy, void *workspace, size_t ws_bytes, void *stream);

/* ---- MultiSpectrogram.calculate_single x3 (train/multi_spectrogram.py:40-55), resolutions (fft,hop) =
 * (512,128), (1024,256), (2048,512), win = fft.  audio [B,N] -> for each resolution i (frames = N/hop+1):
 *   mag[i]     [B,128,frames] = log1p(mel128(|X|))      phase[i] [B,F,frames] = (|X| > 1e-3) * angle(X) (optional)
 *   fft_mag[i] [B,F,frames]   = |X|,  F = fft/2+1                                                          */
int sty_multispec_workspace_bytes(int B, int N, size_t *bytes);
int sty_multispec_fwd(int B, int N, const float *audio, float *const *mag, float *const *phase,
                      float *const *fft_mag, void *workspace, size_t ws_bytes, void *stream);

/* ---- soft alignment: DurationProcessor.duration_to_alignment (train/utils.py:752-791) ------------
 * durations [B,L] -> alignment [B,L,T] (softmax over L)                                               */
int sty_alignment_fwd(int B, int L, int T, const float *durations, float *alignment, void *stream);

/* ---- second-stage predictors, inference ---------------------------------------
 * Models of kind "duration_predictor" / "pitch_energy_predictor", bound by the reference's state_dict keys.
 * DurationPredictor.forward(texts, text_lengths, style) (duration_predictor.py:74-87) -> dur_pred [B,L,classes];
 * PitchEnergyPredictor.forward(texts, text_lengths, alignment [B,L,T], style) (pitch_energy_predictor.py:62-82)
 * -> pitch [B,T], energy [B,T].  DurationProcessor (softmax over classes -> alignment) stays on the host side. */
int sty_duration_workspace_bytes(const sty_model *m, int B, int L, size_t *bytes);
int sty_duration_fwd(sty_model *m, int B, int L, const int64_t *texts, const int64_t *text_lengths, const float *style,
                     float *dur_pred, void *workspace, size_t ws_bytes, void *stream);
int sty_pitch_energy_workspace_bytes(const sty_model *m, int B, int L, int T, size_t *bytes);
int sty_pitch_energy_fwd(sty_model *m, int B, int L, int T, const int64_t *texts, const int64_t *text_lengths,
                         const float *alignment, const float *style, float *pitch, float *energy, void *workspace,
                         size_t ws_bytes, void *stream);

/* PitchStyleEncoder.forward(x [B,n_mels,T], pitch [B,T], energy [B,T]) -> [B,style_dim] at coarse_multiplier 1
 * (mel_style_encoder.py:155-205); model kind "pitch_style_encoder".                                             */
int sty_pitch_style_workspace_bytes(const sty_model *m, int B, int T, size_t *bytes);
int sty_pitch_style_fwd(sty_model *m, int B, int T, const float *mel, const float *pitch, const float *energy,
                        float *style, void *workspace, size_t ws_bytes, void *stream);

/* ---- alignment stage, inference (train/dataprep/align_text.py; `python -m stylish_tts_amd.align`) ------------------
 * Model kind "text_aligner" = tdnn_blstm_ctc_model_base(n_mels, tokens) in eval mode (train/models/text_aligner.py:33-45,
 * 130-274), bound by the reference's state_dict keys (encoder.layers.{0,1,2}.0.{weight,bias}, encoder.layers.{0,1,2}.2.
 * running_{mean,var}, encoder.layers.3.ffn.{0,3,6,9,12}.{weight,bias}, encoder_output_layer.{weight,bias});
 * hidden_dim, n_mels and tokens are read from the bound shapes.  CTCModel.forward (text_aligner.py:73-127) + the
 * "t b k -> b t k" of align_text.py:303:  mel [B,n_mels,T] (as sty_mel_fwd writes it), mel_lengths [B] int64 ->
 * log_probs [B,T,tokens+1].  Frames at or beyond mel_lengths[b] are zeroed in front of each of the three TDNN convs
 * (text_aligner.py:221-225).  fp32 operands and accumulation: sty_model_set_train_opts with compute_bf16 and
 * sty_model_enable_training / sty_model_bind_grad return STY_EINVAL for this kind.                                     */
int sty_aligner_workspace_bytes(const sty_model *m, int B, int T, size_t *bytes);
int sty_aligner_fwd(sty_model *m, int B, int T, const float *mel, const int64_t *mel_lengths, float *log_probs,
                    void *workspace, size_t ws_bytes, void *stream);
/* CTC forced alignment: torchaudio.functional.forced_align as align_text.py:317 calls it, for a whole batch.
 * log_probs [B,T,V1], targets [B,U] int64 (row b uses its first target_lengths[b] entries; none may equal `blank`),
 * input_lengths / target_lengths [B] int64 -> labels [B,T] int32 = the class emitted at every frame, scores [B,T] =
 * log_probs[b,t,labels[b,t]]; frames at or beyond input_lengths[b] get label -1 and score 0.  Viterbi over the
 * 2 * target_length + 1 states "blank, tok, blank, ..." in fp32 max / + only (DESIGN.md has the recurrence and its tie
 * rule).  status [B] int32: 0 = aligned; 1 = input_lengths[b] < target_lengths[b] + adjacent repeats (no alignment
 * exists; torchaudio raises); 2 = a length or a target out of range.  Rows with a non-zero status get labels -1 and
 * scores 0; the other rows of the batch are unaffected.  U <= 512, V1 <= 1024.                                         */
int sty_forced_align_workspace_bytes(int B, int T, int U, size_t *bytes);
int sty_forced_align(int B, int T, int V1, int U, const float *log_probs, const int64_t *targets,
                     const int64_t *input_lengths, const int64_t *target_lengths, int blank, int32_t *labels,
                     float *scores, int32_t *status, void *workspace, size_t ws_bytes, void *stream);

/* ---- pitch extraction (train/cli.py:205-243 `pitch --method rmvpe`, train/dataprep/pitch_extractor.py:137-149,
 *      train/dataprep/rmvpe/; `python -m stylish_tts_amd.pitch`) --------------------------------------------------------
 * Model kind "rmvpe" = E2E0(n_blocks, 1, (2, 2), 5, inter_layers, 1, en_out_channels) in eval mode (rmvpe/model.py:49-86,
 * deepunet.py, seq.py), bound by the reference's state_dict keys (unet.encoder.bn.*, unet.encoder.layers.L.conv.J.{conv.0,
 * conv.1, conv.3, conv.4, shortcut}.*, unet.intermediate.layers.I.conv.J.*, unet.decoder.layers.L.{conv1.0, conv1.1,
 * conv2.J}.*, cnn.*, fc.0.gru.{weight,bias}_{ih,hh}_l0[_reverse], fc.1.*); n_blocks, inter_layers and en_out_channels are
 * read from the bound tensors, five encoder / decoder levels, 128 mel bins, one BiGRU layer of 256 and 360 classes are fixed.
 * Inference only, fp32 operands (pitch values hang on an arg-max): compute_bf16, sty_model_enable_training and
 * sty_model_bind_grad return STY_EINVAL for this kind.
 * Front end (rmvpe/inference.py:45-60, rmvpe/spec.py): audio [B,N] at 24 kHz -> torchaudio Resample(24000, 16000,
 * lowpass_filter_width=128) (sinc_interp_hann, rolloff 0.99: two phases of 391 taps at stride 3, M = ceil(2N/3) samples) ->
 * MelSpectrogram(128, 16000, 1024, 200, None, 30, 8000): periodic hann, centre / reflect, MAGNITUDE spectrum, librosa
 * mel(htk=True) with Slaney normalisation, log(clamp(., 1e-5)) -> logmel [B,128,n], n = M / 200 + 1.  torchaudio and librosa
 * are restated from their documented closed forms: PARITY UNPINNED at this boundary.  The two tables, evaluated in double
 * and rounded to fp32 once, HOST memory: resample kernel [2][391] (phase, tap), mel basis [128][513].                    */
void sty_rmvpe_resample_kernel_host(float *out);
void sty_rmvpe_mel_basis_host(float *out);
int sty_rmvpe_mel_workspace_bytes(int B, int N, size_t *bytes);
int sty_rmvpe_mel_fwd(int B, int N, const float *audio, float *logmel, void *workspace, size_t ws_bytes, void *stream);
/* RMVPE.mel2hidden (rmvpe/inference.py:29-36): logmel [B,128,n] -> salience [B,n,360].  The frame axis is padded by
 * reflection to the next multiple of 32 and the whole net, the BiGRU included (its backward direction starts at the padded
 * end), runs on the padded length; the first n frames are kept.  n < 17 cannot be reflected: STY_ESHAPE.                 */
int sty_rmvpe_workspace_bytes(const sty_model *m, int B, int n, size_t *bytes);
int sty_rmvpe_fwd(sty_model *m, int B, int n, const float *logmel, float *salience, void *workspace, size_t ws_bytes,
                  void *stream);
/* to_local_average_f0 (rmvpe/utils.py:114-131): salience [B,n,360] -> f0 [B,n] in Hz.  Arg-max (lowest index on a tie),
 * the window [c-4, c+5) clipped to [0, 360), cents = sum s (20 i + 1997.3794084376191) / sum s, f0 = 10 * 2^(cents/1200),
 * 0 where the row's maximum is < thred.  Viterbi decoding (use_viterbi) is not built.                                   */
int sty_rmvpe_decode(int B, int n, const float *salience, float thred, float *f0, void *stream);

/* ---- alignment stage, training (train_alignment, train/stage_type.py:268-341; `python -m stylish_tts_amd.train_align`) --
 * Model kind "text_aligner_train": the keys and shapes of "text_aligner", with sty_model_enable_training /
 * sty_model_bind_grad accepted (compute_bf16 is refused as for its sibling).  sty_aligner_fwd serves this kind too (the
 * eval-mode forward on running statistics: validation).
 * sty_aligner_fwd_train = CTCModel.forward under module.train() (train/models/text_aligner.py:73-127, 209-274): per TDNN
 * layer the masked conv + ReLU, BatchNorm1d(affine=False) on the batch statistics of all B*T positions -- the bound
 * running_mean / running_var are updated in place (momentum sty_train_opts.bn_momentum, unbiased variance) -- and
 * Dropout(drop_p); the Ffn of five Linear + ReLU + Dropout with its skip; the output Linear and log_softmax.  Dropout masks
 * are the library's hash u(drop_seed, site, element) (its dropout everywhere): sites 0-2 behind the BatchNorms, 3-7 behind the Ffn's ReLUs, element = linear
 * index in [B][hidden][T]; keep = u >= drop_p, scaled by 1 / (1 - drop_p); drop_p = 0 skips them.
 * sty_aligner_bwd: d_logits [B][tokens+1][T] = d loss / d (input of the log_softmax), channel-major as sty_ctc_loss_fwd_bwd
 * writes it; parameter gradients are added to the bound gradient buffers.  One backward per forward (STY_ESTATE otherwise). */
int sty_aligner_train_workspace_bytes(sty_model *m, int B, int T, size_t *bytes);
int sty_aligner_fwd_train(sty_model *m, int B, int T, const float *mel, const int64_t *mel_lengths, float drop_p,
                          unsigned drop_seed, float *log_probs, void *workspace, size_t ws_bytes, void *stream);
int sty_aligner_bwd(sty_model *m, const float *d_logits, void *stream);
/* CTC loss and its gradient: CTCLossWithLabelPriors.forward (train/losses.py:478-653; k2.ctc_loss(reduction="mean",
 * use_double_scores=True, target_lengths=...) at losses.py:600-615) with the semantics of
 * torch.nn.functional.ctc_loss(reduction="mean", zero_infinity=False): exact CTC in float64 log-space, no beam (k2 prunes
 * with output_beam = 10: not reproduced).  log_probs [B,T,V1] (what sty_aligner_fwd[_train] writes); log_priors [V1] or
 * NULL: the scores are log_probs - prior_scale * log_priors (losses.py:585-588), the priors are constants; targets [B,U]
 * int64, input_lengths / target_lengths [B] int64.  nll [B] double = -log p(target | input); loss [1] =
 * mean_b(nll_b / max(U_b, 1)), unweighted; d_logits [B,V1,T] (NULL: loss only) = weight / (B max(U_b, 1)) *
 * (exp(log_probs) - occupancy), the log_softmax backward folded in, zero at and beyond input_lengths[b].
 * status [B] int32: 0 ok; 1 no valid path; 2 a length or a target out of range.  Rows with a non-zero status get
 * nll = +inf and a zero gradient (loss is then +inf); the other rows are unaffected.  U <= 512, V1 <= 1024.
 * workspace: alpha of every frame, [B][T][2U+1] double (read only with d_logits).                                      */
int sty_ctc_loss_workspace_bytes(int B, int T, int V1, int U, size_t *bytes);
int sty_ctc_loss_fwd_bwd(int B, int T, int V1, int U, const float *log_probs, const float *log_priors, float prior_scale,
                         const int64_t *targets, const int64_t *input_lengths, const int64_t *target_lengths, int blank,
                         float weight, double *nll, float *loss, int32_t *status, float *d_logits, void *workspace,
                         size_t ws_bytes, void *stream);

/* ---- fine-grained entry points for unit parity (each = one reference sub-module) ------------------ */
/* GeneratorConvNeXtBlock (conv_next.py:80-93) of channel count C on [B,C,T]; prefix e.g.
 * "generator.basegen.phase_convnext.0".                                                              */
int sty_convnext_fwd(sty_model *m, const char *prefix, int B, int C, int T, const float *x, const float *style,
                     float *y, void *workspace, size_t ws_bytes, void *stream);
/* AdaptiveGeneratorBlock (ada_norm.py:109-120), 32 channels, k=11, dil 1/3/5.                         */
int sty_resblock_fwd(sty_model *m, const char *prefix, int B, int T, const float *x, const float *style, float *y,
                     void *workspace, size_t ws_bytes, void *stream);
/* The same two sub-modules in the TRAINING graph, forward and backward in one call (unit parity of the fused backward
 * kernels -- the recompute-based ConvNeXt32 backward, the AdaIN / Snake prologue backward, the depthwise-conv and
 * LayerNorm backward): kind "convnext" or "resblock"; x, gy (= d loss / d y) [B,C,T] -> y, gx [B,C,T], d_style [B,64];
 * parameter gradients are added to the gradients bound with sty_model_bind_grad.                             */
int sty_block_train_workspace_bytes(sty_model *m, const char *kind, const char *prefix, int B, int C, int T,
                                    size_t *bytes);
int sty_block_fwd_bwd(sty_model *m, const char *kind, const char *prefix, int B, int C, int T, const float *x,
                      const float *style, const float *gy, float *y, float *gx, float *d_style, void *workspace,
                      size_t ws_bytes, void *stream);
/* Softmax attention (text_encoder.py:234-280 with `lengths`, conformer.py:85-91 without, prosody_encoder.py:23-40: 2 heads of
 * 160 / 96 with `lengths`) forward + backward on separate q, k, v [B, H*DH, T] (DH = 16, 64, 96 or 160): d_o -> dq, dk, dv.  */
int sty_attention_workspace_bytes(int B, int H, int T, size_t *bytes);
int sty_attention_fwd_bwd(int B, int H, int DH, int T, const float *q, const float *k, const float *v,
                          const int64_t *lengths, const float *d_o, float *o, float *dq, float *dk, float *dv,
                          void *workspace, size_t ws_bytes, void *stream);
/* The same with WavLM's gated relative position bias (modeling_wavlm.py, WavLMAttention): logit (i, j) = q_i . k_j / sqrt(DH) +
 * gate[b, h, i] * tab[h, j - i + T - 1]; gate [B, H, T], tab [H, 2T - 1] (fp32, never rounded), d_o -> dq, dk, dv and d_gate
 * [B, H, T] (written, no atomic).  compute_bf16 = 1 (DH 64 only): the five products on v_mfma_f32_32x32x16_bf16 with both operands
 * rounded to bf16, the bias added to the logit in fp32; 0: the fp32 kernels (DH 64 or 16).  Workspace as above.               */
int sty_attention_rel_fwd_bwd(int B, int H, int DH, int T, const float *q, const float *k, const float *v, const float *gate,
                              const float *tab, const float *d_o, float *o, float *dq, float *dk, float *dv, float *d_gate,
                              int compute_bf16, void *workspace, size_t ws_bytes, void *stream);
/* STFT(64, hop 4).transform -> (mag, atan2(y,x)) bins 0..31, last frame dropped (generator.py:724-729);
 * wave [B,N] -> spec, phase [B,32,N/4].                                                               */
int sty_stft64_fwd(int B, int N, const float *wave, float *spec, float *phase, void *stream);
/* the bases sty_stft64_fwd / sty_istft64_fwd use when a model binds none: the reference's registered buffers
 * (models/stft.py:39-96, to 2 ulp) forward_real, forward_imag, backward_real, backward_imag, each [33][64];
 * out = HOST memory, 4 * 33 * 64 floats.                                                              */
void sty_stft64_bases_host(float *out);
/* synthesis head: exp/atan2-free cos,sin + conv-transpose iSTFT + tanh (generator.py:782-799,896);
 * logamp, real, imag [B,32,F] -> audio [B,1,4F].                                                      */
int sty_istft64_fwd(int B, int F, const float *logamp, const float *real, const float *imag, float *audio,
                    void *stream);
/* harmonic source (generator.py:720-723, 415-447, 496-510): pitch, voiced [B,T], noise [B,300T,9] or
 * NULL -> prior [B,300T].  lin_w [9], lin_b [1] = m_source.l_linear.                                  */
int sty_source_fwd(int B, int T, const float *pitch, const float *voiced, const float *noise, uint64_t seed,
                   const float *lin_w, const float *lin_b, float *prior, void *workspace, size_t ws_bytes,
                   void *stream);
int sty_source_workspace_bytes(int B, int T, size_t *bytes);
/* Kernels of the backward's normalisation / activation glue alone, for unit tests.                     */
/* GRN (conv_next.py:15-18) backward on h [B,C4,T], C4 <= 1024: the forward's statistics and scale, then from ds [B,C4]
 * (= d loss / d scale) coef [B,C4] (d loss / d h += coef[b][c] h) and dgamma [C4] +=.  from_gx != 0: the backward starts
 * from the per-channel norms the forward kept (as the training graph does); 0: it rebuilds them from the partial sums. */
int sty_grn_bwd_workspace_bytes(int B, int C4, int T, size_t *bytes);
int sty_grn_bwd(int B, int C4, int T, const float *h, const float *ds, const float *gamma, int from_gx, float *coef,
                float *dgamma, void *workspace, size_t ws_bytes, void *stream);
/* Pointwise activation backward (kind: 1 ReLU, 2 Swish, 3 Snake with alpha [C], 5 exact GELU) on x, dy [B,C,T] -> dx
 * (accumulate: added to it), dalpha [C] += (Snake; may be NULL).  h [B,C,T], coef [B,C] (both or neither): the output
 * gradient is dy + coef[b][c] h; fused != 0: formed inside the activation kernel, 0: added to dy IN PLACE by a pass of
 * its own first.                                                                                                         */
int sty_act_bwd(int kind, int B, int C, int T, const float *x, float *dy, const float *alpha, const float *h,
                const float *coef, int fused, float *dx, int accumulate, float *dalpha, void *stream);
/* AdaIN fold from per-row partial sums part [B*C][nseg][2] doubles (sum, sum of squares over T samples), gb [B,2C] ->
 * a = (1 + gamma) rstd, s = beta - a mean [B,C]; mean, rstd [B,C] (both or neither): the statistics themselves.       */
int sty_adain_finalize(int B, int C, int T, int nseg, const double *part, const float *gb, float eps, float *a, float *s,
                       float *mean, float *rstd, void *stream);

/* ---- training (backward, K15): vocoder first ---------------------------------------------------------
 * sty_model_bind_grad: where the gradient of a bound parameter is ACCUMULATED (zero it yourself, e.g.
 * optimizer.zero_grad).  Call it (or sty_model_enable_training) before sty_model_finalize.
 * sty_vocoder_fwd_train runs MultiGenerator.forward in its training graph (eval-mode statistics: BatchNorm
 * running stats, no dropout) keeping what the backward needs in `workspace`, which must stay untouched until
 * sty_vocoder_bwd returns.  sty_vocoder_bwd takes d loss / d audio [B,1,300T] and writes d loss / d mel
 * [B,128,T] and d loss / d style [B,64] (each optional) and adds the parameter gradients.                  */
int sty_model_enable_training(sty_model *m);
/* module.train() behaviour of the *_fwd_train entry points (all zero = eval-mode statistics, the default).
 * Dropout masks are a counter-based hash of (dropout_seed, call site, element), not torch's Philox stream: parity with
 * the reference holds when its F.dropout / SDPA are patched to the same function (tools/gen_golden_train.py).   */
typedef struct {
  int bn_batch_stats;  /* conformer BatchNorm1d (conformer.py:183): batch statistics, running_mean / running_var of the
                          bound state_dict buffers are updated in place                                          */
  int sn_power_iter;   /* spectral_norm (mel_style_encoder.py:18-39): one power iteration per forward, weight_u /
                          weight_v of the bound state_dict buffers are updated in place                          */
  int f0_smooth;       /* Decoder box-smoothing width of F0 (decoder.py:53-75): 0, 7 or 15; the reference draws it
                          per step with random.randint, here the caller does                                      */
  int energy_smooth;   /* of the energy: 0, 7, 15 or 31                                                          */
  float bn_momentum;   /* 0.1 (nn.BatchNorm1d default)                                                           */
  unsigned dropout_seed; /* != 0: TextEncoder dropout is active (text_encoder.py: prenet 0.5 after every ReLU :63,:418;
                          encoder: attention probabilities :274, after attention :387, inside the FFN :328, after the
                          FFN :391).  Draw a new seed every step.  The conformer's dropouts are dead in the reference
                          (conformer.py:278-290 never forwards the rates).                                        */
  float text_dropout;  /* model.yml text_encoder.dropout (0.2)                                                    */
  int compute_bf16;    /* 1: config c3's "bf16 autocast for conv/GEMM": the operands of every dense conv / Linear of the
                          training graph (forward, input gradient, weight gradient) are rounded to bf16 and multiplied
                          on v_mfma_f32_32x32x16_bf16; accumulation, storage, norms, attention, losses stay fp32.
                          Also honoured by the inference entry points (sty_vocoder_fwd, sty_speech_fwd).              */
  int frozen;          /* 1: the model is one of a stage's eval_models (the speech predictor in train_textual,
                          stage_type.py:461): the backward produces input gradients only -- the weight-gradient GEMMs
                          of the dense convs are skipped and the bound parameter gradients must be ignored.          */
  float block_dropout; /* PitchEnergyPredictor only: nn.Dropout(model.yml pitch_energy_predictor.dropout = 0.2) between
                          the AdaIN + LeakyReLU and each conv of its eight AdaptiveDecoderBlocks
                          (pitch_energy_predictor.py:22,33-56; ada_norm.py:157,172-179).  Active with dropout_seed != 0;
                          the speech predictor's Decoder builds its blocks with the default 0 (decoder.py:19-35).    */
} sty_train_opts;
int sty_model_set_train_opts(sty_model *m, const sty_train_opts *opts);
/* fp32 split mode (bf16x3) of the inference entries, kind "speech_predictor" only (every other kind: STY_EINVAL, the kind named
 * in the error text): the 32 -> 32 channel convs the persistent kernel takes (the vocoder's AdaptiveGeneratorBlocks and prior /
 * output convs) split each fp32 operand into three bf16 pieces and multiply six pairs of pieces on the bf16 matrix cores, with
 * fp32 accumulation -- fp32 accuracy (the parity gates of the fp32 mode hold) on the bf16 matrix cores.  Every other conv keeps its
 * fp32 route.  Exclusive with the bf16 compute mode, never silently: refused (STY_EINVAL) while compute_bf16 is set, and
 * sty_model_set_train_opts(compute_bf16 = 1) is refused while the split is on.  Switching it on un-finalizes the model when the
 * weights' fragment triples still have to be packed (call sty_model_finalize again, as after sty_model_enable_training);
 * switching it off again needs nothing.  Read by sty_vocoder_fwd, sty_speech_fwd and sty_resblock_fwd; the training graph
 * (*_fwd_train, *_bwd) does not read it.                                                                                  */
int sty_model_set_fp32_split(sty_model *m, int on);

/* Data-parallel overlap: a callback the backward entry points invoke ON THE CALLING THREAD as soon as
 * a segment of the bound parameter gradients is final on `stream` (every later kernel of the same backward leaves it
 * alone), so that the caller can start that segment's all-reduce while the rest of the backward still runs.
 *   speech_predictor: segment 0 = every parameter outside `text_encoder.*` (announced before the text encoder's
 *                     backward), segment 1 = `text_encoder.*` (announced at the end of sty_speech_bwd);
 *   other kinds:      segment 0 = everything, announced at the end of the backward entry point.
 * Without a hook (one rank: nothing to overlap) no segment is announced early and sty_speech_bwd does not make the
 * calling stream wait for the library's weight-gradient stream in the middle of the backward.
 * Replaces what the reference gets from accelerate's DDP reducer hooks (train/train_context.py:94-104).          */
typedef void (*sty_grad_hook)(void *user, int segment);
int sty_model_set_grad_hook(sty_model *m, sty_grad_hook hook, void *user);
int sty_model_bind_grad(sty_model *m, const char *key, float *grad);
int sty_vocoder_train_workspace_bytes(sty_model *m, int B, int T, size_t *bytes);
int sty_vocoder_fwd_train(sty_model *m, const sty_vocoder_io *io, void *workspace, size_t ws_bytes, void *stream);
int sty_vocoder_bwd(sty_model *m, const float *d_audio, float *d_mel, float *d_style, void *stream);
/* Same for SpeechPredictor.forward (text encoder -> alignment expand -> decoder -> vocoder): gradients of every
 * parameter of the predictor, plus d loss / d style [B,64] and d loss / d energy [B,T] (each optional).      */
int sty_speech_train_workspace_bytes(sty_model *m, int B, int L, int T, size_t *bytes);
int sty_speech_fwd_train(sty_model *m, const sty_speech_io *io, void *workspace, size_t ws_bytes, void *stream);
int sty_speech_bwd(sty_model *m, const float *d_audio, float *d_style, float *d_energy, void *stream);
/* Optional: the weight-side half of the next sty_speech_fwd_train (weight-norm / packed weights, input-gradient packs, bf16
 * fragments) issued on `stream` ahead of time -- after the optimizer step that produced the parameters (train/stage.py:
 * 104-124 steps the optimizer at the end of train_batch); that forward then skips it and waits, on ITS stream, for an event
 * recorded behind this call.  The parameters must not change in between: the library cannot see an optimizer step (it runs
 * on flat buffers) -- sty_model_invalidate cancels the preparation and is the caller's statement that they did.          */
int sty_speech_prepare_train(sty_model *m, void *stream);
/* ... and d loss / d pitch [B,T] (the textual stage feeds the PREDICTED pitch and energy to the frozen speech predictor,
 * train/stage_type.py:139-160; the harmonic source and the voiced flag carry no gradient).  Any output may be NULL.   */
int sty_speech_bwd_pe(sty_model *m, const float *d_audio, float *d_style, float *d_pitch, float *d_energy, void *stream);
/* d_style of the last sty_speech_bwd is complete before the text encoder's backward has run: this makes `stream` wait
 * for exactly that point, so that the style encoder's backward can start on `stream` while the call's own stream still
 * works through the text encoder (AcousticTrainer does this).                                                    */
int sty_speech_d_style_ready(sty_model *m, void *stream);
/* Where the harmonic-prior branch of the last sty_speech_fwd_train ran (and its backward runs): io.style_stream when the
 * branch was issued beside the trunk AND its tape entries are marked for the backward to issue there too, NULL when it is
 * issued in place on the call's own stream (no style stream given, sty_set_single_stream(1)).  For tests and timelines. */
int sty_speech_branch_stream(sty_model *m, void **stream);
/* Same for MelStyleEncoder.forward: gradients of every parameter (through the eval-mode spectral norm
 * W/sigma(W) with fixed u, v: torch.nn.utils.spectral_norm, mel_style_encoder.py:67-152) from d loss / d style. */
int sty_style_train_workspace_bytes(sty_model *m, int B, int T, size_t *bytes);
int sty_style_fwd_train(sty_model *m, int B, int T, const float *mel, float *style, void *workspace, size_t ws_bytes,
                        void *stream);
int sty_style_bwd(sty_model *m, const float *d_style, void *stream);
/* Optional: the weight-side half of the next sty_style_fwd_train / sty_pitch_style_fwd_train (spectral-norm power
 * iteration of module.train(), normalised and packed weights) issued on `stream` ahead of time, e.g. while another stream
 * still computes the mel input; that forward then skips it (any stream: it waits for an event recorded behind this call).
 * The parameters and train opts must not change in between (sty_model_invalidate cancels it).                        */
int sty_style_prepare_train(sty_model *m, void *stream);
/* Parity taps of the last sty_style_fwd_train / sty_pitch_style_fwd_train: index 0 = the stem conv's output, 1..4 = the
 * ResBlk outputs (mel_style_encoder.py:96-118), 5 = the 5x5 head conv's output at every position (valid where the window
 * fits), 6..9 = the input of the second LeakyReLU of ResBlk 1..4 (mel_style_encoder.py:110-113).  grad = 0: the activation; grad = 1 (after sty_style_bwd): d loss / d activation.  Writes [B,C,H,W] (the library's
 * zero pad column removed) to dst and the dimensions to C, H, W; dst = NULL only reports the dimensions.             */
int sty_style_tap(sty_model *m, int index, int grad, float *dst, int *C, int *H, int *W, void *stream);
/* AcousticStep.pitch_loss for one curve (train/stage_type.py:236-262: smooth_l1(target, pred) + smooth_l1 of their first
 * differences, means): loss[0] = value; d_pred [B,T] += k * d loss / d pred with k = weight / (loss + 1e-9) when `normalize`
 * (LossLog.backwards_loss, train/loss_log.py:82-94) or k = weight.  workspace: 16 bytes.                               */
int sty_pitch_loss_fwd_bwd(int B, int T, const float *target, const float *pred, float weight, int normalize,
                           float *loss, float *d_pred, void *workspace, size_t ws_bytes, void *stream);
/* Duration stage losses (train_duration, train/stage_type.py:495-556).
 * sty_prediction_to_duration: DurationProcessor.prediction_to_duration (train/utils.py:745-750): pred [B,L,NC] ->
 *   duration [B,L] = mask * sum_c softmax(pred)_c class_table_c / (sum_c softmax_c + 1e-9).
 * sty_duration_loss_fwd_bwd: losses[0] = mean over items of smooth_l1(duration[:len], target_dur[:len]) ("duration"),
 *   losses[1] = mean over items of CrossEntropy(pred[:len], target_class[:len], weight = ce_weight) ("duration_ce",
 *   DurationLoss, train/losses.py:430-446); d_pred [B,L,NC] = gradient of w_duration * duration / duration.detach() +
 *   w_ce * ce / ce.detach() (LossLog.backwards_loss) plus d_duration_extra [B,L] (e.g. the generator-side gradient of
 *   dur_disc; may be NULL) carried through prediction_to_duration.  workspace: 16 + 4 B bytes.                          */
int sty_prediction_to_duration(int B, int L, int NC, const float *pred, const int64_t *text_lengths,
                               const float *class_table, float *duration, void *stream);
int sty_duration_loss_fwd_bwd(int B, int L, int NC, const float *pred, const int64_t *text_lengths,
                              const float *target_dur, const int64_t *target_class, const float *class_table,
                              const float *ce_weight, float w_duration, float w_ce, const float *d_duration_extra,
                              float *losses, float *d_pred, void *workspace, size_t ws_bytes, void *stream);
/* DurationPredictor (duration_predictor.py:58-87) in the training graph: forward -> out [B,L,classes]; backward from
 * d_out adds the parameter gradients and writes d_style [B,64] (may be NULL).                                            */
int sty_duration_train_workspace_bytes(sty_model *m, int B, int L, size_t *bytes);
int sty_duration_fwd_train(sty_model *m, int B, int L, const int64_t *texts, const int64_t *text_lengths,
                           const float *style, float *out, void *workspace, size_t ws_bytes, void *stream);
int sty_duration_bwd(sty_model *m, const float *d_out, float *d_style, void *stream);
/* PitchEnergyPredictor (pitch_energy_predictor.py:62-82) in the training graph: forward -> pitch, energy [B,T]; backward
 * from d_pitch, d_energy [B,T] adds the parameter gradients and writes d_style [B,64] (may be NULL).                    */
int sty_pitch_energy_train_workspace_bytes(sty_model *m, int B, int L, int T, size_t *bytes);
int sty_pitch_energy_fwd_train(sty_model *m, int B, int L, int T, const int64_t *texts, const int64_t *text_lengths,
                               const float *alignment, const float *style, float *pitch, float *energy, void *workspace,
                               size_t ws_bytes, void *stream);
int sty_pitch_energy_bwd(sty_model *m, const float *d_pitch, const float *d_energy, float *d_style, void *stream);
/* PitchStyleEncoder (mel_style_encoder.py:155-205, the second-stage `pe_style_encoder`) in the training graph: forward, then
 * sty_style_bwd; x [B,dim_in,T], pitch, energy [B,T] are data (no gradient), parameter gradients as for the other kinds.   */
int sty_pitch_style_train_workspace_bytes(sty_model *m, int B, int T, size_t *bytes);
int sty_pitch_style_fwd_train(sty_model *m, int B, int T, const float *mel, const float *pitch, const float *energy,
                              float *style, void *workspace, size_t ws_bytes, void *stream);

/* ---- one dense Conv1d ('same' padding, torch.nn.functional.conv1d semantics) on the MFMA implicit-GEMM kernel every
 * conv / Linear of the path runs on; for unit parity tests and kernel tuning.  x [B,Cin,T], w [Cout,Cin,K],
 * bias [Cout] or NULL -> y [B,Cout,T].  (K-1)*dil <= 128.                                                     */
int sty_conv1d_workspace_bytes(int Cout, int Cin, int K, size_t *bytes);
/* compute_bf16 of sty_conv1d_fwd: 0 = fp32 operands; 1 = bf16 operands; 2 = bf16 operand twins (the input's twin made here, the
 * output's written behind the workspace); 3 is taken by sty_conv1d_bwd (x is a two-byte tensor) and means bf16 operands here;
 * 4 = the fp32 split mode (bf16x3: every fp32 operand as three bf16 pieces, six products per k-step on the bf16 matrix cores,
 * fp32 accuracy) where the conv is eligible for it (a 32 -> 32 channel conv on the persistent kernel) and the fp32 route
 * elsewhere; the fragment triples are packed into the workspace, which sty_conv1d_workspace_bytes sizes for them.
 * sty_conv1d_route with 4 answers STY_CONV_32P for an eligible shape and what 0 answers for every other.  sty_conv1d_fwd and
 * sty_conv1d_route alone know mode 4: sty_conv1d_fwd_ex and sty_conv1d_fwd_shuffle take 0 or 1 and refuse everything else,
 * sty_conv1d_bwd treats every other nonzero value as bf16.                                                                  */
int sty_conv1d_fwd(int B, int Cin, int Cout, int K, int dil, int T, const float *x, const float *w, const float *bias,
                   float *y, void *workspace, size_t ws_bytes, int compute_bf16, void *stream);
/* The same conv with the fused prologue and output stage of the text encoder's convs: x * in_mask[b,t] in front (in_mask [B,T] or
 * NULL), then y = relu?(conv + bias) * out_mask (before the residual, or behind it with out_mask_post) + residual; every tensor
 * fp32, compute_bf16 0 or 1.                                                                                              */
int sty_conv1d_fwd_ex(int B, int Cin, int Cout, int K, int dil, int T, const float *x, const float *w, const float *bias,
                      const float *in_mask, const float *residual, const float *out_mask, int out_mask_post, int relu,
                      float *y, void *workspace, size_t ws_bytes, int compute_bf16, void *stream);
/* The generator's pixel-shuffle up-sampling conv (generator.py:731-780): the same conv with the output stored shuffled,
 * y [B, Cout / shuffle, T * shuffle] with y[b][co / shuffle][t * shuffle + co % shuffle]; Cout % shuffle == 0; compute_bf16 0 / 1. */
int sty_conv1d_fwd_shuffle(int B, int Cin, int Cout, int K, int dil, int T, int shuffle, const float *x, const float *w,
                           const float *bias, float *y, void *workspace, size_t ws_bytes, int compute_bf16, void *stream);
/* Which kernel family the dispatch picks for a conv of this shape carrying the operands named in `flags` (host only, nothing is
 * launched): *kernel = position in the dispatch order's list of families (STY_CONV_*), -1 where the conv is refused.
 * STY_ROUTE_FLAT_IMAGE: the conv is a 3-row 2-D conv in flat-image mode (the discriminators' layout): Cin = 3 * the image's
 * channels, T = rows * row pitch (the pitch itself does not enter the choice).                                            */
enum { STY_ROUTE_IN_MASK = 1, STY_ROUTE_RESIDUAL = 2, STY_ROUTE_OUT_MASK = 4, STY_ROUTE_RELU = 8, STY_ROUTE_TWO_BYTE_X = 16,
       STY_ROUTE_STATS = 32, STY_ROUTE_Y16 = 64, STY_ROUTE_X16 = 128, STY_ROUTE_FLAT_IMAGE = 256,
       /* the output is stored pixel-shuffled / the source is (the input-gradient conv of such a layer): the factor, 2 .. 15, goes
        * into flags as well, factor << STY_ROUTE_SHUFFLE_SHIFT */
       STY_ROUTE_SHUFFLE_STORE = 512, STY_ROUTE_SHUFFLE_SOURCE = 1024, STY_ROUTE_SHUFFLE_SHIFT = 16 };
enum { STY_CONV_STEM2D = 0, STY_CONV_32P, STY_CONV_SC, STY_CONV_K1, STY_CONV_Q, STY_CONV_P16, STY_CONV_TILED };
int sty_conv1d_route(int B, int Cin, int Cout, int K, int dil, int T, int compute_bf16, int flags, int *kernel);
/* Gradients of the same conv on the kernels the training graph uses: dw [Cout,Cin,K] and dbias [Cout] (or NULL) from
 * (x, gy [B,Cout,T]) on the weight-gradient kernels (wgrad.hip), dx [B,Cin,T] (or NULL) on the implicit-GEMM kernel
 * with the flipped weights.  compute_bf16 as in sty_train_opts; 3: bf16 mode with x a bf16 tensor [B,Cin,T] (two-byte
 * storage; dw / dbias only, dx NULL, T even), as the many-tap 32-channel weight gradient reads the 75T-rate activations.
 * sty_conv1d_bwd_workspace_bytes takes no mode: its figure covers every compute_bf16 value, 3 included.                */
int sty_conv1d_bwd_workspace_bytes(int B, int Cin, int Cout, int K, int T, size_t *bytes);
int sty_conv1d_bwd(int B, int Cin, int Cout, int K, int dil, int T, const float *x, const float *w, const float *gy,
                   float *dw, float *dbias, float *dx, void *workspace, size_t ws_bytes, int compute_bf16,
                   void *stream);
/* The gradients of sty_conv1d_fwd_shuffle from gy [B, Cout / shuffle, T * shuffle], the gradient of the shuffled output, as the
 * training graph computes them: dw, dbias as above, dx (or NULL) by the input-gradient conv reading the shuffled gradient;
 * accumulate != 0: dx += (the conv takes dx as its residual operand).  Workspace: sty_conv1d_bwd_workspace_bytes; compute_bf16 0 / 1. */
int sty_conv1d_bwd_shuffle(int B, int Cin, int Cout, int K, int dil, int T, int shuffle, const float *x, const float *w,
                           const float *gy, float *dw, float *dbias, float *dx, int accumulate, void *workspace, size_t ws_bytes,
                           int compute_bf16, void *stream);
/* The second stage of the two-stage reductions (bias gradient of a dense conv, weight / bias gradient of a depthwise conv)
 * alone, for unit tests: fixed-order float64 sums of nblk partials per output.  dw_form == 0: part [C][nblk] -> db[c] +=;
 * dw_form != 0: part [C][nblk][K+1] -> dw[c][k] += (k < K), db[c] += (k == K).                                      */
int sty_partial_sum(int dw_form, const float *part, int C, int K, int nblk, float *dw, float *db, void *stream);

/* ---- optimizer: torch.optim.AdamW (train/optimizers.py:110-118) over one flat fp32 bucket ------------------
 * p, g, m, v: n floats each, 16-byte aligned, identically laid out; step = 1, 2, ... (bias correction).
 * grad_scale multiplies g on the way in: 1 / world_size turns the SUM all-reduce of the gradient buckets into the
 * mean without a pass of its own (1.0f: plain AdamW, bit-identical).  The betas are doubles: 1 - beta and the bias
 * corrections are formed in double, as torch forms them (1.0f - 0.99f is 9.5e-7 off 0.01).                        */
int sty_adamw_step(size_t n, float *p, const float *g, float *m, float *v, float lr, double beta1, double beta2,
                   float eps, float weight_decay, int step, float grad_scale, void *stream);
/* The same step at the rate lr * *lr_mult, lr_mult a DEVICE double: the discriminators' learning-rate multiplier
 * (train/optimizers.py:54-65) never leaves the GPU, so a GAN step has no host read-back.  sty_disc_lr_track keeps it:
 * state (DEVICE double[2]) = { last_loss, multiplier }; one call writes state[1] = get_disc_lr_multiplier() of the
 * current last_loss (train/losses.py:241-256) and THEN folds *loss (DEVICE float, may be NULL: multiplier only) into the
 * running mean, last_loss = 0.95 last_loss + 0.05 loss (losses.py:287) -- the order of train/stage.py, where the optimizer
 * steps with the multiplier of the previous mean.                                                                  */
int sty_adamw_step_scaled(size_t n, float *p, const float *g, float *m, float *v, double lr, const double *lr_mult,
                          double beta1, double beta2, float eps, float weight_decay, int step, float grad_scale,
                          void *stream);
int sty_disc_lr_track(double *state, const float *loss, double ideal_loss, double f_max, double h_min, double x_max,
                      double x_min, void *stream);

/* ---- acoustic-stage losses without third-party models, forward + backward in one call ---------------
 * mel  = MultiResolutionSTFTLoss (train/losses.py:17-38) on log1p(mel128|X|); multi_phase = losses.py:41-91;
 * seed = w_mel*mel/(mel.detach()+1e-9) + w_phase*multi_phase/(multi_phase.detach()+1e-9)  (loss_log.py:82-94).
 * audio_gt, audio_pred [B,N] -> losses[2] (device: mel, multi_phase), d_audio_pred [B,N] = d seed / d audio_pred. */
int sty_acoustic_loss_workspace_bytes(int B, int N, size_t *bytes);
/* Optional: the TARGET side of the loss features (the three STFT resolutions of audio_gt, multi_spectrogram.py:57-66 under
 * no_grad) depends on data only.  sty_acoustic_loss_target computes it into `workspace` ahead of time -- e.g. on the main
 * stream while it waits for the style encoder -- and a later sty_acoustic_loss_fwd_bwd / sty_acoustic_gan_loss_fwd_bwd with
 * the SAME workspace, B and N and audio_gt = NULL uses it instead of recomputing it.                              */
int sty_acoustic_loss_target(int B, int N, const float *audio_gt, void *workspace, size_t ws_bytes, void *stream);
int sty_acoustic_loss_fwd_bwd(int B, int N, const float *audio_gt, const float *audio_pred, float w_mel,
                              float w_phase, float *losses, float *d_audio_pred, void *workspace, size_t ws_bytes,
                              void *stream);

/* ---- forward-only loss values for the validation pass (validate_acoustic / _textual / _duration,
 * train/stage_type.py:376-633; csrc/val_loss.hip) ---------------
 * The values the three *_fwd_bwd entries above log, without a gradient buffer and with FIXED-ORDER reductions: every
 * workgroup stores its float64 partial at its own index, one finalize workgroup adds them in index order, no atomics; the
 * partial count depends on the shape alone.  Two calls on the same buffers give equal bits (a validation loss is compared
 * against manifest.best_loss across passes).
 * sty_mel_loss_fwd: the "mel" term alone (MultiResolutionSTFTLoss, train/losses.py:17-38) on the three log1p(mel128|X|)
 *   tensors sty_acoustic_loss_fwd_bwd compares (the same feature launches; no phase, no backward tensors):
 *   loss[0] = mean over the three resolutions of sum|t - p| / (sum|t| + 1e-6).  per_item [B][3][2] doubles or NULL: every
 *   utterance's own (sum|t - p|, sum|t|) per resolution; their sums over B are the sums loss[0] is made of.  N > 1024.
 * sty_mel_loss_features (host only): where sty_mel_loss_fwd leaves the features in its workspace -- byte offset of
 *   resolution 0..2, side 0 (target) / 1 (prediction), a float tensor [128][B][frames] -- so that a caller can read what was
 *   reduced.
 * sty_pitch_loss_fwd: the value of sty_pitch_loss_fwd_bwd for one [B,T] curve.  workspace: 16 B bytes.
 * sty_duration_loss_fwd: losses[0..1] as sty_duration_loss_fwd_bwd defines them.  workspace: 16 B bytes.                */
int sty_mel_loss_workspace_bytes(int B, int N, size_t *bytes);
int sty_mel_loss_features(int B, int N, int resolution, int side, size_t *offset_bytes, int *frames);
int sty_mel_loss_fwd(int B, int N, const float *audio_gt, const float *audio_pred, float *loss, double *per_item,
                     void *workspace, size_t ws_bytes, void *stream);
int sty_pitch_loss_fwd(int B, int T, const float *target, const float *pred, float *loss, void *workspace,
                       size_t ws_bytes, void *stream);
int sty_duration_loss_fwd(int B, int L, int NC, const float *pred, const int64_t *text_lengths, const float *target_dur,
                          const int64_t *target_class, const float *class_table, const float *ce_weight, float *losses,
                          void *workspace, size_t ws_bytes, void *stream);

/* ---- slm loss value (WavLMLoss, train/losses.py:376-394; csrc/wavlm.hip; stylish_tts_amd/slm.py) -----------------------
 * Model kind "wavlm" = transformers' WavLMModel in eval mode (no dropout, SpecAugment or LayerDrop), bound by the keys of
 * WavLMModel.state_dict() without masked_spec_embed: feature_extractor.conv_layers.I.conv.weight, ...0.layer_norm.*,
 * feature_projection.{layer_norm, projection}.*, encoder.pos_conv_embed.conv.{bias, parametrizations.weight.original0/1},
 * encoder.layer_norm.*, encoder.layers.L.{attention.{q,k,v,out}_proj, attention.gru_rel_pos_linear, layer_norm,
 * feed_forward.{intermediate_dense, output_dense}, final_layer_norm}.*, ...attention.gru_rel_pos_const and
 * encoder.layers.0.attention.rel_attn_embed.weight.  Widths, depths, heads, kernels, groups and num_buckets are read from
 * the bound shapes; what no shape shows (the conv strides, max_bucket_distance, layer_norm_eps) comes from
 * sty_wavlm_set_config, called before sty_model_finalize.  Built: feat_extract_norm "group", do_stable_layer_norm false,
 * conv_bias false, exact GELU.  Frozen; fp32 operands on the fp32 matrix cores unless sty_wavlm_set_compute says bf16: the
 * compute_bf16 of sty_model_set_train_opts, sty_model_enable_training and sty_model_bind_grad return STY_EINVAL for this kind (the
 * gradient with respect to the wave is built, see below; no weight gradient is).
 * Resampler: torchaudio.transforms.Resample(orig, new) with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff
 * 0.99) restated from the documented closed form -- torchaudio is no dependency: PARITY UNPINNED at this boundary.  The rates are
 * reduced by their gcd (24000 -> 16000 is 3 -> 2: two phases of 23 taps at stride 3); sty_slm_resample_len = ceil(N new /
 * orig).  sty_slm_resample_kernel_host: the table [new][2 width + orig], width = ceil(6 orig / (0.99 min(orig, new))) in
 * reduced rates, HOST memory, evaluated in double and rounded once; returns the number of floats (out may be NULL).
 * sty_wavlm_frames: frames T of N16 samples, floor((n - k) / s) + 1 per conv layer; no frame left: STY_ESHAPE.
 * sty_wavlm_fwd: audio16 [B,N16] -> hidden [layers + 1, B, T, hidden_size]: [0] = the encoder's input after the positional
 * conv and LayerNorm, [i] = the output of layer i (the tuple output_hidden_states=True returns).
 * sty_wavlm_rel_buckets_host: _relative_positions_bucket of the distances -(T - 1) .. T - 1 (HOST memory).
 * sty_slm_loss_fwd: loss[0] = mean |a - b| over n floats, float64 partials added in index order (two calls, equal bits). */
int sty_wavlm_set_config(sty_model *m, int n_conv, const int *conv_stride, int max_bucket_distance, float layer_norm_eps);
/* sty_wavlm_set_compute: the kind's operand mode, 0 = fp32 (the default), 1 = bf16: the dense contractions and, at head dim 64, the
 *   attention's products round both operands to bf16 (RNE) and run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; everything
 *   returned or kept stays fp32 (DESIGN.md section 4.24 lists the rounding points).  Kind "wavlm" and values 0 / 1 only (STY_EINVAL
 *   otherwise); callable before or after finalize and between calls, nothing is re-packed.  The workspace queries answer for the
 *   current mode; a sty_wavlm_bwd in another mode than its sty_wavlm_fwd_keep returns STY_ESTATE. */
int sty_wavlm_set_compute(sty_model *m, int bf16);
int sty_slm_resample_len(int N, int orig, int new_rate);
int sty_slm_resample_kernel_host(int orig, int new_rate, float *out);
int sty_slm_resample_fwd(int B, int N, int orig, int new_rate, const float *audio, float *out, void *stream);
int sty_wavlm_frames(const sty_model *m, int N16, int *T);
int sty_wavlm_workspace_bytes(const sty_model *m, int B, int N16, size_t *bytes);
int sty_wavlm_fwd(sty_model *m, int B, int N16, const float *audio16, float *hidden, void *workspace, size_t ws_bytes,
                  void *stream);
int sty_wavlm_rel_buckets_host(int T, int num_buckets, int max_distance, int32_t *out);
int sty_slm_loss_workspace_bytes(size_t n, size_t *bytes);
int sty_slm_loss_fwd(size_t n, const float *a, const float *b, float *loss, void *workspace, size_t ws_bytes, void *stream);
/* The gradient of the slm term with respect to the predicted wave: the input-gradient chain of the frozen network.  No kernel
 * of it uses a float atomic: the same inputs give the same bits, in default and deterministic mode alike.
 * sty_wavlm_fwd_keep: the hidden states of sty_wavlm_fwd, bit for bit, keeping in the workspace what the backward reads (every
 *   layer's inputs, pre-activations, q / k / v / o and the attention's row log-sum-exp; nothing is recomputed).  The workspace
 *   is sized by sty_wavlm_grad_workspace_bytes and must stay untouched until sty_wavlm_bwd.
 * sty_wavlm_bwd: d_hidden [layers + 1, B, T, hidden_size] (the cotangent of the stack) -> d_audio16 [B, N16], written whole
 *   (samples no frame reads get 0); d_enc_in (optional, [B, hidden_size, T]): the gradient at the feature projection's output, in
 *   front of the positional conv.  Consumes the workspace of the sty_wavlm_fwd_keep call before it: without one STY_ESTATE,
 *   another (B, N16) or workspace STY_ESHAPE, a workspace too small STY_ENOMEM -- all refused on the host, nothing launched.
 * sty_slm_loss_fwd_bwd: loss as sty_slm_loss_fwd (the same bits) and d_b[i] = scale * sign(b[i] - a[i]) / n, 0 at a tie.
 * sty_slm_resample_bwd: the adjoint of sty_slm_resample_fwd, d_out [B, ceil(N new / orig)] -> d_audio [B, N]; accumulate != 0:
 *   d_audio[i] = d_audio[i] + g[i] in one fp32 add. */
int sty_wavlm_grad_workspace_bytes(const sty_model *m, int B, int N16, size_t *bytes);
int sty_wavlm_fwd_keep(sty_model *m, int B, int N16, const float *audio16, float *hidden, void *workspace, size_t ws_bytes,
                       void *stream);
int sty_wavlm_bwd(sty_model *m, int B, int N16, const float *d_hidden, float *d_audio16, float *d_enc_in, void *workspace,
                  size_t ws_bytes, void *stream);
/* One strided feature conv alone (Conv1d(Cin, Cout, k, stride s), bias-free), forward and input gradient, through the stage +
 * conv and dgrad + un-stage launches the plan makes for it in the mode asked for: x [B, Cin, Nin] a pre-activation, w [Cout, Cin, k]
 * -> y = conv(GELU(x)) [B, Cout, T], T = (Nin - k) / s + 1; gy [B, Cout, T] -> dx [B, Cin, Nin] = GELU'(x) * conv^T(gy), zero where no
 * frame reads.  view (optional, fp32 [B, s Cin, T + ceil(k / s) - 1]): the phase-major view the fp32 mode stages; view16 (optional,
 * bf16, the same shape; compute_bf16 = 1 on a twin family only): the operand twin the bf16 mode stages in its place.  routes
 * (optional, int[4], HOST): kernel family of the conv and of the transposed conv (sty_conv1d_route's numbers), and whether each read
 * a bf16 twin. */
int sty_wavlm_strided_conv_workspace_bytes(int B, int Cin, int Cout, int k, int s, int Nin, size_t *bytes);
int sty_wavlm_strided_conv_fwd_bwd(int B, int Cin, int Cout, int k, int s, int Nin, const float *x, const float *w, int compute_bf16,
                                   float *y, const float *gy, float *dx, float *view, void *view16, int *routes, void *workspace,
                                   size_t ws_bytes, void *stream);
int sty_slm_loss_fwd_bwd(size_t n, const float *a, const float *b, float scale, float *loss, float *d_b, void *workspace,
                         size_t ws_bytes, void *stream);
int sty_slm_resample_bwd(int B, int N, int orig, int new_rate, const float *d_out, float *d_audio, int accumulate, void *stream);

/* ---- adversarial terms of the acoustic stage: spectrogram discriminators ---------------
 * SpecDiscriminator (train/models/discriminator.py:13-68): five weight-normed Conv2d 3x9 / 3x3 with LeakyReLU(0.1),
 * a weight-normed 3x3 score conv after each.  Parameters by reference key: index i = 0..4 is `discriminators.i`,
 * 5 + i is `out.i`; g = parametrizations.weight.original0 [Cout,1,1,1], v = ...original1 [Cout,Cin,KH,KW], bias.  */
typedef struct {
  const float *g[10];
  const float *v[10];
  const float *bias[10];
} sty_specdisc_params;
typedef struct { /* gradients, same shapes; the calls ADD into them */
  float *g[10];
  float *v[10];
  float *bias[10];
} sty_specdisc_grads;
/* W1 = ceil(W/2), W2 = ceil(W1/2), W3 = ceil(W2/2): the five score maps have H*W, H*W1, H*W2, H*W3, H*W3 elements
 * per batch item; `scores` buffers hold them back to back, each [B][H*Wi] (torch.flatten(out, 1, -1) of the module). */
int sty_specdisc_workspace_bytes(int B, int H, int W, int with_grads, size_t *bytes);
/* SpecDiscriminator.forward: x [B,1,H,W] (H = frequency bins, W = frames) -> the five score maps.                   */
int sty_specdisc_forward(const sty_specdisc_params *p, int B, int H, int W, const float *x, float *scores,
                         int compute_bf16, void *workspace, size_t ws_bytes, void *stream);
/* GeneratorLossHelper.forward + backward (train/losses.py:330-373) and / or DiscriminatorLossHelper.forward + backward
 * (train/losses.py:228-290) of ONE discriminator on target, pred [B,1,H,W], from a single forward pass (both helpers
 * see the same weights and tensors in the reference's step, train/stage.py:104-147):
 *   gen_loss[0] += loss;  d_pred [B,H,W] += gen_scale * d loss / d pred            (either may be NULL; both NULL: skipped)
 *   disc_loss[0] += loss, disc_loss[1] += loss without the relativistic term (what DiscriminatorLossHelper.last_loss
 *   tracks);  grads += disc_scale * d loss / d parameters                           (likewise)                          */
int sty_specdisc_losses(const sty_specdisc_params *p, int B, int H, int W, const float *target, const float *pred,
                        float gen_scale, float *gen_loss, float *d_pred, float disc_scale, float *disc_loss,
                        const sty_specdisc_grads *grads, int compute_bf16, void *workspace, size_t ws_bytes,
                        void *stream);

/* PitchDiscriminator (train/models/pitch_discriminator.py:6-68; `pitch_disc`: dim_in 2, kernel 21; `dur_disc`: dim_in 1,
 * kernel 5): the 1-D sibling of SpecDiscriminator with the same parameter table (g, v, bias of `discriminators.0..4` and
 * `out.0..4`).  x [B, dim_in, T] -> five score maps [B, T] back to back; losses as sty_specdisc_losses (d_pred [B,dim_in,T]). */
int sty_pitchdisc_workspace_bytes(int B, int dim_in, int kernel, int T, int with_grads, size_t *bytes);
int sty_pitchdisc_forward(const sty_specdisc_params *p, int B, int dim_in, int kernel, int T, const float *x,
                          float *scores, void *workspace, size_t ws_bytes, void *stream);
int sty_pitchdisc_losses(const sty_specdisc_params *p, int B, int dim_in, int kernel, int T, const float *target,
                         const float *pred, float gen_scale, float *gen_loss, float *d_pred, float disc_scale,
                         float *disc_loss, const sty_specdisc_grads *grads, void *workspace, size_t ws_bytes,
                         void *stream);

/* ContextFreeDiscriminator (train/models/discriminator.py:91-177), the waveform discriminator `disc`, in training mode
 * (BatchNorm batch statistics; running_mean / running_var are updated in place with `bn_momentum` on every forward).
 * conv index: 0-3 `conv.i.net.0`, 4-5 `temporal.i.net.0`, 6-7 `spectral.i.net.0`, 8 `fusion.net.0`, 9 `attn.1`, 10 `last.0`,
 * 11 `last.2` (conv_b NULL for 0-3: bias=False); bn index 0-8: the `.net.1` BatchNorm1d of the same nine blocks.          */
typedef struct {
  const float *conv_w[12];
  const float *conv_b[12];
  const float *bn_w[9];
  const float *bn_b[9];
  float *bn_rm[9];
  float *bn_rv[9];
} sty_cfdisc_params;
typedef struct { /* gradients, same shapes; the calls ADD into them */
  float *conv_w[12];
  float *conv_b[12];
  float *bn_w[9];
  float *bn_b[9];
} sty_cfdisc_grads;
/* x [B,N] (N >= 1024) -> scores [B, t*16], t = (N - 1024) / 512 + 1 windows ("b (t c f)" of the module's forward).     */
int sty_cfdisc_workspace_bytes(int B, int N, int with_grads, size_t *bytes);
int sty_cfdisc_forward(const sty_cfdisc_params *p, int B, int N, const float *x, float *scores, float bn_momentum,
                       int compute_bf16, void *workspace, size_t ws_bytes, void *stream);
/* Both loss helpers on (target, pred) [B,N] from one forward pass of each, as sty_specdisc_losses.                     */
int sty_cfdisc_losses(const sty_cfdisc_params *p, int B, int N, const float *target, const float *pred, float gen_scale,
                      float *gen_loss, float *d_pred, float disc_scale, float *disc_loss, const sty_cfdisc_grads *grads,
                      float bn_momentum, int compute_bf16, void *workspace, size_t ws_bytes, void *stream);

/* The acoustic losses WITH the adversarial term of the three spectrogram discriminators (AcousticStep.generator_loss,
 * train/stage_type.py:208-220, "mrd" part of GeneratorLoss / DiscriminatorLoss, train/losses.py:191-208, 313-327; the
 * waveform discriminator `disc` adds into the same d_audio_pred through sty_cfdisc_losses): as sty_acoustic_loss_fwd_bwd, plus
 *   d_audio_pred += w_gen * d (sum_r GeneratorLossHelper_r(target_fft_r, pred_fft_r)) / d audio_pred   (the "generator"
 *   loss enters LossLog.backwards_loss un-normalised, train/loss_log.py:84-86), and, from the same forward pass,
 *   the discriminator-side loss of every resolution; mrd_grads[r] += disc_scale * its parameter gradients for the
 *   resolutions whose bit is set in step_mask (the reference steps mrd{disc_index} only, train/stage.py:139-141).
 * mrd, mrd_grads: arrays of 3 (mrd0..2 = resolutions fft 512 / 1024 / 2048).  gan_losses: device [7] = generator loss
 * summed over the three, then (discriminator loss, the same without the relativistic term) per resolution.          */
int sty_acoustic_gan_workspace_bytes(int B, int N, int with_grads, size_t *bytes);
int sty_acoustic_gan_loss_fwd_bwd(int B, int N, const float *audio_gt, const float *audio_pred, float w_mel,
                                  float w_phase, float w_gen, const sty_specdisc_params *mrd, float disc_scale,
                                  const sty_specdisc_grads *mrd_grads, int step_mask, float *losses, float *gan_losses,
                                  float *d_audio_pred, void *workspace, size_t ws_bytes, void *gan_workspace,
                                  size_t gan_ws_bytes, int compute_bf16, void *stream);

/* ---- gradient exchange of the data-parallel step ---------------------------------------------
 * Replaces what the reference gets from accelerate's per-module DDP wrappers (train/train_context.py:94-104,
 * train/train.py:208-211: bucketed gradient all-reduce over NCCL): one communicator per process (one process per GPU) over
 * RCCL, on a HIP stream the LIBRARY owns.  The rank that calls sty_comm_unique_id hands the 128 bytes to the others by any
 * side channel (stylish_tts_amd/dist.py: one broadcast through torch.distributed), every rank then calls sty_comm_init
 * (collective: it returns when all `world` ranks have called it).  stream_priority: < 0 the runtime's greatest priority, 0
 * priority 0, > 0 its least priority (hipDeviceGetStreamPriorityRange; -1 / 1 on MI355X).
 * sty_comm_allreduce_bucket(buf, n): buf[0..n) := sum over ranks, in place, asynchronously on the communicator's stream, ordered
 * BEHIND everything `producer_stream` holds at the time of the call; as ncclReduceScatter + ncclAllGather when n is a multiple
 * of 4 * world, ncclAllReduce otherwise.  sty_comm_wait makes `consumer_stream` wait for every bucket handed over so far (no
 * host synchronisation).  RCCL is resolved with dlopen at the first call (STY_RCCL_LIB overrides the name).               */
typedef struct sty_comm sty_comm;
int sty_comm_unique_id(void *id128);
int sty_comm_init(const void *id128, int rank, int world, int stream_priority, sty_comm **out);
int sty_comm_allreduce_bucket(sty_comm *c, float *buf, size_t n, void *producer_stream);
int sty_comm_wait(sty_comm *c, void *consumer_stream);
/* Run the collectives on a stream of the CALLER's instead (it stays the caller's; it must outlive the communicator's use). */
int sty_comm_set_stream(sty_comm *c, void *stream);
int sty_comm_stats(sty_comm *c, uint64_t *buckets, uint64_t *reduce_scatter_all_gather, double *bytes);
int sty_comm_destroy(sty_comm *c);

/* ---- the static voicepack's table (train/voicepack.py:116-136 `make_static`) -----------------------------------------
 * sty_pack_accumulate replaces `styles[length.item() - 1].append(combined)` (voicepack.py:118-122) for a whole batch:
 * row i of styles [n][D] is added to bucket text_lengths[i] - 1 of sums [rows][D] (float64) and counts [rows] is
 * incremented; all buffers on the device, the caller zeroes sums / counts before the first call.  The rows of one bucket
 * are added in row order by one thread per column, with no float atomics: the same calls give the same bits.  A length
 * outside 1..rows is the caller's to refuse on the host (before upload); such a row is not added.
 * sty_pack_finalize replaces `torch.stack(sum(styles[lower:upper], []), 0).mean(0)` per row of the pack
 * (voicepack.py:131-135): pack[i] = (sum of sums[b] for b in [lo[i], hi[i]) ascending) / (sum of counts[b]), one division
 * and one rounding to fp32.  lo / hi [rows] (device): the windows as a Python slice normalises them, resolved on the host
 * from `counts` (stylish_tts_amd/voicepack.py resolve_windows, voicepack.py:124-130).  A window without rows gives NaN. */
int sty_pack_accumulate(int n, int D, int rows, const float *styles, const int64_t *text_lengths, double *sums,
                        int64_t *counts, void *stream);
int sty_pack_finalize(int rows, int D, const double *sums, const int64_t *counts, const int32_t *lo, const int32_t *hi,
                      float *pack, void *stream);

/* ---- in-situ kernel timing (used by bench.py for the roofline object) --------------------------------
 * When enabled, every launch of the instrumented kernel families is bracketed by HIP events on the launch
 * stream.  sty_prof_report synchronises the device, sums the event times per family and writes up to `cap`
 * rows; it returns the number of families.  flops/bytes are ALGORITHMIC counts computed from the launch shapes
 * (DESIGN.md section "roofline accounting"), not counter readings.                                       */
typedef struct {
  char name[48];   /* family: the launch site's label (kernel name, tile parameter, bf16 marker) */
  char inst[144];  /* the instantiation that ran, as rocprofv3 --kernel-trace prints it minus "void sty::" and the argument
                      list, e.g. "convp16_kernel<2, 0, 0, true, true>" (one row per (family, inst) pair) */
  uint64_t launches;
  double ms;    /* summed launch durations */
  double flops; /* summed algorithmic flops */
  double bytes; /* summed algorithmic HBM bytes (each operand tensor read once, each result written once) */
} sty_prof_row;
int sty_prof_enable(int on);
/* Restrict the timing to one kernel family (its name as sty_prof_report prints it); NULL or "" = all.  Two events
 * per launch on ~700 launches cost ~7 % of a c2 training step; bench.py times every family during warm-up, then only
 * the dominant one inside the timed region.                                                                      */
int sty_prof_only(const char *family);
/* Measurement aid: 1 = the training entry points use no internal side stream (weight gradients run in line).  Kernel
 * durations measured that way are free of the stretch from sharing the chip with another stream.  The workspace must
 * have been sized in the same mode it is used in (call before sty_*_train_workspace_bytes).                        */
int sty_set_single_stream(int on);
/* Deterministic mode (process-wide, default 0): 1 = every sum whose result depends on the order in which atomics arrive
 * (parameter gradients summed over the batch, d style, the embedding scatter, the style head, the double-precision loss
 * and BatchNorm sums of the losses and discriminators) takes a fixed-order path: partial slots and an in-order sum.  Two
 * runs of a training step on the same inputs then give the same bits.  The mode is latched by each sty_*_fwd_train call
 * (by the call itself where forward and backward are one call): a backward runs in the mode of its forward, whatever the
 * switch says by then.  sty_*_workspace_bytes return the figure of the current mode (mode 1 adds the slots); a training
 * forward given less than its mode needs returns STY_ENOMEM before anything is launched.  Mode 0 launches exactly what the
 * library launched before the switch existed.  Nothing is claimed about the order of a gradient exchange between ranks. */
int sty_set_deterministic(int on);
int sty_get_deterministic(void);
int sty_prof_report(sty_prof_row *rows, int cap);

#ifdef __cplusplus
}
#endif
#endif
