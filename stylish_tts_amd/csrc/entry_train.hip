// The training entries: sizing, forward, early preparation and backward of every trainable model kind, over the
// training graphs of train.hip.  What the entries share stands first.
#include <functional>

#include "run.h"

using namespace sty;

extern "C" {

// ready for a training forward or its sizing call: the model is finalized and of the right kind, training is enabled
// (not_enabled: the status when it is not) and the trainer exists
static int train_ready(sty_model* m, int not_enabled, const char* kind_a, const char* kind_b = nullptr) {
  int rc = model_ready(m, kind_a, kind_b);
  if (rc) return rc;
  if (!m->train_enabled) {
    set_error("training not enabled: call sty_model_enable_training / sty_model_bind_grad before finalize");
    return not_enabled;
  }
  if (!m->trainer) m->trainer = trainer_create(m);
  return STY_OK;
}
// ... and the entry's own argument check passed (bad_args: its outcome, msg: what sty_last_error then says), in that order
static int train_entry_ready(sty_model* m, int not_enabled, const char* kind_a, const char* kind_b, bool bad_args, const char* msg) {
  const int rc = train_ready(m, not_enabled, kind_a, kind_b);
  if (rc || !bad_args) return rc;
  set_error("%s", msg);
  return STY_EINVAL;
}
// the model is ready and a training forward has left its graph behind (have: what else the entry needs; msg: its own text where not)
static int recorded_ready(const sty_model* m, const char* kind_a, const char* kind_b, bool have, const char* msg) {
  const int rc = model_ready(m, kind_a, kind_b);
  if (rc || (m->trainer && have)) return rc;
  set_error("%s", msg);
  return STY_ESTATE;
}
// the end of a backward: the packed gradients of a segment (-1: all) go to the caller's buffers, then the gradient hook
static int finish_bwd(sty_model* m, hipStream_t st, int seg = -1) {
  int rc = weights_unpack(m, st, seg);
  if (rc) return rc;
  if (m->grad_hook) m->grad_hook(m->grad_hook_user, seg < 0 ? 0 : seg);
  return STY_OK;
}
// A *_bwd entry: a forward was recorded and the gradient is there (have_grad), then the graph's backward and finish_bwd
static int train_bwd(sty_model* m, const char* kind_a, const char* kind_b, bool have_grad, const char* msg, void* stream,
                     const std::function<int(Trainer*, hipStream_t)>& backward) {
  int rc = recorded_ready(m, kind_a, kind_b, have_grad, msg);
  if (rc || (rc = backward(m->trainer, S(stream)))) return rc;
  return finish_bwd(m, S(stream));
}

// Deterministic mode: the partial slots of its fixed-order sums are part of a training graph's workspace figure, and the
// backward takes them long after the forward has launched.  A *_fwd_train entry therefore sizes its graph for the mode first
// (the sizing pass: host code only) and refuses a smaller workspace here, before anything is launched.
static int det_ws_check(const char* what, size_t ws_bytes, const std::function<int(size_t*)>& size_of) {
  if (!deterministic_mode()) return STY_OK;
  size_t need = 0;
  const int rc = size_of(&need);
  if (rc) return rc;
  if (ws_bytes < need) {
    set_error("%s: workspace too small for the deterministic mode: need %zu bytes, have %zu", what, need, ws_bytes);
    return STY_ENOMEM;
  }
  return STY_OK;
}

// sty_*_prepare_train may run on another stream than the forward that consumes it: an event recorded behind the preparation
// orders the two (a no-op on the same stream).  The library cannot see a parameter update between the two calls (AdamW runs
// on flat buffers, not on a model): sty_model_invalidate is the caller's statement that the parameters changed.
static int prepared_mark(sty_model* m, void* stream) {
  if (!m->prepared_ev) STY_HIP(hipEventCreateWithFlags(&m->prepared_ev, hipEventDisableTiming));
  STY_HIP(hipEventRecord(m->prepared_ev, S(stream)));
  return STY_OK;
}
static int prepared_consume(sty_model* m, void* stream) {
  m->train_prepared = false;
  if (m->prepared_ev) STY_HIP(hipStreamWaitEvent(S(stream), m->prepared_ev, 0));
  return STY_OK;
}
// Weight-side half of a style encoder's training forward: the training-mode spectral-norm power iteration (u, v in the
// caller's buffers) and the prepared (normalised, packed) weights.  It depends on the parameters only, so a caller may
// issue it early (sty_style_prepare_train) beside the work that produces the encoder's input; the forward then skips it.
static int style_train_prepare(sty_model* m, void* stream) {
  if (m->train_prepared)  // done by sty_style_prepare_train since the last forward
    return prepared_consume(m, stream);
  int rc;
  if (m->topts.sn_power_iter && (rc = weights_sn_power_iter(m, S(stream)))) return rc;  // (u, v in the caller's buffers)
  // weights change between steps: re-derive the prepared form every step
  if ((rc = sty_model_prepare(m, stream))) return rc;
  m->prepared = false;
  return STY_OK;
}
// a sty_*_prepare_train entry: the weight-side half (prepare) ahead of the forward that consumes it
static int prepare_train(sty_model* m, const char* kind_a, const char* kind_b, int (*prepare)(sty_model*, void*), void* stream) {
  int rc = train_ready(m, STY_ESTATE, kind_a, kind_b);
  if (rc) return rc;
  m->train_prepared = false;
  if ((rc = prepare(m, stream)) || (rc = prepared_mark(m, stream))) return rc;
  m->train_prepared = true;
  return STY_OK;
}

// how a training forward gets its prepared weights
enum TrainPrepare {
  PREPARE_EACH_STEP,  // sty_model_prepare: parameters change every step
  PREPARE_SPEECH,     // ... unless sty_speech_prepare_train has done it since the last optimizer step
  PREPARE_STYLE,      // style_train_prepare
};
// What a *_fwd_train entry does between its argument check and its graph: the deterministic mode's workspace check (name:
// the entry's, size_of: its sizing entry on the same dimensions), then the weights.  A training step mutates buffers and is
// followed by an optimizer step, so `prepared` is cleared: inference re-prepares.
static int train_fwd_begin(sty_model* m, const char* name, size_t ws_bytes, const std::function<int(size_t*)>& size_of,
                           TrainPrepare how, void* stream) {
  int rc = det_ws_check(name, ws_bytes, size_of);
  if (rc) return rc;
  switch (how) {
    case PREPARE_STYLE:
      return style_train_prepare(m, stream);
    case PREPARE_SPEECH:
      if (m->train_prepared) {
        if ((rc = prepared_consume(m, stream))) return rc;
        break;
      }
      [[fallthrough]];
    case PREPARE_EACH_STEP:
      if ((rc = sty_model_prepare(m, stream))) return rc;
  }
  m->prepared = false;
  return STY_OK;
}

int sty_speech_train_workspace_bytes(sty_model* m, int B, int L, int T, size_t* bytes) {
  const int rc = train_entry_ready(m, STY_EINVAL, "speech_predictor", nullptr, !bytes || B <= 0 || L <= 0 || T <= 1,
                                   "sty_speech_train_workspace_bytes: bad argument");
  if (rc) return rc;
  const sty_speech_io io = speech_io_dims(B, L, T);
  return trainer_speech_forward(m->trainer, &io, nullptr, 0, nullptr, bytes);
}

int sty_speech_fwd_train(sty_model* m, const sty_speech_io* io, void* workspace, size_t ws_bytes, void* stream) {
  const bool bad = !io || !workspace || !io->texts || !io->text_lengths || !io->alignment || !io->pitch || !io->energy ||
                   !io->voiced || !io->style || !io->denormal_pitch || !io->audio || io->B <= 0 || io->L <= 0 || io->T <= 1;
  auto size_of = [&](size_t* n) { return sty_speech_train_workspace_bytes(m, io->B, io->L, io->T, n); };
  int rc = train_entry_ready(m, STY_ESTATE, "speech_predictor", nullptr, bad, "sty_speech_fwd_train: bad argument");
  if (rc || (rc = train_fwd_begin(m, "sty_speech_fwd_train", ws_bytes, size_of, PREPARE_SPEECH, stream))) return rc;
  return trainer_speech_forward(m->trainer, io, workspace, ws_bytes, S(stream), nullptr);
}
// The weight-side half of the next sty_speech_fwd_train (packs, input-gradient packs, bf16 fragments: ~20 launches that depend
// on the parameters only) ahead of time: AcousticTrainer issues it right after the predictor's AdamW step, while the style
// encoder's backward still runs on its streams, so the next step's forward starts with the text encoder.
int sty_speech_prepare_train(sty_model* m, void* stream) {
  return prepare_train(m, "speech_predictor", nullptr, sty_model_prepare, stream);
}

int sty_speech_bwd(sty_model* m, const float* d_audio, float* d_style, float* d_energy, void* stream) {
  return sty_speech_bwd_pe(m, d_audio, d_style, nullptr, d_energy, stream);
}
// ... also d loss / d pitch through the Decoder's F0 conv (train_textual feeds the PREDICTED pitch / energy to the frozen
// speech predictor, stage_type.py:139-160; the harmonic source and the voiced flag carry no gradient)
int sty_speech_bwd_pe(sty_model* m, const float* d_audio, float* d_style, float* d_pitch, float* d_energy, void* stream) {
  int rc = model_ready(m, "speech_predictor");
  if (rc) return rc;
  if (!m->trainer || !d_audio) {
    set_error("sty_speech_bwd: no forward recorded or null gradient");
    return STY_ESTATE;
  }
  // Gradient segment 0 (everything outside the text encoder) is un-packed and announced from inside the backward, as
  // soon as the decoder's backward and the style projections' backward have run; the text encoder's backward follows.
  bool seg0_done = false;
  int hook_rc = STY_OK;
  hipStream_t st = S(stream);
  // (Nobody to announce it to -- no gradient hook, i.e. no data-parallel exchange to overlap: the main stream then does
  // not stop for the weight-gradient stream in the middle of the backward, and both segments are un-packed at the end.)
  if (m->grad_hook)
    trainer_set_segment_hook(m->trainer, [&](int) {
      hook_rc = finish_bwd(m, st, 0);
      seg0_done = true;
    });
  rc = trainer_speech_backward(m->trainer, d_audio, d_style, d_energy, st, d_pitch);
  trainer_set_segment_hook(m->trainer, nullptr);
  if (rc) return rc;
  if (hook_rc) return hook_rc;
  if (!seg0_done && (rc = finish_bwd(m, st, 0))) return rc;
  return finish_bwd(m, st, 1);
}

int sty_speech_d_style_ready(sty_model* m, void* stream) {
  const int rc = recorded_ready(m, "speech_predictor", nullptr, true, "sty_speech_d_style_ready: no backward has run");
  if (rc) return rc;
  return trainer_wait_d_style(m->trainer, S(stream));
}
int sty_speech_branch_stream(sty_model* m, void** stream) {
  const int rc = recorded_ready(m, "speech_predictor", nullptr, stream, "sty_speech_branch_stream: no training forward has run, or stream == NULL");
  if (rc) return rc;
  *stream = trainer_branch_stream(m->trainer);
  return STY_OK;
}
int sty_vocoder_train_workspace_bytes(sty_model* m, int B, int T, size_t* bytes) {
  const int rc = train_entry_ready(m, STY_EINVAL, "speech_predictor", "vocoder", !bytes || B <= 0 || T <= 1,
                                   "sty_vocoder_train_workspace_bytes: bad argument");
  if (rc) return rc;
  const sty_vocoder_io io = vocoder_io_dims(B, T);
  return trainer_vocoder_forward(m->trainer, &io, nullptr, 0, nullptr, bytes);
}

int sty_vocoder_fwd_train(sty_model* m, const sty_vocoder_io* io, void* workspace, size_t ws_bytes, void* stream) {
  const bool bad = !io || !workspace || !io->mel || !io->style || !io->audio || io->B <= 0 || io->T <= 1 ||
                   (!io->prior_override && (!io->pitch || !io->voiced));
  auto size_of = [&](size_t* n) { return sty_vocoder_train_workspace_bytes(m, io->B, io->T, n); };
  int rc = train_entry_ready(m, STY_ESTATE, "speech_predictor", "vocoder", bad, "sty_vocoder_fwd_train: bad argument");
  if (rc || (rc = train_fwd_begin(m, "sty_vocoder_fwd_train", ws_bytes, size_of, PREPARE_EACH_STEP, stream))) return rc;
  return trainer_vocoder_forward(m->trainer, io, workspace, ws_bytes, S(stream), nullptr);
}

int sty_vocoder_bwd(sty_model* m, const float* d_audio, float* d_mel, float* d_style, void* stream) {
  return train_bwd(m, "speech_predictor", "vocoder", d_audio, "sty_vocoder_bwd: no forward recorded or null gradient", stream,
                   [&](Trainer* t, hipStream_t st) { return trainer_vocoder_backward(t, d_audio, d_mel, d_style, st); });
}

// ---- text aligner in the training graph (train_alignment, stage_type.py:268-341): forward, then sty_aligner_bwd ----
int sty_aligner_train_workspace_bytes(sty_model* m, int B, int T, size_t* bytes) {
  const int rc = train_entry_ready(m, STY_EINVAL, "text_aligner_train", nullptr, !bytes || B <= 0 || T <= 0,
                                   "sty_aligner_train_workspace_bytes: bad argument");
  if (rc) return rc;
  return trainer_aligner_forward(m->trainer, B, T, nullptr, nullptr, 0.1f, 0u, nullptr, nullptr, 0, nullptr, bytes);
}
int sty_aligner_fwd_train(sty_model* m, int B, int T, const float* mel, const int64_t* mel_lengths, float drop_p,
                          unsigned drop_seed, float* log_probs, void* workspace, size_t ws_bytes, void* stream) {
  const bool bad = !mel || !mel_lengths || !log_probs || !workspace || B <= 0 || T <= 0 || !(drop_p >= 0.f && drop_p < 1.f) ||
                   (size_t)B * T < 2;
  int rc = train_entry_ready(m, STY_ESTATE, "text_aligner_train", nullptr, bad,
                             "sty_aligner_fwd_train: bad argument (no null buffer, 0 <= drop_p < 1, at least two positions for the "
                             "batch statistics)");
  if (rc) return rc;
  if (m->topts.compute_bf16) {
    set_error("sty_aligner_fwd_train: compute_bf16 is refused for the text aligner");
    return STY_EINVAL;
  }
  auto size_of = [&](size_t* n) { return sty_aligner_train_workspace_bytes(m, B, T, n); };
  if ((rc = train_fwd_begin(m, "sty_aligner_fwd_train", ws_bytes, size_of, PREPARE_EACH_STEP, stream))) return rc;
  return trainer_aligner_forward(m->trainer, B, T, mel, mel_lengths, drop_p, drop_seed, log_probs, workspace, ws_bytes,
                                 S(stream), nullptr);
}
int sty_aligner_bwd(sty_model* m, const float* d_logits, void* stream) {
  return train_bwd(m, "text_aligner_train", nullptr, d_logits, "sty_aligner_bwd: no recorded forward or null gradient", stream,
                   [&](Trainer* t, hipStream_t st) { return trainer_aligner_backward(t, d_logits, st); });
}
// DurationPredictor in the training graph (train_duration, stage_type.py:495-556): forward, then sty_duration_bwd
int sty_duration_train_workspace_bytes(sty_model* m, int B, int L, size_t* bytes) {
  const int rc = train_entry_ready(m, STY_EINVAL, "duration_predictor", nullptr, !bytes || B <= 0 || L <= 0,
                                   "sty_duration_train_workspace_bytes: bad argument");
  if (rc) return rc;
  return trainer_duration_forward(m->trainer, B, L, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, bytes);
}
int sty_duration_fwd_train(sty_model* m, int B, int L, const int64_t* texts, const int64_t* text_lengths, const float* style,
                           float* out, void* workspace, size_t ws_bytes, void* stream) {
  auto size_of = [&](size_t* n) { return sty_duration_train_workspace_bytes(m, B, L, n); };
  int rc = train_entry_ready(m, STY_ESTATE, "duration_predictor", nullptr,
                             !texts || !text_lengths || !style || !out || !workspace || B <= 0 || L <= 0,
                             "sty_duration_fwd_train: bad argument");
  if (rc || (rc = train_fwd_begin(m, "sty_duration_fwd_train", ws_bytes, size_of, PREPARE_EACH_STEP, stream))) return rc;
  return trainer_duration_forward(m->trainer, B, L, texts, text_lengths, style, out, workspace, ws_bytes, S(stream), nullptr);
}
int sty_duration_bwd(sty_model* m, const float* d_out, float* d_style, void* stream) {
  return train_bwd(m, "duration_predictor", nullptr, d_out, "sty_duration_bwd: no recorded forward or null gradient", stream,
                   [&](Trainer* t, hipStream_t st) { return trainer_duration_backward(t, d_out, d_style, st); });
}
// PitchEnergyPredictor in the training graph (train_textual, stage_type.py:119-127): forward, then sty_pitch_energy_bwd
int sty_pitch_energy_train_workspace_bytes(sty_model* m, int B, int L, int T, size_t* bytes) {
  const int rc = train_entry_ready(m, STY_EINVAL, "pitch_energy_predictor", nullptr, !bytes || B <= 0 || L <= 0 || T <= 0,
                                   "sty_pitch_energy_train_workspace_bytes: bad argument");
  if (rc) return rc;
  return trainer_pitch_energy_forward(m->trainer, B, L, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                      nullptr, bytes);
}
int sty_pitch_energy_fwd_train(sty_model* m, int B, int L, int T, const int64_t* texts, const int64_t* text_lengths,
                               const float* alignment, const float* style, float* pitch, float* energy, void* workspace,
                               size_t ws_bytes, void* stream) {
  const bool bad = !texts || !text_lengths || !alignment || !style || !pitch || !energy || !workspace || B <= 0 || L <= 0 || T <= 0;
  auto size_of = [&](size_t* n) { return sty_pitch_energy_train_workspace_bytes(m, B, L, T, n); };
  int rc = train_entry_ready(m, STY_ESTATE, "pitch_energy_predictor", nullptr, bad, "sty_pitch_energy_fwd_train: bad argument");
  if (rc || (rc = train_fwd_begin(m, "sty_pitch_energy_fwd_train", ws_bytes, size_of, PREPARE_EACH_STEP, stream))) return rc;
  return trainer_pitch_energy_forward(m->trainer, B, L, T, texts, text_lengths, alignment, style, pitch, energy, workspace,
                                      ws_bytes, S(stream), nullptr);
}
int sty_pitch_energy_bwd(sty_model* m, const float* d_pitch, const float* d_energy, float* d_style, void* stream) {
  return train_bwd(m, "pitch_energy_predictor", nullptr, d_pitch && d_energy,
                   "sty_pitch_energy_bwd: no recorded forward or null gradient", stream,
                   [&](Trainer* t, hipStream_t st) { return trainer_pitch_energy_backward(t, d_pitch, d_energy, d_style, st); });
}

int sty_style_prepare_train(sty_model* m, void* stream) {
  return prepare_train(m, "mel_style_encoder", "pitch_style_encoder", style_train_prepare, stream);
}
int sty_style_train_workspace_bytes(sty_model* m, int B, int T, size_t* bytes) {
  const int rc = train_entry_ready(m, STY_EINVAL, "mel_style_encoder", nullptr, !bytes || B <= 0 || T < 40,
                                   "sty_style_train_workspace_bytes: bad argument");
  if (rc) return rc;
  return trainer_style_forward(m->trainer, B, T, nullptr, nullptr, nullptr, 0, nullptr, bytes);
}
int sty_style_fwd_train(sty_model* m, int B, int T, const float* mel, float* style, void* workspace, size_t ws_bytes,
                        void* stream) {
  auto size_of = [&](size_t* n) { return sty_style_train_workspace_bytes(m, B, T, n); };
  int rc = train_entry_ready(m, STY_ESTATE, "mel_style_encoder", nullptr, !mel || !style || !workspace || B <= 0 || T < 40,
                             "sty_style_fwd_train: bad argument (T >= 40 frames)");
  if (rc || (rc = train_fwd_begin(m, "sty_style_fwd_train", ws_bytes, size_of, PREPARE_STYLE, stream))) return rc;
  return trainer_style_forward(m->trainer, B, T, mel, style, workspace, ws_bytes, S(stream), nullptr);
}
// PitchStyleEncoder in the training graph (the second-stage `pe_style_encoder`): forward, then sty_style_bwd
int sty_pitch_style_train_workspace_bytes(sty_model* m, int B, int T, size_t* bytes) {
  const int rc = train_entry_ready(m, STY_EINVAL, "pitch_style_encoder", nullptr, !bytes || B <= 0 || T < 40,
                                   "sty_pitch_style_train_workspace_bytes: bad argument");
  if (rc) return rc;
  return trainer_style_forward(m->trainer, B, T, nullptr, nullptr, nullptr, 0, nullptr, bytes);
}
int sty_pitch_style_fwd_train(sty_model* m, int B, int T, const float* mel, const float* pitch, const float* energy,
                              float* style, void* workspace, size_t ws_bytes, void* stream) {
  auto size_of = [&](size_t* n) { return sty_pitch_style_train_workspace_bytes(m, B, T, n); };
  int rc = train_entry_ready(m, STY_ESTATE, "pitch_style_encoder", nullptr,
                             !mel || !pitch || !energy || !style || !workspace || B <= 0 || T < 40,
                             "sty_pitch_style_fwd_train: bad argument (T >= 40 frames)");
  if (rc || (rc = train_fwd_begin(m, "sty_pitch_style_fwd_train", ws_bytes, size_of, PREPARE_STYLE, stream))) return rc;
  return trainer_style_forward(m->trainer, B, T, mel, style, workspace, ws_bytes, S(stream), nullptr, pitch, energy);
}
int sty_style_bwd(sty_model* m, const float* d_style, void* stream) {
  return train_bwd(m, "mel_style_encoder", "pitch_style_encoder", d_style, "sty_style_bwd: no recorded forward or null gradient",
                   stream, [&](Trainer* t, hipStream_t st) { return trainer_style_backward(t, d_style, st); });
}
// parity taps of the style encoder's training graph: activation (grad = 0) or its gradient (grad = 1, after sty_style_bwd)
int sty_style_tap(sty_model* m, int index, int grad, float* dst, int* C, int* H, int* W, void* stream) {
  const int rc = recorded_ready(m, "mel_style_encoder", "pitch_style_encoder", true, "sty_style_tap: no recorded forward");
  if (rc) return rc;
  return trainer_style_tap(m->trainer, index, grad, dst, C, H, W, S(stream));
}

// ---- unit backward entry points: one sub-module in the training graph, forward + backward ----
int sty_block_train_workspace_bytes(sty_model* m, const char* kind, const char* prefix, int B, int C, int T,
                                    size_t* bytes) {
  int rc = train_entry_ready(m, STY_EINVAL, "speech_predictor", "vocoder", !kind || !prefix || !bytes || B <= 0 || C <= 0 || T <= 0,
                             "sty_block_train_workspace_bytes: bad argument");
  if (rc) return rc;
  int k = 0;
  const void* blk = nullptr;
  if ((rc = find_block(m, kind, prefix, C, &k, &blk))) return rc;
  return trainer_block_fwd_bwd(m->trainer, k, blk, B, C, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                               nullptr, bytes);
}

int sty_block_fwd_bwd(sty_model* m, const char* kind, const char* prefix, int B, int C, int T, const float* x,
                      const float* style, const float* gy, float* y, float* gx, float* d_style, void* workspace,
                      size_t ws_bytes, void* stream) {
  int rc = train_entry_ready(m, STY_ESTATE, "speech_predictor", "vocoder",
                             !kind || !prefix || !x || !style || !gy || !workspace || B <= 0 || C <= 0 || T <= 0,
                             "sty_block_fwd_bwd: bad argument");
  if (rc) return rc;
  int k = 0;
  const void* blk = nullptr;
  if ((rc = find_block(m, kind, prefix, C, &k, &blk))) return rc;
  auto size_of = [&](size_t* n) { return sty_block_train_workspace_bytes(m, kind, prefix, B, C, T, n); };
  if ((rc = train_fwd_begin(m, "sty_block_fwd_bwd", ws_bytes, size_of, PREPARE_EACH_STEP, stream))) return rc;
  rc = trainer_block_fwd_bwd(m->trainer, k, blk, B, C, T, x, style, gy, y, gx, d_style, workspace, ws_bytes, S(stream),
                             nullptr);
  if (rc) return rc;
  return weights_unpack(m, S(stream));
}

}  // extern "C"
