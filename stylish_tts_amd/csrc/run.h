// The inference side as the entry-point files share it: Run (one call's workspace, stream and status, with the block and
// plan methods), the readiness checks in front of an entry, and the per-model forward functions.  Bodies longer than a few
// lines live in one .hip each: plan_speech.hip has the speech predictor and the vocoder, plan_predictors.hip the style
// encoders, the second-stage predictors, the aligner and RMVPE, plan_wavlm.hip the WavLM graph, builder.hip the readiness checks.
#pragma once
#include <string.h>

#include "model.h"

namespace sty {

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---------------------------------------------------------------------------------------------------
// forward plans
// ---------------------------------------------------------------------------------------------------
struct Run {
  sty_model* m;
  Bump ws;
  hipStream_t st;
  int B;
  float* gb = nullptr;  // style fc outputs
  int rc = STY_OK;

  // workspace == nullptr: a sizing call (allocations are tracked, nothing is launched)
  Run(sty_model* model, int batch, void* workspace, size_t ws_bytes, void* stream) : m(model), st(S(stream)), B(batch) {
    ws.base = (char*)workspace;
    ws.cap = ws_bytes;
  }
  // the end of an entry point: the size a sizing call asked for, or an overflow of the caller's workspace
  int finish(size_t* need, const void* workspace, size_t ws_bytes) {
    if (need) *need = align_up(peak > ws.off ? peak : ws.off, 256) + 256;
    if (workspace && (ws.overflow || peak > ws_bytes)) {
      set_error("workspace too small: need %zu bytes, have %zu", peak, ws_bytes);
      return STY_ENOMEM;
    }
    return rc;
  }

  const float* gbp(const AdaFc& a) const { return gb ? gb + a.off * B : nullptr; }
  void chk(int r) {
    if (rc == STY_OK && r != STY_OK) rc = r;
  }
  bool live() const { return ws.base != nullptr && rc == STY_OK; }

  void conv(const ConvArgs& a0) {
    ConvArgs a = a0;
    a.bf16 = m->topts.compute_bf16 | m->wav_bf16;  // the compute mode also applies to the inference plans (wavlm: its own door)
    a.split = m->fp32_split && !a.bf16;             // sty_model_set_fp32_split: the inference plans alone read it
    if (live()) chk(launch_conv1d(a, st));
  }
  ConvArgs base(const PackedConv& w, const float* x, int T, float* y) {
    ConvArgs a;
    a.x[0] = x;
    a.xc[0] = w.Cin;
    a.nsrc = 1;
    a.B = B;
    a.T = T;
    a.w = w;
    a.pad = (w.K - 1) / 2;
    a.y = y;
    return a;
  }

  // AdaIN fold of tensor x [B][C][T] -> per-(b,c) affine (a, s)
  void adain(const float* x, int C, int T, const AdaFc& fc, float* a, float* s, double* part) {
    if (!live()) return;
    chk(launch_row_stats(x, B * C, T, part, st));
    chk(launch_adain_finalize(part, row_stats_nseg(T), gbp(fc), B, C, T, 1e-5f, a, s, st));
  }

  size_t peak = 0;
  void note_peak() { peak = ws.off > peak ? ws.off : peak; }
  struct Scope {  // temporaries taken inside a scope are released (bump pointer rewound) at its end
    Run& r;
    size_t off;
    explicit Scope(Run& run) : r(run), off(run.ws.off) {}
    ~Scope() {
      r.note_peak();
      r.ws.off = off;
    }
  };

  void layernorm_ada(const float* x, float* y, int C, int T, const AdaFc& fc) {
    if (live()) chk(launch_chan_layernorm(x, y, B, C, T, 1e-5f, 1, nullptr, nullptr, gbp(fc), 0, nullptr, st));
  }
  void tap(float* dst, const float* src, size_t n) {
    if (dst && src && rc == STY_OK) {
      hipError_t e = hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) rc = hip_fail(e, "tap copy");
    }
  }

  // ---- blocks and plans (plan_speech.hip) ----
  void convnext(const ConvNeXt& c, const float* x, float* y, int T);
  void resblock(const ResBlock32& r, float* x, int T);
  void conformer(const Conformer& c, const float* x, float* out, int C, int T);
  void vocoder(const sty_vocoder_io& io);
  void text_encoder(const int64_t* tokens, const int64_t* lengths, int L, float* mu);
  void dec_block(const DecBlock& d, const float* xcat, float* out, int T);
  void decoder(const float* asr, const float* pitch, const float* energy, const float* voiced, int T, float* out);
};

// ---- in front of an entry point (builder.hip) ----
// the model exists, is of the kind (either kind) and finalized
int model_ready(const sty_model* m, const char* kind_a, const char* kind_b = nullptr);
// ... and the entry's own argument check passed (bad_args: its outcome, msg: what sty_last_error then says), in that order
int entry_ready(const sty_model* m, const char* kind_a, const char* kind_b, bool bad_args, const char* msg);
// an inference forward prepares the weights unless a call since the last change of the parameters has
inline int ensure_prepared(sty_model* m, void* stream) { return m->prepared ? STY_OK : sty_model_prepare(m, stream); }
// a sizing call's io: the dimensions alone, every pointer null
inline sty_speech_io speech_io_dims(int B, int L, int T) {
  sty_speech_io io;
  memset(&io, 0, sizeof(io));
  io.B = B;
  io.L = L;
  io.T = T;
  return io;
}
inline sty_vocoder_io vocoder_io_dims(int B, int T) {
  sty_vocoder_io io;
  memset(&io, 0, sizeof(io));
  io.B = B;
  io.T = T;
  return io;
}

// ---- the forward functions ----
int run_style_fc(Run& r, const float* style);  // plan_speech.hip
// the vocoder block a state_dict prefix names, *k = 0: a ConvNeXt, 1: a ResBlock32 (no_resblock: the message, with one %s for the prefix)
int find_block(sty_model* m, const char* kind, const char* prefix, int C, int* k, const void** blk,
               const char* no_resblock = "no such resblock (32 channels): %s");
void style_run(Run& r, const float* mel, int T, float* style);  // plan_predictors.hip
void duration_forward(Run& r, const int64_t* texts, const int64_t* lengths, int L, float* out);
void pitch_energy_forward(Run& r, const int64_t* texts, const int64_t* lengths, const float* alignment, const float* style,
                          int L, int T, float* f0, float* energy);
void aligner_forward(Run& r, const float* mel, const int64_t* lengths, int T, float* out);
void rmvpe_forward(Run& r, int n, const float* logmel, float* sal);
void wavlm_forward(Run& r, int N16, const float* audio, float* hidden, WavlmKeep* kp = nullptr);  // plan_wavlm.hip
void wavlm_backward(Run& r, int N16, const WavlmKeep& kp, const float* d_hidden, float* d_audio, float* d_enc_in);

}  // namespace sty
