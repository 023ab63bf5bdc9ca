// Host-side model object: parameters bound by reference state_dict key, prepared-weight arena, forward plans.
#pragma once
#include <math.h>

#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "sty_common.h"
#include "weights.h"

namespace sty {

struct Param {
  const float* p = nullptr;
  std::vector<int64_t> shape;
};

int convnext32_ntiles(int T);
int launch_convnext32(const Cnx32Args& a, int B, int pass, hipStream_t st);
int launch_attention(const AttnArgs& a, int B, int DH, hipStream_t st);
int launch_rope_n(float* q, float* k, int B, int H, int DH, int L, int d, hipStream_t st, float sgn = 1.0f);
int launch_style_expand(const float* style, int B, int S, int L, float* y, hipStream_t st);
int launch_row_sum_add(const float* src, int rows, int L, float* dst, hipStream_t st);
int launch_wn_dw_bwd(const float* dw, const float* g, const float* v, int C, int K, float* dg, float* dv, hipStream_t st);
int launch_dur_post_bwd(const float* d, const float* mask, const float* go, int B, int NC, int L, float* gd, hipStream_t st);
int trainer_duration_forward(struct Trainer* t, int B, int L, const int64_t* texts, const int64_t* lengths, const float* style,
                             float* out, void* ws, size_t ws_bytes, hipStream_t st, size_t* need);
int trainer_duration_backward(struct Trainer* t, const float* d_out, float* d_style, hipStream_t st);
int trainer_aligner_forward(struct Trainer* t, int B, int T, const float* mel, const int64_t* lengths, float drop_p,
                            unsigned drop_seed, float* log_probs, void* ws, size_t ws_bytes, hipStream_t st, size_t* need);
int trainer_aligner_backward(struct Trainer* t, const float* d_logits, hipStream_t st);
int launch_scale_copy(const float* x, float a, size_t n, float* y, hipStream_t st);
int launch_mask_mul(float* x, const float* mask, int B, int C, int T, hipStream_t st);
int launch_wn_dw(const float* g, const float* v, int C, int K, float* w, hipStream_t st);
int launch_pad_time(const float* x, int rows, int T, int pad, float* y, hipStream_t st);
int launch_dur_post(const float* d, const float* mask, int B, int NC, int L, float* out, hipStream_t st);
int launch_rope(float* q, float* k, int B, int H, int DH, int L, int d, const float* theta4, hipStream_t st);
int launch_rope_copy(const float* qs, const float* ks, float* q, float* k, int B, int H, int DH, int L, int d,
                     const float* theta4, hipStream_t st);
int source_workspace_floats(int B, int T);
int launch_source(int B, int T, const float* pitch, const float* voiced, const float* noise, uint64_t seed,
                  const float* lin_w, const float* lin_b, float* prior, float* ws, hipStream_t st);
int launch_stft64(int B, int N, const float* wave, const float* br, const float* bi, float* spec, float* phase,
                  hipStream_t st);
int launch_istft64(int B, int F, const float* logamp, const float* real, const float* imag, const float* bbr,
                   const float* bbi, float* audio, hipStream_t st);
void build_stft64_bases(float* out);
size_t mel_workspace_floats(int B, int N, int n_fft, int hop, int n_mels);
int launch_mel(int B, int N, const float* audio, int n_fft, int win, int hop, int n_mels, int sample_rate, float mean,
               float std_, float* mel, float* energy, float* ws, hipStream_t st);
size_t multispec_workspace_floats(int B, int N, int n_fft, int hop);
size_t acoustic_loss_workspace_floats(int B, int N);
int launch_acoustic_loss(int B, int N, const float* audio_gt, const float* audio_pred, float w_mel, float w_phase,
                         float* losses_out, float* d_pred, float* ws, hipStream_t st);
// disc.hip: one spectrogram discriminator on target / pred images (element (b, h, w) at b*sb + h*sh + w; 0, 0 = dense),
// generator- and / or discriminator-side loss + backward (see sty_specdisc_losses); workspace == nullptr: dry run -> *need
int specdisc_run(const sty_specdisc_params* p, int B, int H, int W, size_t sb, size_t sh, const float* target,
                 const float* pred, float* scores_t, float* scores_p, float gen_scale, float* gen_loss, float* d_pred,
                 float disc_scale, float* disc_loss, const sty_specdisc_grads* grads, int compute_bf16, void* workspace,
                 size_t ws_bytes, hipStream_t st, size_t* need);
// adversarial term of the acoustic loss: the three spectrogram discriminators on the |STFT| of the three resolutions
struct AcousticGan {
  const sty_specdisc_params* p[3] = {nullptr, nullptr, nullptr};
  const sty_specdisc_grads* g[3] = {nullptr, nullptr, nullptr};  // entries may be null (that discriminator is not stepped)
  float w_gen = 1.f, disc_scale = 1.f;
  float* out = nullptr;  // device [7]: generator loss (sum), then (loss, loss without the relativistic term) per resolution
  int bf16 = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
};
size_t acoustic_gan_workspace_bytes(int B, int N, int with_grads);
int launch_acoustic_loss_gan(int B, int N, const float* audio_gt, const float* audio_pred, float w_mel, float w_phase,
                             float* losses_out, float* d_pred, float* ws, const AcousticGan* gan, hipStream_t st);
int launch_multispec_single(int B, int N, const float* audio, int n_fft, int hop, int sample_rate, float* mag,
                            float* phase, float* fft_mag, float* ws, hipStream_t st);
// the loss features of one signal at resolution r (0..2), forward only: mag [128][B][N / hop_r + 1] = log1p(mel128 |X|), the
// tensors the acoustic loss compares (frontend.hip; val_loss.hip reduces them)
size_t loss_features_scratch_floats(int B, int N);
int launch_loss_features(int B, int N, const float* audio, int r, float* mag, float* scratch, hipStream_t st);

// bump allocator over a caller-provided workspace (or a dry run that only measures)
struct Bump {
  char* base = nullptr;
  size_t off = 0, cap = 0;
  bool overflow = false;
  template <typename T>
  T* take(size_t n) {
    off = align_up(off, 256);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    if (base && off > cap) overflow = true;
    return p;
  }
};

// y16 (optional): the bf16 operand twin of the output for the conv that reads it next (ConvArgs::x16) -- bf16(lrelu(y))
// behind the learned down-sampling, bf16(y) behind the pooling
int launch_dwconv2d_s2(const float* x, const float* w9, const float* bias, int B, int C, int H, int W, float* y,
                       hipStream_t st, __bf16* y16_lrelu = nullptr);
int launch_avgpool2(const float* x, int BC, int H, int W, float scale, float* y, hipStream_t st, __bf16* y16 = nullptr);
int launch_pool_fc(const float* x, int B, int C, int n, int count, const float* W, const float* bvec, int S,
                   float* out, hipStream_t st);
struct AdaFc {      // one AdaIN / AdaLN style projection
  int idx = -1;     // index in the module's fc table
  int C = 0;        // channels (fc produces 2C)
  size_t off = 0;   // its [B][2C] output sits at gb_base + off*B
};

struct ConvNeXt {
  int C = 0;
  const float *dw_w = nullptr, *dw_b = nullptr, *b1 = nullptr, *alpha = nullptr, *grn_gamma = nullptr;
  AdaFc norm;
  PackedConv pw1, pw2;     // pw2.bias = b2eff (b2 + W2 . grn_beta)
  const float* w2a = nullptr;  // C == 32 only: chained-GEMM fragments
  const float* w1p = nullptr;
  const float *w1_raw = nullptr, *w2_raw = nullptr;  // pwconv1.weight [4C][C], pwconv2.weight [C][4C] as bound
};

struct ResBlock32 {
  PackedConv c1[3], c2[3];
  AdaFc n1[3], n2[3];
  const float *a1[3], *a2[3];
};

struct Conformer {
  AdaFc ff1n, ff2n, attn_n, conv_n, post_n;
  PackedConv ff1a, ff1b, ff2a, ff2b, to_q, to_kv, to_out, pw1, pw2;
  const float *dw_w, *dw_b, *bn_w, *bn_b, *bn_rm, *bn_rv;
};

struct VocoderPlan {
  PackedConv amp_input_conv;
  const float *amp_norm_w, *amp_norm_b;
  Conformer conf;
  std::vector<ConvNeXt> amp_convnext;   // 5 x C=256
  PackedConv upconv[3];
  ConvNeXt upblock[3];                  // C = 128, 64, 32
  const float *lin_w, *lin_b;           // m_source.l_linear
  const float *stft_fr, *stft_fi, *stft_br, *stft_bi;
  PackedConv amp_prior_conv, phase_prior_conv, phase_input_conv, amp_output_conv, real_conv, imag_conv;
  ResBlock32 amp_prior_block, phase_prior_block;
  const float *phase_norm_w, *phase_norm_b, *amp_fln_w, *amp_fln_b, *phase_fln_w, *phase_fln_b;
  std::vector<ConvNeXt> phase_convnext;  // 8 x C=32
  int hidden = 256;
};

struct TextEncLayer {
  PackedConv q, k, v, o, f1, f2;
  const float *n1g, *n1b, *n2g, *n2b;
};
struct TextEncPlan {
  const float* emb = nullptr;
  int tokens = 0, H = 0;
  PackedConv pre[3], proj, proj_m;
  const float *pre_g[3], *pre_b[3];
  std::vector<TextEncLayer> layers;
  float theta[4];
};

struct DecBlock {
  int Cin = 0, Cout = 0;
  PackedConv c1, c2, sc;
  bool has_sc = false;
  AdaFc n1, n2;
};
struct DecoderPlan {
  DecBlock encode, decode[4];
  PackedConv asr_res;
  float* fnv_w = nullptr;  // [3][4]: effective k3 weights + bias of F0_conv, N_conv, voiced_conv (prepared)
  const float *f0_g, *f0_v, *f0_b, *n_g, *n_v, *n_b, *v_g, *v_v, *v_b;
};

// ---- second-stage predictors, inference plans ----
struct ProsodyLayer {  // prosody_encoder.py:33-61
  PackedConv q, k, v, o, f1, f2, proj;
  AdaFc n1, n2;
};
struct DurationPlan {  // duration_predictor.py:16-58
  AdaFc qn, kn;
  PackedConv cq, ck, cv, co, post, proj;
  const float *dw_g = nullptr, *dw_v = nullptr, *dw_b = nullptr;  // weight-normed depthwise k5 of cross_post
  std::vector<ConvNeXt> cnx;
  int classes = 16;
};
struct PitchEnergyPlan {  // pitch_energy_predictor.py:8-60
  std::vector<ProsodyLayer> layers;
  DecBlock f0[4], nn[4];
  PackedConv f0p, np;
  int heads = 2;
};

// TextAligner = tdnn_blstm_ctc_model_base (text_aligner.py:33-45), eval mode: three TDNN convs (k = 5, 3, 3) each followed by
// ReLU and BatchNorm1d(affine=False) on running statistics, an Ffn of five Linear + ReLU with one skip, the output Linear
struct AlignerPlan {
  PackedConv tdnn[3], ffn[5], out;
  const float *rm[3] = {nullptr, nullptr, nullptr}, *rv[3] = {nullptr, nullptr, nullptr};
  float *bn_scale[3] = {nullptr, nullptr, nullptr}, *bn_shift[3] = {nullptr, nullptr, nullptr};  // prepared: 1 / sqrt(var + eps), -mean * scale
  float *bn_one = nullptr, *bn_zero = nullptr;  // kind text_aligner_train: the weight / bias of affine=False for the BatchNorm kernels
  int hidden = 640, n_mels = 80, classes = 179;
};
// align.hip
int launch_aligner_bn_prep(const float* mean, const float* var, int C, float eps, float* scale, float* shift, hipStream_t st);
int launch_aligner_bn(float* x, int B, int C, int T, const float* scale, const float* shift, hipStream_t st);
int launch_log_softmax_rows(const float* x, int B, int V, int T, float* out, hipStream_t st);
int launch_fill_f32(float* x, int n, float v, hipStream_t st);

// RMVPE = E2E0(n_blocks, 1, (2, 2), 5, inter_layers, 1, en_out_channels) in eval mode (train/dataprep/rmvpe/model.py:49-86,
// deepunet.py, seq.py); rmvpe.hip has the kernels, plan_predictors.hip the plan
constexpr int RMVPE_MELS = 128, RMVPE_CLASSES = 360, RMVPE_HOP = 200, RMVPE_LEVELS = 5;
constexpr float RMVPE_LOG_CLAMP = -11.5129254649702f;  // log(1e-5)
struct RmvpePackJob {  // one conv whose BatchNorm (if any) is folded while it is packed (rmvpe_pack_conv_kernel)
  const float *w = nullptr, *bias = nullptr, *bn_w = nullptr, *bn_b = nullptr, *bn_rm = nullptr, *bn_rv = nullptr;
  float *wp = nullptr, *bp = nullptr;
  int Cout = 0, Cin = 0, KH = 1, KW = 1, CinP = 0, CoutP = 0, co_off = 0, deconv = 0;
};
struct RmvpeBlock {  // ConvBlockRes (deepunet.py:6-41)
  int Cin = 0, Cout = 0;
  PackedConv c1, c2, sc;  // 3x3 + BN, 3x3 + BN (2-D mode: Cin = 3 * Cin2d), 1x1 with bias
  bool has_sc = false;
};
struct RmvpeUp {  // ConvTranspose2d + BN of a ResDecoderBlock (deepunet.py:72-84)
  int Cin = 0, Cout = 0;
  const float *wd = nullptr, *bias = nullptr;  // [Cin][Cout][9] scaled, [Cout]
};
struct RmvpePlan {
  int n_blocks = 0, inter_layers = 0, C0 = 0;
  const float* in_bn[4] = {nullptr, nullptr, nullptr, nullptr};  // encoder.bn weight, bias, running_mean, running_var
  float* in_ss = nullptr;                                        // prepared: scale, shift
  std::vector<RmvpeBlock> enc[RMVPE_LEVELS], inter, dec[RMVPE_LEVELS];
  RmvpeUp up[RMVPE_LEVELS];
  PackedConv cnn, gru_ih, head;  // Conv2d(C0 -> 3), [W_ih forward; W_ih reverse] 384 -> 1536, Linear(512 -> 360)
  const float *whh[2] = {nullptr, nullptr}, *bhh[2] = {nullptr, nullptr};
  float* whhT = nullptr;  // prepared: [2][256][768]
  std::vector<RmvpePackJob> packs;
};
inline int rmvpe_resampled_len(int N) { return (int)((2 * (long long)N + 2) / 3); }  // ceil(2 N / 3)
int rmvpe_mel_frames(int N);
size_t rmvpe_mel_workspace_floats(int B, int N);
void build_rmvpe_resample_kernel(float* out);
void build_rmvpe_mel_basis(float* out);
int launch_rmvpe_mel(int B, int N, const float* audio, float* logmel, float* ws, hipStream_t st);
// frontend.hip: |STFT| (periodic hann of n_fft, centre / reflect) of audio [B][Ns] -> mag [B][F][frames]; y: [B][2F][frames] scratch
int launch_stft_mag(int B, int Ns, const float* audio, int n_fft, int hop, int sample_rate, float* y, float* mag, hipStream_t st);
int rmvpe_prepare(const RmvpePlan& p, hipStream_t st);
int launch_rmvpe_input(const float* logmel, const float* ss, int B, int n, int Tp, float* x, hipStream_t st);
int launch_rmvpe_deconv(const float* x, const float* wd, const float* bias, int B, int Cin, int Cout, int Hi, int Wi, size_t ybs,
                        float* y, hipStream_t st);
int launch_rmvpe_gru_in(const float* x, int B, int T, float* y, hipStream_t st);
int launch_rmvpe_gru(const float* xg, const float* whhT, const float* bhh0, const float* bhh1, int B, int T, float* hout,
                     hipStream_t st);
int launch_rmvpe_salience(const float* logits, int B, int T, int n, float* sal, hipStream_t st);
int launch_rmvpe_decode(const float* sal, int rows, float thred, float* f0, hipStream_t st);

// FIR resampler of torchaudio's sinc_interp_hann form in rates reduced by their gcd (rmvpe.hip): `nw` phases of 2 width + orig
// taps at stride orig, y[b][nw q + p] = sum_j taps[p][j] x[b][orig q + j - width], zero outside [0, N)
inline int resample_width(int orig, int nw, double lpw) {
  const double base = (double)(orig < nw ? orig : nw) * 0.99;
  return (int)ceil(lpw * orig / base);
}
void build_resample_kernel(int orig, int nw, double lpw, float* out);
int launch_resample_fir(const float* x, const float* taps, int B, int N, int M, int orig, int nw, int width, float* y, hipStream_t st);

// WavLM = transformers' WavLMModel in eval mode (wavlm.hip has the kernels, plan_wavlm.hip the plan, weights.hip the packs)
constexpr int WAVLM_MAX_CONV = 8;
struct WavlmPackJob {  // wp[(kk / s) CinP + (kk % s) Cin + ci][co] = w[co0 + co][ci][kk] * (g ? g[kk] / nrm[kk] : 1); bp[co] = bias[co0 + co]
  const float *w = nullptr, *g = nullptr, *nrm = nullptr, *bias = nullptr;
  float *wp = nullptr, *bp = nullptr;
  int Cout = 0, Cin = 0, K = 1, s = 1, CinP = 0, CoutP = 0, co0 = 0;
};
struct WavlmLayer {
  PackedConv q, k, v, o, f1, f2;
  const float *gate_w = nullptr, *gate_b = nullptr, *gate_c = nullptr;  // gru_rel_pos_linear [8][DH], [8]; gru_rel_pos_const [H]
  const float *ln1_w = nullptr, *ln1_b = nullptr, *ln2_w = nullptr, *ln2_b = nullptr;
};
struct WavlmPlan {
  // sty_wavlm_set_config
  int n_conv = 0, stride[WAVLM_MAX_CONV] = {0}, max_distance = 800;
  float ln_eps = 1e-5f;
  // from the bound shapes
  int dim[WAVLM_MAX_CONV] = {0}, kern[WAVLM_MAX_CONV] = {0};
  int hidden = 0, heads = 0, pos_k = 0, pos_groups = 0, num_buckets = 0;
  const float *conv0_w = nullptr, *gn_w = nullptr, *gn_b = nullptr;
  PackedConv conv[WAVLM_MAX_CONV];  // i >= 1: the stride-s conv as a stride-1 conv of ceil(k / s) taps over s C phase-major channels
  const float *fp_ln_w = nullptr, *fp_ln_b = nullptr, *enc_ln_w = nullptr, *enc_ln_b = nullptr, *rel_embed = nullptr;
  PackedConv proj;
  const float* pos_v = nullptr;
  float* pos_nrm = nullptr;        // prepared: ||v[:, :, k]|| per tap
  std::vector<PackedConv> pos;     // one per group
  std::vector<WavlmLayer> layers;
  std::vector<WavlmPackJob> packs;
  // input-gradient weights of the convs packed by `packs` (made from their packed form behind them; the 1x1 convs go through
  // the model's dgrad table as every other kind's do)
  PackedConv conv_d[WAVLM_MAX_CONV];
  std::vector<PackedConv> pos_d;
};
// what sty_wavlm_fwd_keep leaves in the caller's workspace for sty_wavlm_bwd (all pointers into it)
struct WavlmKeepLayer {
  float *q = nullptr, *k = nullptr, *v = nullptr, *o = nullptr, *lse = nullptr, *gate = nullptr, *a1 = nullptr, *a2 = nullptr,
        *pre = nullptr;
};
struct WavlmKeep {
  bool valid = false;
  int B = 0, N16 = 0;
  int bf16 = 0;  // the operand mode of the forward that kept (sty_wavlm_set_compute); its backward must run in the same one
  const void* ws = nullptr;
  size_t saved_end = 0;  // workspace offset behind the kept tensors: the backward's scratch starts here
  float *out0 = nullptr, *ga = nullptr, *gs = nullptr, *gmean = nullptr, *grstd = nullptr;
  float* pre[WAVLM_MAX_CONV] = {nullptr};  // pre-activation of feature conv i >= 1
  int prs[WAVLM_MAX_CONV] = {0};           // ... and its row stride in floats (bf16 mode: a conv over the padded view leaves Tp columns)
  float *feat = nullptr, *pre_pos = nullptr, *xa_enc = nullptr, *tab = nullptr;
  std::vector<float*> x;  // layer inputs: x[l] enters layer l, x[layers] is the last output
  std::vector<WavlmKeepLayer> layers;
};
int wavlm_prepare(const WavlmPlan& p, hipStream_t st);  // weights.hip
int launch_wavlm_conv0(const float* x, const float* w, int B, int N, int C, int K, int S, int T, float* y, double* part, hipStream_t st);
int wavlm_conv0_ntiles(int T);
// mean_out / rstd_out (optional, [BC]): the row statistics themselves, kept for the backward
int launch_wavlm_gn_finalize(const double* part, int ntiles, const float* w, const float* b, int BC, int C, int T, float eps, float* a,
                             float* s, hipStream_t st, float* mean_out = nullptr, float* rstd_out = nullptr);
// x [B][C][Tin] -> y [B][S C][Tp], y[b][p C + c][t] = f(x[b][c][S t + p]) (0 past Tin); f = GELU(a[b][c] x + s[b][c]) with a set, else x
// gelu_in (without a): f = GELU(x), the input being a pre-activation (forward_keep)
int launch_wavlm_stage(const float* x, const float* a, const float* s, int B, int C, int Tin, int S, int Tp, float* y, hipStream_t st,
                       int gelu_in = 0);
// bf16 operand mode: x on rows of xrs >= Tin floats; y fp32 (y16 = 0) or the bf16 operand twin of the view (y16 = 1)
int launch_wavlm_stage_rs(const float* x, const float* a, const float* s, int B, int C, int Tin, int xrs, int S, int Tp, void* y,
                          int y16, hipStream_t st, int gelu_in = 0);
// [B][G Cg][T] <-> [G][B][Cg][T]
int launch_wavlm_group_perm(const float* x, int B, int G, int Cg, int T, int to_groups, float* y, hipStream_t st);
// bucket: the entry of distance -(T - 1) (the caller offsets a larger table)
int launch_wavlm_rel_table(const float* embed, const int32_t* bucket, int H, int T, float* tab, hipStream_t st);
int launch_wavlm_gate(const float* x, const float* w, const float* b, const float* c, int B, int H, int DH, int T, float* gate,
                      hipStream_t st);
int launch_wavlm_transpose_out(const float* x, int B, int C, int T, float* y, hipStream_t st);  // [B][C][T] -> [B][T][C]
void wavlm_rel_buckets(int T, int num_buckets, int max_distance, int32_t* out);
int slm_loss_groups(size_t n);
// d_b (optional): also d_b[i] = mag sign(b[i] - a[i]), 0 at a tie
int launch_slm_loss(size_t n, const float* a, const float* b, float* loss, double* part, hipStream_t st, float mag = 0.f,
                    float* d_b = nullptr);
// ---- WavLM backward to the wave (wavlm.hip; plan_wavlm.hip: wavlm_backward) ----
int launch_wavlm_gelu(const float* pre, const float* res, size_t n, float* y, hipStream_t st);  // y = res + GELU(pre), res optional
int launch_wavlm_intake(const float* dh, int B, int C, int T, int accumulate, float* dx, hipStream_t st);  // dx[b][c][t] (+)= dh[b][t][c]
int launch_wavlm_gate_bwd(const float* x, const float* w, const float* b, const float* c, const float* dgate, int B, int H, int DH,
                          int T, float* dx, hipStream_t st);  // dx += (accumulated into the head slices)
// dx [B][C][Tin] = (dview [B][S C][Tp] un-staged, zero past the view) * GELU'(pre [B][C][Tin])
int launch_wavlm_unstage(const float* dview, const float* pre, int B, int C, int Tin, int S, int Tp, float* dx, hipStream_t st);
// bf16 operand mode: pre on rows of prs floats; dx on rows of ors >= Tin elements (zero from Tin on), fp32 or bf16 (dx16 = 1)
int launch_wavlm_unstage_rs(const float* dview, const float* pre, int B, int C, int Tin, int prs, int S, int Tp, int ors, void* dx,
                            int dx16, hipStream_t st);
int launch_wavlm_pack(const WavlmPackJob& j, hipStream_t st);  // weights.hip: one job of wavlm_prepare (the unit entry's pack)
int wavlm_gn_bwd_ntiles(int T);
// GroupNorm(C, C) backward with layer 1's un-staging and GELU' fused; part: B C ntiles 2 doubles, coef: B C 2 floats
int launch_wavlm_gn_bwd(const float* x, const float* dview, const float* ga, const float* gs, const float* mean, const float* rstd, int B,
                        int C, int T, int S, int Tp, double* part, float* coef, float* dx, hipStream_t st);
int launch_wavlm_conv0_bwd(const float* dy, const float* w, int B, int N, int C, int K, int S, int T, float* dx, hipStream_t st);
// the adjoint of launch_resample_fir in gather form: dx[b][i] (+)= sum over the outputs that read sample i (rmvpe.hip)
int launch_resample_fir_bwd(const float* dy, const float* taps, int B, int N, int M, int orig, int nw, int width, int accumulate,
                            float* dx, hipStream_t st);

struct Trainer;
struct StyleResBlk {  // mel_style_encoder.py:69-118
  int Cin = 0, Cout = 0;
  bool down = false, has_sc = false;
  PackedConv c1, c2, sc;      // 3x3, 3x3, 1x1 (2-D mode: Cin = KH * Cin2d)
  const float* dw_w9 = nullptr;  // prepared depthwise stride-2 weights [Cin][9]
  const float* dw_b = nullptr;
};
struct StylePlan {
  int n_mels = 80, style_dim = 64;
  PackedConv stem;            // 3x3, 1 -> n_mels
  StyleResBlk blk[4];
  PackedConv head;            // 5x5 valid
  const float *fc_w = nullptr, *fc_b = nullptr;
};

}  // namespace sty

struct sty_model {
  std::string kind;
  std::unordered_map<std::string, sty::Param> params;
  std::vector<std::string> requested;
  bool finalized = false, prepared = false;
  bool train_prepared = false;  // sty_style_prepare_train ran and the next training forward has not consumed it yet
  hipEvent_t prepared_ev = nullptr;  // recorded behind that preparation on ITS stream: the consuming forward waits for it
  int style_dim = 64;
  // prepared-weight arena
  char* arena = nullptr;
  size_t arena_bytes = 0;
  sty::Bump ab;
  std::vector<sty::PackJob> jobs;
  std::vector<sty::StyleFcDesc> fcs;  // host copy; out = offset encoded as pointer, patched per call
  sty::StyleFcDesc* fcs_dev = nullptr;
  size_t gb_floats_per_batch = 0;
  std::string missing;
  sty::VocoderPlan voc;
  sty::TextEncPlan te;
  sty::DecoderPlan dec;
  sty::StylePlan sty_enc;
  sty::DurationPlan dur;
  sty::PitchEnergyPlan pe;
  sty::AlignerPlan ali;
  sty::RmvpePlan rmv;
  sty::WavlmPlan wav;
  sty::WavlmKeep wav_keep;
  // sty_model_set_fp32_split (kind speech_predictor): the inference entries run the 32-channel convs conv32p takes in its split
  // form; split_packed: the arena of the last finalize holds the fragment triples (PackedConv::w3) of those convs
  int fp32_split = 0;
  bool split_packed = false;
  int wav_bf16 = 0;  // sty_wavlm_set_compute: the dense contractions of the kind on the bf16 matrix cores (0 for every other kind)
  // device bucket table of the distances -(wav_bucket_T - 1) .. wav_bucket_T - 1: a bucket depends on the distance alone, so one
  // table sized for the largest frame count seen serves every smaller one at an offset
  int32_t* wav_bucket_dev = nullptr;
  int wav_bucket_T = 0;
  sty::PackedConv pse_pre;  // PitchStyleEncoder.preconv (mel_style_encoder.py:166)
  float* stft_default = nullptr;  // device [4][33][64]
  // ---- training ----
  bool train_enabled = false;
  char* garena = nullptr;  // gradients of the prepared (packed) weights, same layout/offsets as `arena`
  std::unordered_map<const float*, float*> pgrad;               // bound parameter -> caller's gradient buffer
  std::unordered_map<std::string, float*> pgrad_by_key;
  std::unordered_map<const float*, sty::PackedConv> dgrad;      // forward packed weights -> input-gradient weights
  std::unordered_map<const float*, sty::PackedConv> plain_of;   // GLU-ordered packed conv -> plain-ordered copy
  void* fcs_bwd_dev = nullptr;
  sty::WeightTables wt;  // device tables of the batched weight-side launches (weights.h)
  // gradient segments (data-parallel overlap): pack jobs [0, seg_job_split) belong to the module that runs its backward
  // LAST (the text encoder of a speech predictor).  Segment 0 = every other parameter: complete, un-packed and announced
  // through grad_hook while the last module's backward still runs.
  size_t seg_job_split = 0;
  sty_grad_hook grad_hook = nullptr;
  void* grad_hook_user = nullptr;
  sty_train_opts topts = {0, 0, 0, 0, 0.1f, 0u, 0.2f, 0, 0};  // train-mode behaviour of the *_fwd_train entry points
  struct sty::Trainer* trainer = nullptr;
};

// ---- backward launchers (bwd.hip, wgrad.hip) and training-mode state ----
#include <functional>
#include <unordered_set>
namespace sty {
// The route launch_conv1d takes for `a` in the model's compute mode.  The plans (Run, Trainer) ask ahead of the launch: who
// leaves AdaIN statistics behind, whether a resblock stores two-byte tensors (ask with xh / yh / rh set), whether the head
// LayerNorm is a pass in front of the persistent kernel or a prologue of the tiled one.
inline ConvRoute plan_route(const sty_model* m, ConvArgs a) {
  a.bf16 = m->topts.compute_bf16;
  return conv1d_route(a);
}
int launch_pro_bwd(int mode, const float* u, int Cu, int cu0, const float* x, int B, int C, int T, const float* pa,
                   const float* ps, int pC, int pc0, const float* alpha, const float* mask, float* dx, int accumulate,
                   float* dpa, float* dps, float* dalpha, hipStream_t st, bool det = false);
int launch_adain_fold_bwd(const float* da, const float* ds, const float* mean, const float* rstd, const float* gb, int B,
                          int C, int T, float* dgb, float* c0, float* c1, hipStream_t st);
int launch_row_axpb(const float* x, const float* c0, const float* c1, int rows, int T, float* dx, hipStream_t st);
// AdaIN + Snake prologue backward with the instance-norm statistics term in ONE launch (bwd.hip); u / x / dx fp32 or bf16 tensors
int launch_pro_bwd_adain(const void* u, int uh, const void* x, int xh, int B, int C, int T, const float* pa, const float* ps,
                         const float* alpha, const float* mean, const float* rstd, const float* gb, void* dx, int dh,
                         int accumulate, float* dgb, float* dalpha, int hw, hipStream_t st, const void* dsrc = nullptr,
                         bool det = false);
// plain casts between an fp32 tensor and a two-byte one (test aids of the block entry point)
int launch_cast_f32_to_16(const float* x, size_t n, void* y16, hipStream_t st);
int launch_cast_16_to_f32(const void* x16, size_t n, float* y, hipStream_t st);
bool chan_ln32_eligible(int B, int C, int T, int relu);  // the one-thread-per-column form (the only one with two-byte tensors)
// h16 bits: 1 = x, 2 = dy, 4 = dx are bf16 tensors
int launch_chan_ln_bwd(const float* x, const float* dy, const float* y, int B, int C, int T, float eps, int ada,
                       const float* w, const float* gb, int relu, const float* out_mask, float* dx, int accumulate,
                       float* mu_tmp, float* r_tmp, float* dgb, float* dw, float* db, hipStream_t st, int h16 = 0,
                       bool det = false);
// gx [B][C4]: the forward's per-channel norms (launch_grn_finalize).  gx == nullptr (the unit entry's comparison only): they
// are rebuilt from the forward's partials (part, nseg)
int launch_grn_bwd(const float* gx, const double* part, int nseg, const float* gamma, const float* ds, int B, int C4,
                   float* coef, float* dgamma, hipStream_t st, bool det = false);
int launch_act_fwd(int kind, const float* x, const float* alpha, int B, int C, int T, float* y, hipStream_t st);
// h, coef [B][C] (optional): the output gradient is dy + coef[b][c] * h, formed in the kernel (the GRN term)
int launch_act_bwd(int kind, const float* x, const float* dy, const float* alpha, int B, int C, int T, float* dx,
                   int accumulate, float* dalpha, hipStream_t st, const float* h = nullptr, const float* coef = nullptr,
                   bool det = false);
int launch_row_scale_add(const float* src, const float* coef, float k, int rows, int T, float* dst, hipStream_t st);
int launch_dwconv_fwd(const float* x, const float* w, const float* bias, int B, int C, int T, int K, int pad, float* y,
                      hipStream_t st);
size_t dwconv_bwd_scratch_floats(int B, int C, int T, int K);
int launch_dwconv_bwd(const float* x, const float* dy, const float* w, int B, int C, int T, int K, int pad, float* dx,
                      int accumulate, float* dw, float* db, float* scratch, hipStream_t st, const float* dx_src = nullptr,
                      int x16 = 0, int dy16 = 0);  // x16 / dy16: bf16 tensors (weight-gradient part only: dx == nullptr)
int launch_bn_eval_fwd(const float* x, const float* w, const float* b, const float* rm, const float* rv, float eps,
                       int B, int C, int T, float* y, hipStream_t st);
int launch_bn_eval_bwd(const float* x, const float* dy, const float* w, const float* rm, const float* rv, float eps,
                       int B, int C, int T, float* dx, float* dw, float* db, hipStream_t st);
size_t bias_grad_scratch_floats(int B, int C, int T);
int launch_partial_sum(int dw_form, const float* part, int C, int K, int nblk, float* dw, float* db, hipStream_t st);
int launch_bias_grad(const float* g, const float* mask, int B, int C, int T, int shuffle, float scale, float* db,
                     float* scratch, hipStream_t st);
int launch_style_fc_bwd(const void* descs_dev, int nlayers, int B, int style_dim, const float* style,
                        const float* dgb_base, float* dstyle, hipStream_t st, bool det = false);
int style_fc_bwd_slots(int nlayers);  // det: dstyle is a [slots][B][style_dim] partial buffer
int launch_istft64_bwd(int B, int F, const float* audio, const float* daudio, const float* logamp, const float* real,
                       const float* imag, const float* bbr, const float* bbi, float* dlogamp, float* dreal,
                       float* dimag, hipStream_t st);
size_t wgrad_partial_floats(const PackedConv& w, int B, int T);
// wgrad.hip, "deferred, grouped reduction": while a WgReduceDefer is current on the calling thread, the reduction that
// follows every weight-gradient kernel is recorded instead of launched (each launch then needs a partial buffer of its
// own that lives until the flush); wgrad_defer_flush sums all recorded jobs in one launch on `st`.
struct WgReduceDefer;
WgReduceDefer* wgrad_defer_create();
void wgrad_defer_destroy(WgReduceDefer* d);
WgReduceDefer* wgrad_defer_set(WgReduceDefer* d);  // returns the previous one (nullptr = immediate reductions)
size_t wgrad_defer_pending(const WgReduceDefer* d);
int wgrad_defer_flush(WgReduceDefer* d, int site, hipStream_t st);
// gwp[i] (+ gbias behind `plane`) += sum over k < nslices of partial[k * stride + i], the slices in a fixed order; recorded
// while a WgReduceDefer is current, launched on `st` otherwise
void launch_wgrad_reduce_planes(const float* partial, int nslices, size_t plane, size_t stride, int nb, float* gwp,
                                float* gbias, hipStream_t st);
int launch_attention_bwd(const AttnArgs& a, const float* dO, float* dQ, float* dK, float* dV, size_t dqbs, size_t dkbs,
                         size_t dvbs, size_t dobs, int B, int DH, float* ws, hipStream_t st, int overwrite = 0);
bool attention_bwd_can_overwrite(const AttnArgs& a, int DH);
bool attention_bwd_mfma_dh(int DH);
size_t attention_bwd_ws_floats(int B, int H, int T);
int launch_rope_signed(float* q, float* k, int B, int H, int DH, int L, int d, const float* theta4, float sgn,
                       hipStream_t st);
int launch_embedding_bwd(const int64_t* tokens, const float* g, int B, int L, int H, int ntok, float scale, float* demb,
                         hipStream_t st, bool det = false);
int launch_bmm_ct_bwd(const float* g, const float* ali, int B, int C, int L, int T, float* denc, hipStream_t st);
int launch_slice_add(const float* src, int Csrc, int c0, int B, int C, int T, float* dst, hipStream_t st);
int launch_fnv_bwd(const float* pitch, const float* energy, const float* voiced, const float* w34, const float* g, int B,
                   int T, float* dw34, float* dp, float* de, float* dv, hipStream_t st, bool det = false);
int fnv_bwd_slices();  // det: dw34 is a [slices][12] partial buffer
int launch_fnv_unpack(const float* dw34, const float* g0, const float* v0, const float* g1, const float* v1,
                      const float* g2, const float* v2, float* dg0, float* dv0, float* db0, float* dg1, float* dv1,
                      float* db1, float* dg2, float* dv2, float* db2, hipStream_t st);
size_t dwconv2d_s2_bwd_scratch_floats(int B, int C, int H, int W);
// dx16 / mask16 (optional; overwriting form only): also write bf16(dx * mask16[b][n]), the operand twin of dx
// dx == nullptr (with dx16): the twin alone -- the caller knows that every reader of dx takes the twin
int launch_dwconv2d_s2_bwd(const float* x, const float* gy, const float* gate, const float* w9, int B, int C, int H, int W, float* dx,
                           int accumulate, float* dw9, float* db, float* scratch, hipStream_t st, __bf16* dx16 = nullptr,
                           const float* mask16 = nullptr);
int launch_pad_cols(const float* x, size_t rows, int W, float* y, hipStream_t st);
int launch_flat_mask(int B, int H, int Wp, int Hv, int Wv, float* m, hipStream_t st);
int launch_dw2d_sn_unpack(const float* g9, const float* w, const float* u, const float* v, const float* t, int C,
                          float* dW, hipStream_t st);
int launch_avgpool2_bwd(const float* gy, int BC, int H, int W, float scale, float* dx, const float* gate, hipStream_t st,
                        __bf16* dx16 = nullptr, const float* mask16 = nullptr, int C = 0);
int launch_pool_fc_bwd(const float* x, int B, int C, int n, int count, const float* W, int S, const float* gs,
                       float* dW, float* db, float* dx, int accumulate, hipStream_t st, float* det_a = nullptr);
int launch_bn_train_fwd(const float* x, const float* w, const float* b, float* rm, float* rv, float eps, float momentum,
                        int B, int C, int T, float* y, float* mean, float* rstd, double* part, hipStream_t st);
int launch_bn_train_bwd(const float* x, const float* dy, const float* w, const float* mean, const float* rstd, int B,
                        int C, int T, float* dx, int accumulate, float* dw, float* db, float* sums, hipStream_t st);
int launch_dropout(const float* x, const float* res, size_t n, float p, unsigned seed, unsigned site, float* y,
                   int accumulate, hipStream_t st, size_t group = 1);
int launch_box_smooth(const float* x, int B, int T, int width, float* y, int accumulate, hipStream_t st);
size_t sn_power_iter_scratch_floats(int Cout, int n);
int trainer_style_forward(struct Trainer* t, int B, int T, const float* mel, float* style, void* ws, size_t ws_bytes,
                          hipStream_t st, size_t* need, const float* pitch = nullptr, const float* energy = nullptr);
int trainer_style_backward(struct Trainer* t, const float* d_style, hipStream_t st);
int trainer_style_tap(struct Trainer* t, int i, int grad, float* dst, int* C, int* H, int* W, hipStream_t st);
// the vocoder's half of a speech predictor call (taps included); the caller adds mel, the decoder's output
inline sty_vocoder_io vocoder_io_of(const sty_speech_io& io) {
  sty_vocoder_io v = io.voc_taps;
  v.B = io.B;
  v.T = io.T;
  v.style = io.style;
  v.pitch = io.denormal_pitch;
  v.voiced = io.voiced;
  v.noise = io.noise;
  v.prior_override = io.prior_override;
  v.seed = io.seed;
  v.audio = io.audio;
  return v;
}
struct Trainer;
Trainer* trainer_create(sty_model* m);
int trainer_speech_forward(Trainer* t, const sty_speech_io* io, void* ws, size_t ws_bytes, hipStream_t st,
                           size_t* need);
int trainer_speech_backward(Trainer* t, const float* d_audio, float* d_style, float* d_energy, hipStream_t st,
                            float* d_pitch = nullptr);
int trainer_block_fwd_bwd(Trainer* t, int kind, const void* blk, int B, int C, int T, const float* x, const float* style,
                          const float* gy, float* y, float* gx, float* d_style, void* ws, size_t ws_bytes, hipStream_t st,
                          size_t* need);
void trainer_set_segment_hook(Trainer* t, std::function<void(int)> fn);  // called once segment 0's gradients are final
bool single_stream_mode();  // sty_set_single_stream: no internal side streams (measurement aid)
// sty_set_deterministic: sums whose result depends on the arrival order of atomics take a fixed-order path.  A launcher's
// `det` argument (default false: the atomic form) says that the gradient pointer it is given in the parameter's place is a
// partial buffer with one slot per writer -- [B][C] for the per-(b, c) rows -- which the caller sums in index order.  Every
// entry that runs a forward latches the mode; its backward follows the forward's.
bool deterministic_mode();
// out[i] += sum over k < nslots of part[k * stride + i], i < n: the slots in a fixed order, in double
int launch_det_sum64(const double* part, int nslots, size_t n, size_t stride, double* out, hipStream_t st);
int trainer_wait_d_style(Trainer* t, hipStream_t stream);
void* trainer_branch_stream(Trainer* t);  // where the prior branch of the last speech forward ran and its backward will (nullptr: in place)
int trainer_pitch_energy_forward(Trainer* t, int B, int L, int T, const int64_t* texts, const int64_t* lengths,
                                 const float* alignment, const float* style, float* pitch, float* energy, void* ws,
                                 size_t ws_bytes, hipStream_t st, size_t* need);
int trainer_pitch_energy_backward(Trainer* t, const float* d_pitch, const float* d_energy, float* d_style, hipStream_t st);
void trainer_destroy(Trainer* t);
int trainer_vocoder_forward(Trainer* t, const sty_vocoder_io* io, void* ws, size_t ws_bytes, hipStream_t st,
                            size_t* need);
int trainer_vocoder_backward(Trainer* t, const float* d_audio, float* d_mel, float* d_style, hipStream_t st);
}  // namespace sty
