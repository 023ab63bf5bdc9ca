// RMVPE pitch extraction (train/dataprep/rmvpe/: model.py:49-86 E2E0, deepunet.py, seq.py, inference.py:29-62,
// utils.py:114-131, spec.py): everything of the pitch command that is not a dense conv on launch_conv1d.
//
// (1) Front end.  torchaudio Resample(24000, 16000, lowpass_filter_width=128), sinc_interp_hann, rolloff 0.99: the ratio
//     reduces to 3 -> 2, so the output is two interleaved phases of a 391-tap FIR at stride 3 (resample_fir_kernel, taps in
//     LDS; the slm loss shares it with 23 taps); the 1024-point |STFT| runs on the LDS FFT of frontend.hip, the 128 x 513 mel basis (librosa mel(htk=True), Slaney
//     normalised) is a K = 1 conv, rmvpe_logmel_kernel takes log(clamp(., 1e-5)).  Both tables are closed forms evaluated in
//     double on the host and rounded to fp32 once (build_resample_kernel, build_rmvpe_mel_basis).  torchaudio and librosa
//     are absent: PARITY UNPINNED at this boundary, as the other front end is.
// (2) Weight side.  Every BatchNorm behind a bias-free conv is folded into the packed weights and the bias
//     (rmvpe_pack_conv_kernel: Conv2d [Cout][Cin][KH][KW] -> the flat 2-D order wp[kw][kh Cin + ci][co], also the GRU's two
//     W_ih as one GEMM of 1536 rows; rmvpe_pack_deconv_kernel: ConvTranspose2d [Cin][Cout][3][3] keeps its order, scaled).
//     encoder.bn sits in front of a zero-padded conv and cannot be folded: its scale and shift are applied by
//     rmvpe_input_kernel, which also transposes [128][n] -> [T][128 + 1] and reflects the frame axis to a multiple of 32.
// (3) rmvpe_deconv_kernel: ConvTranspose2d(3 x 3, stride 2, pad 1, output_padding 1) + BN + ReLU over the four output
//     parities.  oh = 2 ih - 1 + kh: output (2 ih, 2 iw) is reached by the centre tap alone, (2 ih, 2 iw + 1) and
//     (2 ih + 1, 2 iw) by two taps, (2 ih + 1, 2 iw + 1) by the four corners -- nine products per input position, channel
//     pair and output quad, where a zero-inserted dense conv spends 36.  A thread owns one input position and DC_CO output
//     channels (weights are wave-uniform: scalar loads) over a quarter of the input channels; the four quarters meet in LDS
//     and the quad goes into the first half of the concat buffer.
// (4) rmvpe_gru_kernel: one workgroup per (direction, group of up to four utterances).  W_ih x + b_ih of every frame is one
//     GEMM in front; per step the workgroup streams W_hh^T [256][768] (768 KB, L2-resident) once for the whole group:
//     thread (j, kq) sums k in [64 kq, 64 kq + 64) for the three gates of unit j, the four partial sums meet in LDS and
//     thread (j, g) applies PyTorch's gates (r, z, n; n = tanh(i_n + r (W_hn h + b_hn)); h' = (1 - z) n + z h) for utterance g.
// (5) rmvpe_decode_kernel (to_local_average_f0): one wave per frame.
#include <math.h>

#include <vector>

#include "model.h"

namespace sty {

// ---------------------------------------------------------------------------------------------------------------------
// host tables
// ---------------------------------------------------------------------------------------------------------------------
constexpr int RS_WIDTH = 194;             // ceil(128 * 3 / 1.98)
constexpr int RS_TAPS = 2 * RS_WIDTH + 3;  // 391
// out [nw][2 width + orig]: phase p, tap j' = j - width (torchaudio _get_sinc_resample_kernel, sinc_interp_hann, rolloff 0.99)
void build_resample_kernel(int orig, int nw, double lpw, float* out) {
  const double base = (double)(orig < nw ? orig : nw) * 0.99, pi = 3.14159265358979323846;
  const int width = resample_width(orig, nw, lpw), taps = 2 * width + orig;
  for (int p = 0; p < nw; ++p)
    for (int j = 0; j < taps; ++j) {
      double t = (-(double)p / (double)nw + (double)(j - width) / (double)orig) * base;
      t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
      const double c = cos(t * pi / lpw / 2.0);
      const double window = c * c;
      t *= pi;
      const double sinc = t == 0.0 ? 1.0 : sin(t) / t;
      out[p * taps + j] = (float)(sinc * window * (base / (double)orig));
    }
}
// out [2][391]: the pitch front end's table, lowpass_filter_width = 128
void build_rmvpe_resample_kernel(float* out) { build_resample_kernel(3, 2, 128.0, out); }
// out [128][513]: librosa.filters.mel(sr=16000, n_fft=1024, n_mels=128, fmin=30, fmax=8000, htk=True), norm="slaney"
void build_rmvpe_mel_basis(float* out) {
  const int n_mels = RMVPE_MELS, F = 513;
  auto hz2mel = [](double f) { return 2595.0 * log10(1.0 + f / 700.0); };
  auto mel2hz = [](double m) { return 700.0 * (pow(10.0, m / 2595.0) - 1.0); };
  const double lo = hz2mel(30.0), hi = hz2mel(8000.0);
  double f[RMVPE_MELS + 2];
  for (int i = 0; i < n_mels + 2; ++i) f[i] = mel2hz(lo + (hi - lo) * (double)i / (double)(n_mels + 1));
  for (int i = 0; i < n_mels; ++i) {
    const double enorm = 2.0 / (f[i + 2] - f[i]);
    for (int k = 0; k < F; ++k) {
      const double fr = 8000.0 * (double)k / (double)(F - 1);
      const double lower = (fr - f[i]) / (f[i + 1] - f[i]), upper = (f[i + 2] - fr) / (f[i + 2] - f[i + 1]);
      const double w = fmax(0.0, fmin(lower, upper));
      out[i * F + k] = (float)(w * enorm);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// front end
// ---------------------------------------------------------------------------------------------------------------------
// y[b][nw q + p] = sum_j k[p][j] x[b][orig q + j - width], zero outside [0, N); M = ceil(nw N / orig) outputs per row; the
// nw (2 width + orig) taps in LDS (the pitch front end: 2 x 391; the slm loss: 2 x 23)
__global__ __launch_bounds__(256) void resample_fir_kernel(const float* __restrict__ x, const float* __restrict__ taps, int N,
                                                           int M, int orig, int nw, int width, float* __restrict__ y) {
  extern __shared__ float k[];
  const int nt = 2 * width + orig;
  for (int i = threadIdx.x; i < nw * nt; i += 256) k[i] = taps[i];
  __syncthreads();
  const int m = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (m >= M) return;
  const int q = m / nw, p = m - q * nw;
  const float* xb = x + (size_t)b * N;
  const int i0 = orig * q - width;
  const int j0 = i0 < 0 ? -i0 : 0, j1 = i0 + nt > N ? N - i0 : nt;
  float acc = 0.f;
  for (int j = j0; j < j1; ++j) acc = fmaf(k[p * nt + j], xb[i0 + j], acc);
  y[(size_t)b * M + m] = acc;
}
int launch_resample_fir(const float* x, const float* taps, int B, int N, int M, int orig, int nw, int width, float* y, hipStream_t st) {
  const int nt = 2 * width + orig;
  ProfScope prof("resample_fir_kernel", 2.0 * nt * B * M, 4.0 * B * ((double)N + M), st);
  hipLaunchKernelGGL(resample_fir_kernel, dim3(cdiv(M, 256), B), dim3(256), (size_t)nw * nt * sizeof(float), st, x, taps, N, M, orig, nw,
                     width, y);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
// The adjoint in gather form: sample i of row b is read by output m = nw q + p at tap j = i + width - orig q, so
// dx[b][i] (+)= sum_q sum_p k[p][i + width - orig q] dy[b][nw q + p], q ascending and p inside it: a fixed order, no atomic.
__global__ __launch_bounds__(256) void resample_fir_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ taps, int N,
                                                               int M, int orig, int nw, int width, int accumulate,
                                                               float* __restrict__ dx) {
  extern __shared__ float k[];
  const int nt = 2 * width + orig;
  for (int i = threadIdx.x; i < nw * nt; i += 256) k[i] = taps[i];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= N) return;
  const float* gb = dy + (size_t)b * M;
  const int top = i + width;             // j = top - orig q in [0, nt)
  int q0 = (top - nt + orig) / orig;     // ceil((top - nt + 1) / orig) for a non-negative numerator
  if (top - nt + 1 <= 0) q0 = 0;
  const int q1 = top / orig;
  float acc = 0.f;
  for (int q = q0; q <= q1; ++q) {
    const int j = top - orig * q;
    for (int p = 0; p < nw; ++p) {
      const int m = nw * q + p;
      if (m < M) acc = fmaf(k[p * nt + j], gb[m], acc);
    }
  }
  const size_t o = (size_t)b * N + i;
  dx[o] = accumulate ? dx[o] + acc : acc;
}
int launch_resample_fir_bwd(const float* dy, const float* taps, int B, int N, int M, int orig, int nw, int width, int accumulate,
                            float* dx, hipStream_t st) {
  const int nt = 2 * width + orig;
  ProfScope prof("resample_fir_bwd_kernel", 2.0 * nt * B * M, 4.0 * B * ((double)N + M), st);
  hipLaunchKernelGGL(resample_fir_bwd_kernel, dim3(cdiv(N, 256), B), dim3(256), (size_t)nw * nt * sizeof(float), st, dy, taps, N, M, orig,
                     nw, width, accumulate, dx);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
// in place: log(clamp(x, 1e-5)); the clamped value is the constant, so that silence is one bit pattern
__global__ __launch_bounds__(256) void rmvpe_logmel_kernel(float* __restrict__ x, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  x[i] = v > 1e-5f ? logf(v) : RMVPE_LOG_CLAMP;
}

static PackedConv g_mel_basis;        // [513] -> [128], built on first use
static float* g_resample_taps = nullptr;
static int front_tables(hipStream_t st) {
  if (g_resample_taps) return STY_OK;
  std::vector<float> taps(2 * RS_TAPS), fb((size_t)RMVPE_MELS * 513);
  build_rmvpe_resample_kernel(taps.data());
  build_rmvpe_mel_basis(fb.data());
  PackedConv pc;
  pc.Cin = 513, pc.Cout = RMVPE_MELS, pc.K = 1;
  pc.CinP = (int)align_up(pc.Cin, CI_CHUNK), pc.CoutP = (int)align_up(pc.Cout, 32);
  std::vector<float> wp((size_t)pc.CinP * pc.CoutP, 0.f);
  for (int i = 0; i < RMVPE_MELS; ++i)
    for (int k = 0; k < 513; ++k) wp[(size_t)k * pc.CoutP + i] = fb[(size_t)i * 513 + k];
  float *dw = nullptr, *dt = nullptr;
  STY_HIP(hipMalloc((void**)&dw, wp.size() * sizeof(float)));
  STY_HIP(hipMalloc((void**)&dt, taps.size() * sizeof(float)));
  (void)st;  // (pageable host memory: the blocking copies are complete on return, whatever stream the first call runs on)
  STY_HIP(hipMemcpy(dw, wp.data(), wp.size() * sizeof(float), hipMemcpyHostToDevice));
  STY_HIP(hipMemcpy(dt, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
  pc.wp = dw;
  g_mel_basis = pc;
  g_resample_taps = dt;
  return STY_OK;
}
int rmvpe_mel_frames(int N) { return rmvpe_resampled_len(N) / RMVPE_HOP + 1; }
size_t rmvpe_mel_workspace_floats(int B, int N) {
  const size_t M = rmvpe_resampled_len(N), n = rmvpe_mel_frames(N), F = 513;
  return (size_t)B * (align_up(M, 64) + 3 * F * n) + 1024;
}
int launch_rmvpe_mel(int B, int N, const float* audio, float* logmel, float* ws, hipStream_t st) {
  int rc = front_tables(st);
  if (rc) return rc;
  const int M = rmvpe_resampled_len(N), n = rmvpe_mel_frames(N), F = 513;
  float* res = ws;
  float* y = res + (size_t)B * align_up(M, 64);
  float* mag = y + (size_t)B * 2 * F * n;
  if ((rc = launch_resample_fir(audio, g_resample_taps, B, N, M, 3, 2, RS_WIDTH, res, st)) != STY_OK) return rc;
  if ((rc = launch_stft_mag(B, M, res, 1024, RMVPE_HOP, 16000, y, mag, st)) != STY_OK) return rc;
  ConvArgs a;
  a.x[0] = mag;
  a.xc[0] = F;
  a.B = B;
  a.T = n;
  a.w = g_mel_basis;
  a.y = logmel;
  if ((rc = launch_conv1d(a, st)) != STY_OK) return rc;
  const size_t ne = (size_t)B * RMVPE_MELS * n;
  hipLaunchKernelGGL(rmvpe_logmel_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, logmel, ne);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// weight side
// ---------------------------------------------------------------------------------------------------------------------
// one block per output channel.  s = bn_w / sqrt(bn_rv + 1e-5) (1 without a BatchNorm);
// deconv == 0: wp[(kw CinP + kh Cin + ci) CoutP + co_off + co] = w[co][ci][kh][kw] s
// deconv == 1: wp[(ci Cout + co) 9 + k] = w[ci][co][k] s
// bp[co_off + co] = (bias - bn_rm) s + bn_b
__global__ __launch_bounds__(256) void rmvpe_pack_conv_kernel(RmvpePackJob j) {
  const int co = blockIdx.x;
  float s = 1.f, sh = j.bias ? j.bias[co] : 0.f;
  if (j.bn_w) {
    s = j.bn_w[co] / sqrtf(j.bn_rv[co] + 1e-5f);
    sh = (sh - j.bn_rm[co]) * s + j.bn_b[co];
  }
  const int taps = j.KH * j.KW, n = j.Cin * taps;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int ci = i / taps, k = i - ci * taps;
    if (j.deconv) {
      j.wp[((size_t)ci * j.Cout + co) * taps + k] = j.w[((size_t)ci * j.Cout + co) * taps + k] * s;
    } else {
      const int kh = k / j.KW, kw = k - kh * j.KW;
      j.wp[((size_t)kw * j.CinP + kh * j.Cin + ci) * j.CoutP + j.co_off + co] = j.w[(size_t)co * n + i] * s;
    }
  }
  if (threadIdx.x == 0) j.bp[j.co_off + co] = sh;
}
// wt[c][r] = w[r][c]
__global__ __launch_bounds__(256) void rmvpe_transpose_kernel(const float* __restrict__ w, int rows, int cols,
                                                              float* __restrict__ wt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cols) return;
  const int c = i / rows, r = i - c * rows;
  wt[i] = w[(size_t)r * cols + c];
}
// encoder.bn on the one input channel -> ss[0] = scale, ss[1] = shift
__global__ void rmvpe_in_bn_kernel(const float* w, const float* b, const float* rm, const float* rv, float* ss) {
  const float s = w[0] / sqrtf(rv[0] + 1e-5f);
  ss[0] = s;
  ss[1] = b[0] - rm[0] * s;
}
// (one launch per conv, ~130 at full size: the kind is inference-only, so this runs once per loaded checkpoint, not per step)
int rmvpe_prepare(const RmvpePlan& p, hipStream_t st) {
  for (const RmvpePackJob& j : p.packs) hipLaunchKernelGGL(rmvpe_pack_conv_kernel, dim3(j.Cout), dim3(256), 0, st, j);
  for (int d = 0; d < 2; ++d)
    hipLaunchKernelGGL(rmvpe_transpose_kernel, dim3(cdiv(768 * 256, 256)), dim3(256), 0, st, p.whh[d], 768, 256,
                       p.whhT + (size_t)d * 768 * 256);
  hipLaunchKernelGGL(rmvpe_in_bn_kernel, dim3(1), dim3(1), 0, st, p.in_bn[0], p.in_bn[1], p.in_bn[2], p.in_bn[3], p.in_ss);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// network glue
// ---------------------------------------------------------------------------------------------------------------------
// logmel [B][128][n] -> x [B][Tp][129]: x[b][t][w] = logmel[b][w][t < n ? t : 2 (n - 1) - t] * scale + shift, pad column 0
__global__ __launch_bounds__(256) void rmvpe_input_kernel(const float* __restrict__ logmel, const float* __restrict__ ss, int n,
                                                          int Tp, float* __restrict__ x) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const int Wp = RMVPE_MELS + 1;
  if (i >= Tp * Wp) return;
  const int t = i / Wp, w = i - t * Wp;
  float v = 0.f;
  if (w < RMVPE_MELS) {
    const int ts = t < n ? t : 2 * (n - 1) - t;  // (n >= 17: Tp - n <= n - 1)
    v = fmaf(logmel[((size_t)b * RMVPE_MELS + w) * n + ts], ss[0], ss[1]);
  }
  x[(size_t)b * Tp * Wp + i] = v;
}
int launch_rmvpe_input(const float* logmel, const float* ss, int B, int n, int Tp, float* x, hipStream_t st) {
  hipLaunchKernelGGL(rmvpe_input_kernel, dim3(cdiv(Tp * (RMVPE_MELS + 1), 256), B), dim3(256), 0, st, logmel, ss, n, Tp, x);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

constexpr int DC_CO = 8, DC_SPLIT = 4;
// x [B][Cin][Hi][Wi + 1] (padded-flat) -> y[b][co][2 Hi][2 Wi + 1] for co < Cout, with batch stride ybs floats (the concat
// buffer's).  y = relu(acc + bias); the pad column of both output rows is written as zero by the thread of the last column.
// A workgroup is 64 input positions x DC_CO output channels; its DC_SPLIT waves each take a quarter of the input channels
// (the deepest levels have 8 - 32 positions per utterance and 512 input channels: one wave per tile was a chain of 512 dependent
// scalar-load waits, 368 us per launch on average; profiles/pitch_throughput.txt has the split form), the partial sums meet in
// LDS in a fixed order and wave w finishes channels 2 w and 2 w + 1.
__global__ __launch_bounds__(64 * DC_SPLIT) void rmvpe_deconv_kernel(const float* __restrict__ x, const float* __restrict__ wd,
                                                                     const float* __restrict__ bias, int Cin, int Cout, int Hi,
                                                                     int Wi, size_t ybs, float* __restrict__ y) {
  __shared__ float part[DC_SPLIT][4 * DC_CO][64];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: the weights stay scalar loads)
  const int q = blockIdx.x * 64 + lane, co0 = blockIdx.y * DC_CO, b = blockIdx.z;
  const bool live = q < Hi * Wi;
  const int qq = live ? q : 0;
  const int ih = qq / Wi, iw = qq - ih * Wi;
  const int ldi = Wi + 1, ni = Hi * ldi, ldo = 2 * Wi + 1, no = 2 * Hi * ldo;
  const bool down = ih + 1 < Hi;
  const int per = (Cin + DC_SPLIT - 1) / DC_SPLIT, ci0 = wv * per, ci1 = min(Cin, ci0 + per);
  const float* p = x + ((size_t)b * Cin + ci0) * ni + (size_t)ih * ldi + iw;
  float a00[DC_CO], a01[DC_CO], a10[DC_CO], a11[DC_CO];
#pragma unroll
  for (int c = 0; c < DC_CO; ++c) a00[c] = a01[c] = a10[c] = a11[c] = 0.f;
  for (int ci = ci0; ci < ci1; ++ci) {
    const float x00 = p[0], x01 = p[1];  // (iw + 1 == Wi reads the row's zero pad column)
    const float x10 = down ? p[ldi] : 0.f, x11 = down ? p[ldi + 1] : 0.f;
    p += ni;
    const float* w = wd + ((size_t)ci * Cout + co0) * 9;
#pragma unroll
    for (int c = 0; c < DC_CO; ++c) {
      if (co0 + c < Cout) {  // (wave-uniform)
        const float* k = w + c * 9;  // k[kh * 3 + kw]
        a00[c] = fmaf(k[4], x00, a00[c]);
        a01[c] = fmaf(k[3], x01, fmaf(k[5], x00, a01[c]));
        a10[c] = fmaf(k[1], x10, fmaf(k[7], x00, a10[c]));
        a11[c] = fmaf(k[0], x11, fmaf(k[2], x10, fmaf(k[6], x01, fmaf(k[8], x00, a11[c]))));
      }
    }
  }
#pragma unroll
  for (int c = 0; c < DC_CO; ++c) {
    part[wv][4 * c + 0][lane] = a00[c];
    part[wv][4 * c + 1][lane] = a01[c];
    part[wv][4 * c + 2][lane] = a10[c];
    part[wv][4 * c + 3][lane] = a11[c];
  }
  __syncthreads();
  if (!live) return;
  float* o = y + (size_t)b * ybs + (size_t)(2 * ih) * ldo + 2 * iw;
  for (int c = wv * (DC_CO / DC_SPLIT); c < (wv + 1) * (DC_CO / DC_SPLIT) && co0 + c < Cout; ++c) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      v[e] = (part[0][4 * c + e][lane] + part[1][4 * c + e][lane]) + (part[2][4 * c + e][lane] + part[3][4 * c + e][lane]);
    const float bv = bias[co0 + c];
    float* oc = o + (size_t)(co0 + c) * no;
    oc[0] = fmaxf(v[0] + bv, 0.f);
    oc[1] = fmaxf(v[1] + bv, 0.f);
    oc[ldo] = fmaxf(v[2] + bv, 0.f);
    oc[ldo + 1] = fmaxf(v[3] + bv, 0.f);
    if (iw == Wi - 1) {
      oc[2] = 0.f;
      oc[ldo + 2] = 0.f;
    }
  }
}
int launch_rmvpe_deconv(const float* x, const float* wd, const float* bias, int B, int Cin, int Cout, int Hi, int Wi, size_t ybs,
                        float* y, hipStream_t st) {
  ProfScope prof("rmvpe_deconv_kernel", 18.0 * B * Cin * Cout * Hi * Wi, 4.0 * B * Hi * (Wi + 1) * ((double)Cin + 4.0 * Cout), st);
  hipLaunchKernelGGL(rmvpe_deconv_kernel, dim3(cdiv(Hi * Wi, 64), cdiv(Cout, DC_CO), B), dim3(64 * DC_SPLIT), 0, st, x, wd, bias,
                     Cin, Cout, Hi, Wi, ybs, y);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// cnn output [B][3][T][129] -> GRU input [B][3 * 128][T], feature c * 128 + w (model.py:84: transpose(1, 2).flatten(-2))
__global__ __launch_bounds__(256) void rmvpe_gru_in_kernel(const float* __restrict__ x, int T, float* __restrict__ y) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const int Wp = RMVPE_MELS + 1, nf = 3 * RMVPE_MELS;
  if (i >= nf * T) return;
  const int f = i / T, t = i - f * T, c = f / RMVPE_MELS, w = f - c * RMVPE_MELS;
  y[(size_t)b * nf * T + i] = x[((size_t)b * 3 + c) * T * Wp + (size_t)t * Wp + w];
}
int launch_rmvpe_gru_in(const float* x, int B, int T, float* y, hipStream_t st) {
  hipLaunchKernelGGL(rmvpe_gru_in_kernel, dim3(cdiv(3 * RMVPE_MELS * T, 256), B), dim3(256), 0, st, x, T, y);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

constexpr int GRU_H = 256, GRU_G = 4;
__device__ __forceinline__ float rm_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
// xg [B][2 * 768][T] = W_ih x + b_ih (direction-major, gates r, z, n), whhT [2][256][768], bhh [2][768] -> h [B][512][T]
__global__ __launch_bounds__(1024) void rmvpe_gru_kernel(const float* __restrict__ xg, const float* __restrict__ whhT,
                                                         const float* __restrict__ bhh0, const float* __restrict__ bhh1, int B,
                                                         int T, float* __restrict__ hout) {
  __shared__ float h[GRU_G][GRU_H];
  __shared__ float part[4][3][GRU_G][GRU_H];
  const int dir = blockIdx.x & 1, b0 = (blockIdx.x >> 1) * GRU_G;
  const int j = threadIdx.x & (GRU_H - 1), kq = threadIdx.x >> 8;
  const float* W = whhT + (size_t)dir * GRU_H * 3 * GRU_H;
  const float* bh = dir ? bhh1 : bhh0;
  const int b = b0 + kq;               // the utterance this thread applies the gates for
  const bool mine = b < B;             // (kq < GRU_G by construction: four k-quarters, four utterances)
  const float br = bh[j], bz = bh[GRU_H + j], bn = bh[2 * GRU_H + j];
  const float* xb = xg + ((size_t)(mine ? b : 0) * 2 + dir) * 3 * GRU_H * T;
  h[kq][j] = 0.f;
  float hprev = 0.f;
  __syncthreads();
  for (int step = 0; step < T; ++step) {
    const int t = dir ? T - 1 - step : step;
    float xr = 0.f, xz = 0.f, xn = 0.f;
    if (mine) {  // issued ahead of the matrix-vector products that hide their latency
      xr = xb[(size_t)j * T + t];
      xz = xb[(size_t)(GRU_H + j) * T + t];
      xn = xb[(size_t)(2 * GRU_H + j) * T + t];
    }
    float acc[3][GRU_G];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int u = 0; u < GRU_G; ++u) acc[g][u] = 0.f;
#pragma unroll 4
    for (int k = kq * 64; k < kq * 64 + 64; ++k) {
      const float* wk = W + (size_t)k * 3 * GRU_H + j;
      const float w0 = wk[0], w1 = wk[GRU_H], w2 = wk[2 * GRU_H];
#pragma unroll
      for (int u = 0; u < GRU_G; ++u) {
        const float hv = h[u][k];
        acc[0][u] = fmaf(w0, hv, acc[0][u]);
        acc[1][u] = fmaf(w1, hv, acc[1][u]);
        acc[2][u] = fmaf(w2, hv, acc[2][u]);
      }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int u = 0; u < GRU_G; ++u) part[kq][g][u][j] = acc[g][u];
    __syncthreads();  // every read of h for this step is done, every partial sum is visible
    if (mine) {
      const float hr = (part[0][0][kq][j] + part[1][0][kq][j]) + (part[2][0][kq][j] + part[3][0][kq][j]) + br;
      const float hz = (part[0][1][kq][j] + part[1][1][kq][j]) + (part[2][1][kq][j] + part[3][1][kq][j]) + bz;
      const float hn = (part[0][2][kq][j] + part[1][2][kq][j]) + (part[2][2][kq][j] + part[3][2][kq][j]) + bn;
      const float r = rm_sigmoid(xr + hr), z = rm_sigmoid(xz + hz);
      const float nn = tanhf(fmaf(r, hn, xn));
      hprev = fmaf(z, hprev - nn, nn);  // (1 - z) n + z h
      h[kq][j] = hprev;
      hout[((size_t)b * 2 * GRU_H + dir * GRU_H + j) * T + t] = hprev;
    }
    __syncthreads();
  }
}
int launch_rmvpe_gru(const float* xg, const float* whhT, const float* bhh0, const float* bhh1, int B, int T, float* hout,
                     hipStream_t st) {
  const int groups = cdiv(B, GRU_G);
  ProfScope prof("rmvpe_gru_kernel", 2.0 * 2 * B * T * 768.0 * 256.0, 4.0 * (2.0 * groups * T * 768.0 * 256.0 + 4.0 * B * 512.0 * T), st);
  hipLaunchKernelGGL(rmvpe_gru_kernel, dim3(2 * groups), dim3(1024), 0, st, xg, whhT, bhh0, bhh1, B, T, hout);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// logits [B][360][T] -> salience [B][n][360] = sigmoid, the first n frames
__global__ __launch_bounds__(256) void rmvpe_salience_kernel(const float* __restrict__ logits, int T, int n,
                                                             float* __restrict__ sal) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= n * RMVPE_CLASSES) return;
  const int t = i / RMVPE_CLASSES, c = i - t * RMVPE_CLASSES;
  sal[(size_t)b * n * RMVPE_CLASSES + i] = rm_sigmoid(logits[((size_t)b * RMVPE_CLASSES + c) * T + t]);
}
int launch_rmvpe_salience(const float* logits, int B, int T, int n, float* sal, hipStream_t st) {
  hipLaunchKernelGGL(rmvpe_salience_kernel, dim3(cdiv(n * RMVPE_CLASSES, 256), B), dim3(256), 0, st, logits, T, n, sal);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// to_local_average_f0 (utils.py:114-131): one wave per frame.  arg-max with the lowest index on a tie (torch.argmax on equal
// values returns the first), the window [c - 4, c + 5) clipped to [0, 360), cents = sum s (20 i + CONST) / sum s (0 / 1 for
// an all-zero window, as the reference's guard), f0 = 10 * 2^(cents / 1200), 0 where the row's maximum is < thred.  The
// nine-term sums and the power run in double: the result is the fp32 rounding of the exact expression.
__global__ __launch_bounds__(256) void rmvpe_decode_kernel(const float* __restrict__ sal, int rows, float thred,
                                                           float* __restrict__ f0) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* s = sal + (size_t)row * RMVPE_CLASSES;
  float best = -INFINITY;
  int bi = RMVPE_CLASSES;
  for (int i = lane; i < RMVPE_CLASSES; i += 64) {
    const float v = s[i];
    if (v > best) best = v, bi = i;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ob > best || (ob == best && oi < bi)) best = ob, bi = oi;
  }
  if (lane != 0) return;
  float out = 0.f;
  if (bi < RMVPE_CLASSES && !(best < thred)) {
    const int lo = bi - 4 < 0 ? 0 : bi - 4, hi = bi + 5 > RMVPE_CLASSES ? RMVPE_CLASSES : bi + 5;
    double ps = 0.0, ws = 0.0;
    for (int i = lo; i < hi; ++i) {
      const double v = (double)s[i];
      ps += v * (20.0 * i + 1997.3794084376191);
      ws += v;
    }
    const double cents = ps / (ws == 0.0 ? 1.0 : ws);
    out = (float)(10.0 * exp2(cents / 1200.0));
  }
  f0[row] = out;
}
int launch_rmvpe_decode(const float* sal, int rows, float thred, float* f0, hipStream_t st) {
  hipLaunchKernelGGL(rmvpe_decode_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, sal, rows, thred, f0);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

}  // namespace sty
