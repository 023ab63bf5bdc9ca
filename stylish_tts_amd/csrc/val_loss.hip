// Forward-only loss entries for the validation pass (validate_acoustic / _textual / _duration, train/stage_type.py:376-633):
// the VALUES sty_acoustic_loss_fwd_bwd (mel term), sty_pitch_loss_fwd_bwd and sty_duration_loss_fwd_bwd log, without a gradient
// buffer and with reductions whose order is fixed by the shape alone.  A logged validation loss is compared against
// manifest.best_loss across passes, so its last bits must not depend on the order in which workgroups arrive: every workgroup
// stores its float64 partial at its own index (no atomics) and one finalize workgroup adds the partials in index order.
// Calling an entry twice on the same buffers gives equal bits.
#include "model.h"

namespace sty {
namespace {

// sum over the 64 lanes of a wave, the same butterfly every time (the result is in every lane)
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

constexpr int MEL_RES[3][2] = {{512, 128}, {1024, 256}, {2048, 512}};  // multi_spectrogram.py:13-20
constexpr int MEL_G_MAX = 64;   // most workgroups per (resolution, utterance)
constexpr int MEL_PER_WG = 1024;  // elements one workgroup takes before a second one is added
inline int mel_frames(int N, int r) { return N / MEL_RES[r][1] + 1; }
// partial count of one (resolution, utterance): a function of the shape only
inline int mel_groups(int frames) {
  const int g = cdiv(128 * frames, MEL_PER_WG);
  return g < MEL_G_MAX ? g : MEL_G_MAX;
}

// workspace of sty_mel_loss_fwd, in floats; every piece starts at a multiple of 64 floats
struct MelLayout {
  size_t part, item, mag[3][2], scratch, total;  // mag[r][side]: side 0 = target, 1 = prediction
};
MelLayout mel_layout(int B, int N) {
  MelLayout l;
  size_t p = 0;
  auto take = [&](size_t n) {
    const size_t q = p;
    p += (n + 63) / 64 * 64;
    return q;
  };
  l.part = take((size_t)3 * B * MEL_G_MAX * 2 * 2);  // [3][B][MEL_G_MAX][2] doubles
  l.item = take((size_t)B * 3 * 2 * 2);              // [B][3][2] doubles
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 2; ++s) l.mag[r][s] = take((size_t)B * 128 * mel_frames(N, r));
  l.scratch = take(loss_features_scratch_floats(B, N));
  l.total = p;
  return l;
}

// part[(b * G + g) * 2 + {0: sum |t - p|, 1: sum |t|}] over the elements (m, fr) of utterance b that workgroup g takes;
// t, p [128][B][frames] (batch-folded)
__global__ __launch_bounds__(256) void mel_partial_kernel(const float* __restrict__ t, const float* __restrict__ p, int B,
                                                          int frames, double* __restrict__ part) {
  __shared__ double red[2][4];
  const int g = blockIdx.x, G = gridDim.x, b = blockIdx.y;
  const unsigned n = 128u * (unsigned)frames;
  double a0 = 0.0, a1 = 0.0;
  for (unsigned i = (unsigned)g * 256u + threadIdx.x; i < n; i += (unsigned)G * 256u) {
    const unsigned m = i / (unsigned)frames, fr = i - m * (unsigned)frames;
    const size_t o = ((size_t)m * B + b) * frames + fr;
    const float tv = t[o];
    a0 += (double)fabsf(tv - p[o]);
    a1 += (double)fabsf(tv);
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = a0;
    red[1][wave] = a1;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    part[((size_t)b * G + g) * 2 + threadIdx.x] =
        ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

struct MelGroups {
  int g[3];
};
// one workgroup: item[b][r][2] = the partials of (r, b) added in index order; loss = mean_r sum_b num / (sum_b den + 1e-6),
// items in index order (loss_finalize_kernel's formula)
__global__ __launch_bounds__(256) void mel_finalize_kernel(const double* __restrict__ part, MelGroups mg, int B,
                                                           double* __restrict__ item, double* __restrict__ per_item,
                                                           float* __restrict__ loss) {
  __shared__ double tot[3][2];
  for (int q = threadIdx.x; q < 3 * B; q += 256) {
    const int r = q / B, b = q - r * B, G = mg.g[r];
    const double* pp = part + ((size_t)r * B * MEL_G_MAX + (size_t)b * G) * 2;
    double num = 0.0, den = 0.0;
    for (int g = 0; g < G; ++g) {
      num += pp[2 * g];
      den += pp[2 * g + 1];
    }
    item[((size_t)b * 3 + r) * 2] = num;
    item[((size_t)b * 3 + r) * 2 + 1] = den;
    if (per_item) {
      per_item[((size_t)b * 3 + r) * 2] = num;
      per_item[((size_t)b * 3 + r) * 2 + 1] = den;
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int r = threadIdx.x >> 1, k = threadIdx.x & 1;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += item[((size_t)b * 3 + r) * 2 + k];
    tot[r][k] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double mel = 0.0;
    for (int r = 0; r < 3; ++r) mel += tot[r][0] / (tot[r][1] + 1e-6);
    loss[0] = (float)(mel / 3.0);
  }
}

__device__ __forceinline__ float vsl1(float d) { return fabsf(d) < 1.f ? 0.5f * d * d : fabsf(d) - 0.5f; }

// one wave per curve: part[b][{0: sum smooth_l1(pred - target), 1: sum smooth_l1 of the first differences}] (the terms of
// pitch_loss_sums_kernel, each an fp32 value, added in float64)
__global__ __launch_bounds__(64) void pitch_partial_kernel(const float* __restrict__ tg, const float* __restrict__ pr, int T,
                                                           double* __restrict__ part) {
  const int b = blockIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int t = threadIdx.x; t < T; t += 64) {
    const size_t o = (size_t)b * T + t;
    s0 += (double)vsl1(pr[o] - tg[o]);
    if (t + 1 < T) s1 += (double)vsl1((pr[o + 1] - pr[o]) - (tg[o + 1] - tg[o]));
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (threadIdx.x == 0) {
    part[2 * b] = s0;
    part[2 * b + 1] = s1;
  }
}
// curves in index order; the value pitch_loss_grad_kernel writes (T > 1 guards the difference term)
__global__ void pitch_finalize_kernel(const double* __restrict__ part, int B, int T, float* __restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.0, c = 0.0;
  for (int b = 0; b < B; ++b) {
    a += part[2 * b];
    c += part[2 * b + 1];
  }
  const double n0 = (double)B * T, n1 = (double)B * (T - 1);
  loss[0] = (float)(a / n0 + (T > 1 ? c / n1 : 0.0));
}

// one wave per item, the terms of duration_loss_sums_kernel: part[b] = {item_dur / B, item_ce / B}
__global__ __launch_bounds__(64) void duration_partial_kernel(const float* __restrict__ pred, const int64_t* __restrict__ lengths,
                                                              const float* __restrict__ tgt, const int64_t* __restrict__ cls,
                                                              const float* __restrict__ tab, const float* __restrict__ cw,
                                                              int B, int L, int NC, double* __restrict__ part) {
  const int b = blockIdx.x;
  const int len = (int)lengths[b];
  const int lim = len < L ? len : L;  // (a length beyond the tensor must not be read; it is a caller's error either way)
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int l = threadIdx.x; l < lim; l += 64) {
    const float* z = pred + ((size_t)b * L + l) * NC;
    float p[32];
    float mx = z[0];
    for (int c = 1; c < NC; ++c) mx = fmaxf(mx, z[c]);
    float den = 0.f;
    for (int c = 0; c < NC; ++c) {
      p[c] = expf(z[c] - mx);
      den += p[c];
    }
    float S = 0.f, E = 0.f;
    for (int c = 0; c < NC; ++c) {
      p[c] /= den;
      S += p[c];
      E = fmaf(p[c], tab[c], E);
    }
    s0 += (double)vsl1(E / (S + 1e-9f) - tgt[(size_t)b * L + l]);
    int y = (int)cls[(size_t)b * L + l];
    y = y < 0 ? 0 : (y >= NC ? NC - 1 : y);
    s1 += (double)(cw[y] * -logf(fmaxf(p[y], 1e-38f)));
    s2 += (double)cw[y];
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (threadIdx.x == 0) {
    part[2 * b] = s0 / ((double)len * B);
    part[2 * b + 1] = s1 / (s2 * B);
  }
}
__global__ void duration_finalize_kernel(const double* __restrict__ part, int B, float* __restrict__ losses) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.0, c = 0.0;
  for (int b = 0; b < B; ++b) {
    a += part[2 * b];
    c += part[2 * b + 1];
  }
  losses[0] = (float)a;
  losses[1] = (float)c;
}

}  // namespace
}  // namespace sty

extern "C" {

int sty_mel_loss_workspace_bytes(int B, int N, size_t* bytes) {
  if (!bytes || B <= 0 || N <= 1024) {
    sty::set_error("sty_mel_loss_workspace_bytes: bad argument (B > 0, N > 1024: the 2048-point transform reflect-pads 1024 samples)");
    return STY_EINVAL;
  }
  *bytes = sty::mel_layout(B, N).total * sizeof(float);
  return STY_OK;
}

int sty_mel_loss_features(int B, int N, int resolution, int side, size_t* offset_bytes, int* frames) {
  if (!offset_bytes || !frames || B <= 0 || N <= 1024 || resolution < 0 || resolution > 2 || side < 0 || side > 1) {
    sty::set_error("sty_mel_loss_features: bad argument (resolution 0..2, side 0 = target / 1 = prediction)");
    return STY_EINVAL;
  }
  *offset_bytes = sty::mel_layout(B, N).mag[resolution][side] * sizeof(float);
  *frames = sty::mel_frames(N, resolution);
  return STY_OK;
}

int sty_mel_loss_fwd(int B, int N, const float* audio_gt, const float* audio_pred, float* loss, double* per_item,
                     void* workspace, size_t ws_bytes, void* stream) {
  if (!audio_gt || !audio_pred || !loss || !workspace || B <= 0 || N <= 1024) {
    sty::set_error("sty_mel_loss_fwd: bad argument (B > 0, N > 1024, no NULL but per_item)");
    return STY_EINVAL;
  }
  const sty::MelLayout l = sty::mel_layout(B, N);
  if (ws_bytes < l.total * sizeof(float)) {
    sty::set_error("sty_mel_loss_fwd: workspace too small (%zu bytes, sty_mel_loss_workspace_bytes says %zu)", ws_bytes,
                   l.total * sizeof(float));
    return STY_ENOMEM;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  double* part = reinterpret_cast<double*>(ws + l.part);
  double* item = reinterpret_cast<double*>(ws + l.item);
  sty::MelGroups mg;
  for (int r = 0; r < 3; ++r) {
    const int frames = sty::mel_frames(N, r);
    mg.g[r] = sty::mel_groups(frames);
    for (int s = 0; s < 2; ++s) {
      int rc = sty::launch_loss_features(B, N, s == 0 ? audio_gt : audio_pred, r, ws + l.mag[r][s], ws + l.scratch, st);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(sty::mel_partial_kernel, dim3(mg.g[r], B), dim3(256), 0, st, ws + l.mag[r][0], ws + l.mag[r][1], B,
                       frames, part + (size_t)r * B * sty::MEL_G_MAX * 2);
  }
  hipLaunchKernelGGL(sty::mel_finalize_kernel, dim3(1), dim3(256), 0, st, part, mg, B, item, per_item, loss);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

int sty_pitch_loss_fwd(int B, int T, const float* target, const float* pred, float* loss, void* workspace, size_t ws_bytes,
                       void* stream) {
  if (!target || !pred || !loss || !workspace || B <= 0 || T <= 0 || ws_bytes < (size_t)B * 16) {
    sty::set_error("sty_pitch_loss_fwd: bad argument (workspace >= 16 B bytes)");
    return STY_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(sty::pitch_partial_kernel, dim3(B), dim3(64), 0, st, target, pred, T, part);
  hipLaunchKernelGGL(sty::pitch_finalize_kernel, dim3(1), dim3(64), 0, st, part, B, T, loss);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

int sty_duration_loss_fwd(int B, int L, int NC, const float* pred, const int64_t* text_lengths, const float* target_dur,
                          const int64_t* target_class, const float* class_table, const float* ce_weight, float* losses,
                          void* workspace, size_t ws_bytes, void* stream) {
  if (!pred || !text_lengths || !target_dur || !target_class || !class_table || !ce_weight || !losses || !workspace ||
      B <= 0 || L <= 0 || NC <= 0 || NC > 32 || ws_bytes < (size_t)B * 16) {
    sty::set_error("sty_duration_loss_fwd: bad argument (<= 32 classes, workspace >= 16 B bytes)");
    return STY_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(sty::duration_partial_kernel, dim3(B), dim3(64), 0, st, pred, text_lengths, target_dur, target_class,
                     class_table, ce_weight, B, L, NC, part);
  hipLaunchKernelGGL(sty::duration_finalize_kernel, dim3(1), dim3(64), 0, st, part, B, losses);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

}  // extern "C"
