// WavLM forward for the slm loss value (WavLMLoss, train/losses.py:376-394; transformers' modeling_wavlm.py in eval mode):
// everything of it that is not a dense conv on launch_conv1d, an attention launch (attn.hip, the gated relative-bias variant)
// or a channel LayerNorm (norms.hip).  plan_wavlm.hip has the plan (wavlm_forward), weights.hip the packs.
//
// (1) Feature encoder, layer 0 (Conv1d(1, C, k, stride s), bias-free; k = 10, s = 5 at full size): bandwidth work.
//     wavlm_conv0_kernel writes the conv's output [B][C][T0] and, from the same registers, the float64 (sum, sum of squares)
//     partial of every (b, c, 256-frame tile): GroupNorm(C, C) is a per-(b, c) norm over the whole time axis, up to 20 799 frames
//     at the c3 wave size.  wavlm_gn_finalize_kernel adds the tiles in index order and folds the affine into (a, s).
// (2) Layers 1 .. n - 1 (stride s, k taps, C -> C'): a stride-s conv over C channels is a stride-1 conv of ceil(k / s) taps over
//     the s C channels of the input read s frames at a time.  wavlm_stage_kernel writes that view, phase-major
//     (y[p C + c][t] = x[c][s t + p]), applying layer 0's norm and GELU on the way for layer 1 (one pass, not three); the conv
//     itself is launch_conv1d on the fp32 matrix cores with the weights packed for the view (weights.hip) and GELU in its
//     epilogue.
// (3) Positional conv (grouped, k even): wavlm_group_perm_kernel turns [B][G Cg][T] into [G][B][Cg][T], one dense conv per group
//     writes x + GELU(conv(x)) in that layout (the last output frame of the even kernel is never computed), the inverse
//     permutation leads into the LayerNorm.
// (4) Attention glue: wavlm_rel_table_kernel (rel_attn_embed through the host bucket table -> [H][2T - 1], once per call),
//     wavlm_gate_kernel (gru_rel_pos_linear on the layer INPUT's head slice -> [B][H][T]).
// (5) wavlm_transpose_out_kernel: [B][C][T] -> the [B][T][C] hidden state the loss reads.
// (6) slm_loss kernels: mean |a - b| with float64 partials at fixed indices, added in index order (val_loss.hip's discipline);
//     with d_b set also scale * sign(b - a) / n, the term's cotangent.
// (7) The backward to the wave (the network is frozen: input gradients only; plan_wavlm.hip has the plan, wavlm_backward): the
//     cotangent intake, the gate backward, the un-staging of a strided conv's view with the GELU' of the layer below, the
//     GroupNorm(C, C) backward with float64 tile partials, layer 0 transposed.  The dense steps are launch_conv1d on
//     input-gradient packs, the attention backward with the gated bias is attn_bwd.hip's, the resampler adjoint rmvpe.hip's.
#include <math.h>

#include "model.h"

namespace sty {
namespace {
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
constexpr int C0_CG = 8;      // channels per workgroup of wavlm_conv0_kernel
constexpr int C0_MAXK = 16;   // most taps of layer 0
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// feature encoder, layer 0 + GroupNorm sums
// ---------------------------------------------------------------------------------------------------------------------
int wavlm_conv0_ntiles(int T) { return cdiv(T, 256); }
// x [B][N], w [C][K] -> y[b][c][t] = sum_k w[c][k] x[b][S t + k] (S t + k < N by T's definition);
// part[((b C + c) ntiles + tile) 2 + {0, 1}] = sum, sum of squares of the tile's frames
__global__ __launch_bounds__(256) void wavlm_conv0_kernel(const float* __restrict__ x, const float* __restrict__ w, int N, int C, int K,
                                                          int S, int T, float* __restrict__ y, double* __restrict__ part) {
  __shared__ double red[2][C0_CG][4];
  const int t = blockIdx.x * 256 + threadIdx.x, c0 = blockIdx.y * C0_CG, b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool in = t < T;
  float xv[C0_MAXK];
  const float* xb = x + (size_t)b * N + (size_t)S * (in ? t : 0);
#pragma unroll
  for (int k = 0; k < C0_MAXK; ++k) xv[k] = (in && k < K) ? xb[k] : 0.f;
#pragma unroll
  for (int cc = 0; cc < C0_CG; ++cc) {
    const int c = c0 + cc;
    if (c >= C) break;  // (uniform)
    const float* wc = w + (size_t)c * K;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < C0_MAXK; ++k)
      if (k < K) acc = fmaf(wc[k], xv[k], acc);
    if (in) y[((size_t)b * C + c) * T + t] = acc;
    const double v = in ? (double)acc : 0.0;
    const double s1 = wave_sum(v), s2 = wave_sum(v * v);
    if (lane == 0) {
      red[0][cc][wave] = s1;
      red[1][cc][wave] = s2;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * C0_CG) {
    const int cc = threadIdx.x >> 1, k = threadIdx.x & 1;
    if (c0 + cc < C)
      part[(((size_t)b * C + c0 + cc) * gridDim.x + blockIdx.x) * 2 + k] =
          ((red[k][cc][0] + red[k][cc][1]) + red[k][cc][2]) + red[k][cc][3];
  }
}
int launch_wavlm_conv0(const float* x, const float* w, int B, int N, int C, int K, int S, int T, float* y, double* part, hipStream_t st) {
  if (K > C0_MAXK) {
    set_error("wavlm: the first feature conv has %d taps (at most %d are built)", K, C0_MAXK);
    return STY_EINVAL;
  }
  ProfScope prof("wavlm_conv0_kernel", 2.0 * K * B * C * T, 4.0 * B * ((double)N + (double)C * T), st);
  hipLaunchKernelGGL(wavlm_conv0_kernel, dim3(wavlm_conv0_ntiles(T), cdiv(C, C0_CG), B), dim3(256), 0, st, x, w, N, C, K, S, T, y, part);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
// GroupNorm(C, C): per row (b, c) mean and biased variance over T frames from the tile partials, added in index order;
// a = w[c] rstd, s = b[c] - a mean
__global__ __launch_bounds__(256) void wavlm_gn_finalize_kernel(const double* __restrict__ part, int ntiles, const float* __restrict__ w,
                                                                const float* __restrict__ bv, int BC, int C, int T, float eps,
                                                                float* __restrict__ a, float* __restrict__ s,
                                                                float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= BC) return;
  const double* p = part + (size_t)row * ntiles * 2;
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < ntiles; ++i) {
    s1 += p[2 * i];
    s2 += p[2 * i + 1];
  }
  const double mean = s1 / T;
  double var = s2 / T - mean * mean;
  var = var < 0.0 ? 0.0 : var;
  const int c = row % C;
  const double av = (double)w[c] / sqrt(var + (double)eps);
  a[row] = (float)av;
  s[row] = (float)((double)bv[c] - av * mean);
  if (mean_out) {  // kept for the backward (forward_keep)
    mean_out[row] = (float)mean;
    rstd_out[row] = (float)(1.0 / sqrt(var + (double)eps));
  }
}
int launch_wavlm_gn_finalize(const double* part, int ntiles, const float* w, const float* b, int BC, int C, int T, float eps, float* a,
                             float* s, hipStream_t st, float* mean_out, float* rstd_out) {
  hipLaunchKernelGGL(wavlm_gn_finalize_kernel, dim3(cdiv(BC, 256)), dim3(256), 0, st, part, ntiles, w, b, BC, C, T, eps, a, s, mean_out,
                     rstd_out);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the s-frames-at-a-time view of a strided conv's input
// ---------------------------------------------------------------------------------------------------------------------
// MODE 0: the view alone; 1: layer 0's norm and GELU on the way; 2: GELU alone (forward_keep: the convs leave pre-activations)
template <int MODE>
__global__ __launch_bounds__(256) void wavlm_stage_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                          const float* __restrict__ s, int C, int Tin, int S, int Tp,
                                                          float* __restrict__ y) {
  const int t = blockIdx.x * 256 + threadIdx.x, pc = blockIdx.y, b = blockIdx.z;
  if (t >= Tp) return;
  const int p = pc / C, c = pc - p * C;
  const long long ts = (long long)S * t + p;
  float v = 0.f;
  if (ts < Tin) {
    v = x[((size_t)b * C + c) * Tin + ts];
    if constexpr (MODE == 1) v = gelu_erf(fmaf(v, a[(size_t)b * C + c], s[(size_t)b * C + c]));
    if constexpr (MODE == 2) v = gelu_erf(v);
  }
  y[((size_t)b * S * C + pc) * Tp + t] = v;
}
int launch_wavlm_stage(const float* x, const float* a, const float* s, int B, int C, int Tin, int S, int Tp, float* y, hipStream_t st,
                       int gelu_in) {
  const dim3 grid(cdiv(Tp, 256), S * C, B);
  ProfScope prof("wavlm_stage_kernel", 0.0, 8.0 * B * S * (double)C * Tp, st);
  if (a)
    hipLaunchKernelGGL(wavlm_stage_kernel<1>, grid, dim3(256), 0, st, x, a, s, C, Tin, S, Tp, y);
  else if (gelu_in)
    hipLaunchKernelGGL(wavlm_stage_kernel<2>, grid, dim3(256), 0, st, x, a, s, C, Tin, S, Tp, y);
  else
    hipLaunchKernelGGL(wavlm_stage_kernel<0>, grid, dim3(256), 0, st, x, a, s, C, Tin, S, Tp, y);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// bf16 operand mode (sty_wavlm_set_compute): the same view with the input's rows `xrs` floats apart (a conv that ran as a
// same-length conv over its padded view leaves rows of Tp, not T, columns) and, H, written once as the bf16 operand twin the conv
// multiplies (ConvArgs::x16): the affine, the GELU and the rounding (RNE) happen here, the conv converts nothing.  A thread owns
// frame t of channel c and walks its S phases: the S consecutive input floats of a frame are read by one thread, the stores of a
// wave are 128 (H) or 256 consecutive bytes per phase.
template <int MODE, bool H>
__global__ __launch_bounds__(256) void wavlm_stage_rs_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                             const float* __restrict__ s, int C, int Tin, int xrs, int S, int Tp,
                                                             void* __restrict__ y) {
  const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (t >= Tp) return;
  const float* xr = x + ((size_t)b * C + c) * xrs;
  float av = 0.f, sv = 0.f;
  if constexpr (MODE == 1) av = a[(size_t)b * C + c], sv = s[(size_t)b * C + c];
  for (int p = 0; p < S; ++p) {
    const long long ts = (long long)S * t + p;
    float v = 0.f;
    if (ts < Tin) {
      v = xr[ts];
      if constexpr (MODE == 1) v = gelu_erf(fmaf(v, av, sv));
      if constexpr (MODE == 2) v = gelu_erf(v);
    }
    sty_st_any(y, ((size_t)b * S * C + (size_t)p * C + c) * Tp + t, v, H);
  }
}
int launch_wavlm_stage_rs(const float* x, const float* a, const float* s, int B, int C, int Tin, int xrs, int S, int Tp, void* y,
                          int y16, hipStream_t st, int gelu_in) {
  if (xrs < Tin) {
    set_error("wavlm: staged rows of %d frames on a row stride of %d", Tin, xrs);
    return STY_EINVAL;
  }
  const dim3 grid(cdiv(Tp, 256), C, B);
  ProfScope prof(y16 ? "wavlm_stage_rs_kernel<16>" : "wavlm_stage_rs_kernel<32>", 0.0, (y16 ? 6.0 : 8.0) * B * S * (double)C * Tp, st);
#define STY_STAGE_RS(MODE)                                                                                                  \
  do {                                                                                                                      \
    if (y16)                                                                                                                \
      hipLaunchKernelGGL((wavlm_stage_rs_kernel<MODE, true>), grid, dim3(256), 0, st, x, a, s, C, Tin, xrs, S, Tp, y);      \
    else                                                                                                                    \
      hipLaunchKernelGGL((wavlm_stage_rs_kernel<MODE, false>), grid, dim3(256), 0, st, x, a, s, C, Tin, xrs, S, Tp, y);     \
  } while (0)
  if (a)
    STY_STAGE_RS(1);
  else if (gelu_in)
    STY_STAGE_RS(2);
  else
    STY_STAGE_RS(0);
#undef STY_STAGE_RS
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// positional conv: group-major layout
// ---------------------------------------------------------------------------------------------------------------------
// to_groups: y[g][b][c][t] = x[b][g Cg + c][t]; otherwise the inverse
__global__ __launch_bounds__(256) void wavlm_group_perm_kernel(const float* __restrict__ x, int B, int G, int Cg, int T, int to_groups,
                                                               float* __restrict__ y) {
  const int t = blockIdx.x * 256 + threadIdx.x, gc = blockIdx.y, b = blockIdx.z;
  if (t >= T) return;
  const int g = gc / Cg, c = gc - g * Cg;
  const size_t flat = ((size_t)b * G * Cg + gc) * T + t, grp = (((size_t)g * B + b) * Cg + c) * T + t;
  if (to_groups)
    y[grp] = x[flat];
  else
    y[flat] = x[grp];
}
int launch_wavlm_group_perm(const float* x, int B, int G, int Cg, int T, int to_groups, float* y, hipStream_t st) {
  hipLaunchKernelGGL(wavlm_group_perm_kernel, dim3(cdiv(T, 256), G * Cg, B), dim3(256), 0, st, x, B, G, Cg, T, to_groups, y);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// attention glue
// ---------------------------------------------------------------------------------------------------------------------
// _relative_positions_bucket (modeling_wavlm.py) of the distances d = j - i in -(T - 1) .. T - 1, in the class's order of
// operations; out[d + T - 1].  (fp32 and float64 arithmetic agree on every distance 0 .. 2047 for (320, 800) and (32, 64);
// tests/golden/slm_small.json holds the class's own tables)
void wavlm_rel_buckets(int T, int num_buckets, int max_distance, int32_t* out) {
  const int nb = num_buckets / 2, max_exact = nb / 2;
  for (int d = -(T - 1); d <= T - 1; ++d) {
    int bucket = d > 0 ? nb : 0;
    const int n = d < 0 ? -d : d;
    if (n < max_exact) {
      bucket += n;
    } else {
      float v = logf((float)n / (float)max_exact);
      v = v / (float)log((double)max_distance / (double)max_exact);
      v = v * (float)(nb - max_exact);
      int large = (int)((float)max_exact + v);
      if (large > nb - 1) large = nb - 1;
      bucket += large;
    }
    out[d + T - 1] = bucket;
  }
}
// tab[h][d] = embed[bucket[d]][h], d < 2T - 1
__global__ __launch_bounds__(256) void wavlm_rel_table_kernel(const float* __restrict__ embed, const int32_t* __restrict__ bucket, int H,
                                                              int n, float* __restrict__ tab) {
  const int d = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
  if (d >= n) return;
  tab[(size_t)h * n + d] = embed[(size_t)bucket[d] * H + h];
}
int launch_wavlm_rel_table(const float* embed, const int32_t* bucket, int H, int T, float* tab, hipStream_t st) {
  hipLaunchKernelGGL(wavlm_rel_table_kernel, dim3(cdiv(2 * T - 1, 256), H), dim3(256), 0, st, embed, bucket, H, 2 * T - 1, tab);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
// x [B][H DH][T] -> gate[b][h][t] = ga (gb const[h] - 1) + 2 with (ga, gb) = sigmoid of the two sums of four of
// Linear(DH, 8)(x[b][h DH .. (h + 1) DH][t])
__global__ __launch_bounds__(256) void wavlm_gate_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bv, const float* __restrict__ cst, int H, int DH,
                                                         int T, float* __restrict__ gate) {
  const int t = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y, b = blockIdx.z;
  if (t >= T) return;
  const float* xp = x + ((size_t)b * H + h) * DH * T + t;
  float r[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) r[o] = 0.f;
  for (int d = 0; d < DH; ++d) {
    const float v = xp[(size_t)d * T];
#pragma unroll
    for (int o = 0; o < 8; ++o) r[o] = fmaf(w[o * DH + d], v, r[o]);
  }
#pragma unroll
  for (int o = 0; o < 8; ++o) r[o] += bv[o];
  const float sa = ((r[0] + r[1]) + r[2]) + r[3], sb = ((r[4] + r[5]) + r[6]) + r[7];
  const float ga = 1.0f / (1.0f + expf(-sa)), gb = 1.0f / (1.0f + expf(-sb));
  gate[((size_t)b * H + h) * T + t] = fmaf(ga, fmaf(gb, cst[h], -1.0f), 2.0f);
}
int launch_wavlm_gate(const float* x, const float* w, const float* b, const float* c, int B, int H, int DH, int T, float* gate,
                      hipStream_t st) {
  hipLaunchKernelGGL(wavlm_gate_kernel, dim3(cdiv(T, 256), H, B), dim3(256), 0, st, x, w, b, c, H, DH, T, gate);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// [B][C][T] -> [B][T][C] through a 32 x 33 LDS tile
__global__ __launch_bounds__(256) void wavlm_transpose_out_kernel(const float* __restrict__ x, int C, int T, float* __restrict__ y) {
  __shared__ float tile[32][33];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, t = t0 + tx;
    tile[r][tx] = (c < C && t < T) ? x[((size_t)b * C + c) * T + t] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int t = t0 + r, c = c0 + tx;
    if (t < T && c < C) y[((size_t)b * T + t) * C + c] = tile[tx][r];
  }
}
int launch_wavlm_transpose_out(const float* x, int B, int C, int T, float* y, hipStream_t st) {
  hipLaunchKernelGGL(wavlm_transpose_out_kernel, dim3(cdiv(T, 32), cdiv(C, 32), B), dim3(256), 0, st, x, C, T, y);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// slm loss: mean |a - b|
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SLM_G_MAX = 1024, SLM_PER_WG = 8192;
int slm_loss_groups(size_t n) {
  const size_t g = (n + SLM_PER_WG - 1) / SLM_PER_WG;
  return g < 1 ? 1 : (g < (size_t)SLM_G_MAX ? (int)g : SLM_G_MAX);
}
// GRAD: also d_b[i] = mag sign(b[i] - a[i]) (0 at a tie), mag = scale / n formed on the host
template <bool GRAD>
__global__ __launch_bounds__(256) void slm_loss_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                                                               double* __restrict__ part, float mag, float* __restrict__ d_b) {
  __shared__ double red[4];
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    acc += (double)fabsf(a[i] - b[i]);
    if constexpr (GRAD) {
      const float d = b[i] - a[i];
      d_b[i] = d > 0.f ? mag : (d < 0.f ? -mag : 0.f);
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ void slm_loss_finalize_kernel(const double* __restrict__ part, int G, size_t n, float* __restrict__ loss) {
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += part[g];
  loss[0] = (float)(s / (double)n);
}
int launch_slm_loss(size_t n, const float* a, const float* b, float* loss, double* part, hipStream_t st, float mag, float* d_b) {
  const int G = slm_loss_groups(n);
  ProfScope prof("slm_loss_partial_kernel", 2.0 * n, (d_b ? 12.0 : 8.0) * n, st);
  if (d_b)
    hipLaunchKernelGGL(slm_loss_partial_kernel<true>, dim3(G), dim3(256), 0, st, a, b, n, part, mag, d_b);
  else
    hipLaunchKernelGGL(slm_loss_partial_kernel<false>, dim3(G), dim3(256), 0, st, a, b, n, part, mag, d_b);
  hipLaunchKernelGGL(slm_loss_finalize_kernel, dim3(1), dim3(1), 0, st, part, G, n, loss);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// backward to the wave (plan_wavlm.hip: wavlm_backward).  The network is frozen: input gradients only, no float atomic anywhere --
// every output element has one writer and every sum a fixed order, so the gradient repeats to the bit.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ float gelu_erf_grad(float v) {
  return 0.5f * (1.0f + erff(v * 0.70710678118654752f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
}
}  // namespace

// forward_keep: y = res + GELU(pre) (res optional), the epilogue the convs apply themselves in the plain forward
__global__ __launch_bounds__(256) void wavlm_gelu_kernel(const float* __restrict__ pre, const float* __restrict__ res, size_t n,
                                                         float* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float g = gelu_erf(pre[i]);
  y[i] = res ? fmaf(1.f, g, res[i]) : g;
}
int launch_wavlm_gelu(const float* pre, const float* res, size_t n, float* y, hipStream_t st) {
  hipLaunchKernelGGL(wavlm_gelu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pre, res, n, y);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// cotangent intake, the inverse of wavlm_transpose_out_kernel with an add: dx[b][c][t] (+)= dh[b][t][c]
__global__ __launch_bounds__(256) void wavlm_intake_kernel(const float* __restrict__ dh, int C, int T, int accumulate,
                                                           float* __restrict__ dx) {
  __shared__ float tile[32][33];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int t = t0 + r, c = c0 + tx;
    tile[r][tx] = (t < T && c < C) ? dh[((size_t)b * T + t) * C + c] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, t = t0 + tx;
    if (c < C && t < T) {
      const size_t o = ((size_t)b * C + c) * T + t;
      dx[o] = accumulate ? dx[o] + tile[tx][r] : tile[tx][r];
    }
  }
}
int launch_wavlm_intake(const float* dh, int B, int C, int T, int accumulate, float* dx, hipStream_t st) {
  hipLaunchKernelGGL(wavlm_intake_kernel, dim3(cdiv(T, 32), cdiv(C, 32), B), dim3(256), 0, st, dh, C, T, accumulate, dx);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// gate = ga (gb const_h - 1) + 2 backward: dgate [B][H][T] through the two sigmoids and Linear(DH, 8) into the head slice of the
// layer input's gradient, dx[b][h DH + d][t] += ...; one thread owns (b, h, t) and with it the DH elements it adds to
__global__ __launch_bounds__(256) void wavlm_gate_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bv, const float* __restrict__ cst,
                                                             const float* __restrict__ dgate, int H, int DH, int T,
                                                             float* __restrict__ dx) {
  const int t = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y, b = blockIdx.z;
  if (t >= T) return;
  const size_t off = ((size_t)b * H + h) * DH * T + t;
  const float* xp = x + off;
  float r[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) r[o] = 0.f;
  for (int d = 0; d < DH; ++d) {
    const float v = xp[(size_t)d * T];
#pragma unroll
    for (int o = 0; o < 8; ++o) r[o] = fmaf(w[o * DH + d], v, r[o]);
  }
#pragma unroll
  for (int o = 0; o < 8; ++o) r[o] += bv[o];
  const float sa = ((r[0] + r[1]) + r[2]) + r[3], sb = ((r[4] + r[5]) + r[6]) + r[7];
  const float ga = 1.0f / (1.0f + expf(-sa)), gb = 1.0f / (1.0f + expf(-sb));
  const float dg = dgate[((size_t)b * H + h) * T + t], c = cst[h];
  const float dsa = dg * fmaf(gb, c, -1.0f) * ga * (1.0f - ga), dsb = dg * ga * c * gb * (1.0f - gb);
  float* dp = dx + off;
  for (int d = 0; d < DH; ++d) {
    const float wa = ((w[d] + w[DH + d]) + w[2 * DH + d]) + w[3 * DH + d];
    const float wb = ((w[4 * DH + d] + w[5 * DH + d]) + w[6 * DH + d]) + w[7 * DH + d];
    dp[(size_t)d * T] += fmaf(wa, dsa, wb * dsb);
  }
}
int launch_wavlm_gate_bwd(const float* x, const float* w, const float* b, const float* c, const float* dgate, int B, int H, int DH,
                          int T, float* dx, hipStream_t st) {
  hipLaunchKernelGGL(wavlm_gate_bwd_kernel, dim3(cdiv(T, 256), H, B), dim3(256), 0, st, x, w, b, c, dgate, H, DH, T, dx);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// un-staging, the adjoint of wavlm_stage_kernel: dx[b][c][S t + p] = dview[b][p C + c][t], zero for frames past the view
// (t >= Tp), times GELU'(pre) of the layer below (pre [B][C][Tin], its conv's pre-activation)
__global__ __launch_bounds__(256) void wavlm_unstage_kernel(const float* __restrict__ dview, const float* __restrict__ pre, int C,
                                                            int Tin, int S, int Tp, float* __restrict__ dx) {
  const int ts = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (ts >= Tin) return;
  const int t = ts / S, p = ts - t * S;
  const size_t o = ((size_t)b * C + c) * Tin + ts;
  const float g = t < Tp ? dview[((size_t)b * S * C + (size_t)p * C + c) * Tp + t] : 0.f;
  dx[o] = g * gelu_erf_grad(pre[o]);
}
int launch_wavlm_unstage(const float* dview, const float* pre, int B, int C, int Tin, int S, int Tp, float* dx, hipStream_t st) {
  ProfScope prof("wavlm_unstage_kernel", 0.0, 12.0 * B * (double)C * Tin, st);
  hipLaunchKernelGGL(wavlm_unstage_kernel, dim3(cdiv(Tin, 256), C, B), dim3(256), 0, st, dview, pre, C, Tin, S, Tp, dx);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// bf16 operand mode: the same with `pre` on rows of prs floats and the result on rows of ors >= Tin elements, fp32 or (H) the
// bf16 operand twin of the next input-gradient conv; the columns Tin .. ors - 1 are written zero -- that conv runs as a
// same-length conv over the padded rows and reads them as the zeros past the gradient's end
template <bool H>
__global__ __launch_bounds__(256) void wavlm_unstage_rs_kernel(const float* __restrict__ dview, const float* __restrict__ pre, int C,
                                                               int Tin, int prs, int S, int Tp, int ors, void* __restrict__ dx) {
  const int ts = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (ts >= ors) return;
  float v = 0.f;
  if (ts < Tin) {
    const int t = ts / S, p = ts - t * S;
    const float g = t < Tp ? dview[((size_t)b * S * C + (size_t)p * C + c) * Tp + t] : 0.f;
    v = g * gelu_erf_grad(pre[((size_t)b * C + c) * prs + ts]);
  }
  sty_st_any(dx, ((size_t)b * C + c) * ors + ts, v, H);
}
int launch_wavlm_unstage_rs(const float* dview, const float* pre, int B, int C, int Tin, int prs, int S, int Tp, int ors, void* dx,
                            int dx16, hipStream_t st) {
  if (prs < Tin || ors < Tin) {
    set_error("wavlm: un-staged rows of %d frames on row strides of %d and %d", Tin, prs, ors);
    return STY_EINVAL;
  }
  ProfScope prof(dx16 ? "wavlm_unstage_rs_kernel<16>" : "wavlm_unstage_rs_kernel<32>", 0.0, (dx16 ? 10.0 : 12.0) * B * (double)C * Tin, st);
  if (dx16)
    hipLaunchKernelGGL(wavlm_unstage_rs_kernel<true>, dim3(cdiv(ors, 256), C, B), dim3(256), 0, st, dview, pre, C, Tin, prs, S, Tp, ors, dx);
  else
    hipLaunchKernelGGL(wavlm_unstage_rs_kernel<false>, dim3(cdiv(ors, 256), C, B), dim3(256), 0, st, dview, pre, C, Tin, prs, S, Tp, ors, dx);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// GroupNorm(C, C) backward behind layer 0, with layer 1's un-staging and the GELU' between them fused in: per row (b, c) over the T
// frames, z = a x + s, dz = dview[p C + c][t / S] GELU'(z), xhat = (x - mean) rstd;
//   dx = w rstd (dz - mean_t dz - xhat mean_t (dz xhat)).
// Pass 1 leaves the float64 (sum dz, sum dz xhat) of every 1024-frame tile, the finalize adds the tiles in index order (the
// forward's discipline), pass 2 is elementwise.
constexpr int GNB_TILE = 1024;
int wavlm_gn_bwd_ntiles(int T) { return cdiv(T, GNB_TILE); }
namespace {
__device__ __forceinline__ float gn_dz(const float* __restrict__ x, const float* __restrict__ dview, size_t row, int c, int b, int C,
                                       int T, int S, int Tp, int t, float a, float s, float* xv) {
  const float v = x[row * T + t];
  *xv = v;
  const int tv = t / S, p = t - tv * S;
  const float g = tv < Tp ? dview[((size_t)b * S * C + (size_t)p * C + c) * Tp + tv] : 0.f;
  return g * gelu_erf_grad(fmaf(v, a, s));
}
}  // namespace
__global__ __launch_bounds__(256) void wavlm_gn_bwd_part_kernel(const float* __restrict__ x, const float* __restrict__ dview,
                                                                const float* __restrict__ ga, const float* __restrict__ gs,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd, int C,
                                                                int T, int S, int Tp, double* __restrict__ part) {
  __shared__ double red[2][4];
  const int c = blockIdx.y, b = blockIdx.z;
  const size_t row = (size_t)b * C + c;
  const float a = ga[row], s = gs[row], mu = mean[row], rs = rstd[row];
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < GNB_TILE / 256; ++k) {
    const int t = blockIdx.x * GNB_TILE + k * 256 + threadIdx.x;
    if (t < T) {
      float xv;
      const float dz = gn_dz(x, dview, row, c, b, C, T, S, Tp, t, a, s, &xv);
      s1 += (double)dz;
      s2 += (double)dz * (double)((xv - mu) * rs);
    }
  }
  s1 = wave_sum(s1), s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = s1, red[1][threadIdx.x >> 6] = s2;
  __syncthreads();
  if (threadIdx.x < 2)
    part[(row * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
        ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}
__global__ __launch_bounds__(256) void wavlm_gn_bwd_finalize_kernel(const double* __restrict__ part, int ntiles, int BC, int T,
                                                                    float* __restrict__ coef) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= BC) return;
  const double* p = part + (size_t)row * ntiles * 2;
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < ntiles; ++i) {
    s1 += p[2 * i];
    s2 += p[2 * i + 1];
  }
  coef[2 * (size_t)row] = (float)(s1 / T);
  coef[2 * (size_t)row + 1] = (float)(s2 / T);
}
__global__ __launch_bounds__(256) void wavlm_gn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dview,
                                                                 const float* __restrict__ ga, const float* __restrict__ gs,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ coef, int C, int T, int S, int Tp,
                                                                 float* __restrict__ dx) {
  const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (t >= T) return;
  const size_t row = (size_t)b * C + c;
  float xv;
  const float a = ga[row];
  const float dz = gn_dz(x, dview, row, c, b, C, T, S, Tp, t, a, gs[row], &xv);
  const float xh = (xv - mean[row]) * rstd[row];
  dx[row * T + t] = a * ((dz - coef[2 * row]) - xh * coef[2 * row + 1]);  // a = w rstd
}
int launch_wavlm_gn_bwd(const float* x, const float* dview, const float* ga, const float* gs, const float* mean, const float* rstd, int B,
                        int C, int T, int S, int Tp, double* part, float* coef, float* dx, hipStream_t st) {
  const int nt = wavlm_gn_bwd_ntiles(T);
  ProfScope prof("wavlm_gn_bwd_kernels", 0.0, 20.0 * B * (double)C * T, st);
  hipLaunchKernelGGL(wavlm_gn_bwd_part_kernel, dim3(nt, C, B), dim3(256), 0, st, x, dview, ga, gs, mean, rstd, C, T, S, Tp, part);
  hipLaunchKernelGGL(wavlm_gn_bwd_finalize_kernel, dim3(cdiv(B * C, 256)), dim3(256), 0, st, part, nt, B * C, T, coef);
  hipLaunchKernelGGL(wavlm_gn_bwd_apply_kernel, dim3(cdiv(T, 256), C, B), dim3(256), 0, st, x, dview, ga, gs, mean, rstd, coef, C, T, S,
                     Tp, dx);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// layer 0 transposed: d audio[b][n] = sum_c sum_{k = n mod S, + S, ... < K} w[c][k] dy[b][c][(n - k) / S]; one thread per sample,
// the channels in index order; samples no frame reads (the tail) come out zero
__global__ __launch_bounds__(256) void wavlm_conv0_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ w, int N, int C,
                                                              int K, int S, int T, float* __restrict__ dx) {
  const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (n >= N) return;
  const int k0 = n % S;
  float acc = 0.f;
  for (int c = 0; c < C; ++c) {
    const float* dyc = dy + ((size_t)b * C + c) * T;
    const float* wc = w + (size_t)c * K;
    for (int k = k0; k < K && k <= n; k += S) {
      const int t = (n - k) / S;
      if (t < T) acc = fmaf(wc[k], dyc[t], acc);
    }
  }
  dx[(size_t)b * N + n] = acc;
}
int launch_wavlm_conv0_bwd(const float* dy, const float* w, int B, int N, int C, int K, int S, int T, float* dx, hipStream_t st) {
  ProfScope prof("wavlm_conv0_bwd_kernel", 2.0 * K * B * C * T, 4.0 * B * ((double)N + (double)C * T), st);
  hipLaunchKernelGGL(wavlm_conv0_bwd_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, st, dy, w, N, C, K, S, T, dx);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

}  // namespace sty
