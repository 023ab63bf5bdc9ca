// The weight side of a model: pack / input-gradient pack / gradient un-pack kernels (one __device__ body per step, run by a
// single-job kernel and by a table kernel that covers every layer of a model in one launch), the device tables, and the two
// sequences weights_prepare (before a forward) and weights_unpack (after a backward).  See weights.h and DESIGN.md section 4.
#include "model.h"

namespace sty {

// ---------------------------------------------------------------------------------------------
// Weight packing (+ weight_norm): one block per output channel co.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack_conv_body(const ConvPackJob& j, int co) {
  __shared__ float red[256];
  const int n = j.Cin * j.K;
  int cp = co;
  if (j.glu) {
    const int Ch = j.Cout / 2;
    const int half = co >= Ch, c = half ? co - Ch : co;
    cp = (c >> 5) * 64 + half * 32 + (c & 31);
  }
  float scale = 1.f;
  const float* src = j.w;
  if (!src) {
    src = j.v;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float x = src[(size_t)co * n + i];
      s += x * x;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    scale = j.g[co] / sqrtf(red[0]);
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    const int ci = i / j.K, k = i % j.K;
    j.wp[((size_t)k * j.CinP + ci) * j.CoutP + cp] = src[(size_t)co * n + i] * scale;
  }
  if (threadIdx.x == 0 && j.bp) j.bp[cp] = j.bias ? j.bias[co] : 0.f;
}
__global__ __launch_bounds__(256) void pack_conv_kernel(ConvPackJob j) { pack_conv_body(j, blockIdx.x); }
// The same step for MANY convs in one launch (the speech predictor has ~130 dense convs: ~400 launches of 4-5 us each per
// optimizer step when issued one by one).  job_of_block[block] selects the job, block - job.blk0 is the block index inside it.
__global__ __launch_bounds__(256) void pack_conv_multi_kernel(const ConvPackJob* __restrict__ jobs,
                                                              const int* __restrict__ job_of_block) {
  const ConvPackJob j = jobs[job_of_block[blockIdx.x]];
  pack_conv_body(j, blockIdx.x - j.blk0);
}
int launch_pack_conv(const float* w, const float* g, const float* v, const float* bias, int Cout, int Cin, int K,
                     float* wp, float* bp, int CinP, int CoutP, hipStream_t st) {
  ConvPackJob j;
  j.w = w, j.g = g, j.v = v, j.bias = bias, j.wp = wp, j.bp = bp;
  j.Cout = Cout, j.Cin = Cin, j.K = K, j.CinP = CinP, j.CoutP = CoutP;
  hipLaunchKernelGGL(pack_conv_kernel, dim3(Cout), dim3(256), 0, st, j);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
int launch_conv_pack_table(const JobTable<ConvPackJob>& t, hipStream_t st) {
  if (t.blocks.n <= 0) return STY_OK;
  hipLaunchKernelGGL(pack_conv_multi_kernel, dim3(t.blocks.n), dim3(256), 0, st, t.jobs, t.blocks.dev);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------
// Input-gradient weights, element i of wd:
//   1-D:            Wd[k'][co][ci] = Wp[K-1-k'][ci][co]
//   2-D (flat):     Wd[kw'][kh' Cout + co][ci] = Wp[KW-1-kw'][(KH-1-kh') Cin + ci][co]
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack_dgrad_body(const DgradPackJob& j, size_t i) {
  if (j.two_d) {
    const size_t n2 = (size_t)j.K * j.KH * j.Cout * j.Cin;
    if (i >= n2) return;
    const int ci = (int)(i % j.Cin);
    const int co = (int)((i / j.Cin) % j.Cout);
    const int kh = (int)((i / ((size_t)j.Cin * j.Cout)) % j.KH);
    const int kw = (int)(i / ((size_t)j.Cin * j.Cout * j.KH));
    j.wd[((size_t)kw * j.CinPd + kh * j.Cout + co) * j.CoutPd + ci] =
        j.wp[((size_t)(j.K - 1 - kw) * j.CinP + (j.KH - 1 - kh) * j.Cin + ci) * j.CoutP + co];
    return;
  }
  const size_t n = (size_t)j.K * j.CinP * j.CoutP;
  if (i >= n) return;
  const int ci = (int)(i % j.CinP);
  const int co = (int)((i / j.CinP) % j.CoutP);
  const int kd = (int)(i / ((size_t)j.CinP * j.CoutP));
  j.wd[i] = j.wp[((size_t)(j.K - 1 - kd) * j.CinP + ci) * j.CoutP + co];
}
__global__ __launch_bounds__(256) void pack_dgrad_kernel(DgradPackJob j) {
  pack_dgrad_body(j, (size_t)blockIdx.x * 256 + threadIdx.x);
}
__global__ __launch_bounds__(256) void pack_dgrad_multi_kernel(const DgradPackJob* __restrict__ jobs,
                                                               const int* __restrict__ job_of_block) {
  const DgradPackJob j = jobs[job_of_block[blockIdx.x]];
  pack_dgrad_body(j, (size_t)(blockIdx.x - j.blk0) * 256 + threadIdx.x);
}
static DgradPackJob dgrad_job(const float* wp, int K, int CinP, int CoutP, float* wd) {
  DgradPackJob j;
  j.wp = wp, j.wd = wd, j.K = K, j.CinP = CinP, j.CoutP = CoutP;
  return j;
}
static DgradPackJob dgrad2d_job(const float* wp, int KW, int KH, int Cin, int Cout, int CinP, int CoutP, int CinPd, int CoutPd,
                                float* wd) {
  DgradPackJob j = dgrad_job(wp, KW, CinP, CoutP, wd);
  j.two_d = 1, j.KH = KH, j.Cin = Cin, j.Cout = Cout, j.CinPd = CinPd, j.CoutPd = CoutPd;
  return j;
}
static int dgrad_job_blocks(const DgradPackJob& j) {
  const size_t n = j.two_d ? (size_t)j.K * j.KH * j.Cout * j.Cin : (size_t)j.K * j.CinP * j.CoutP;
  return (int)((n + 255) / 256);
}
static int launch_pack_dgrad_job(const DgradPackJob& j, hipStream_t st) {
  hipLaunchKernelGGL(pack_dgrad_kernel, dim3(dgrad_job_blocks(j)), dim3(256), 0, st, j);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
int launch_pack_dgrad(const float* wp, int K, int CinP, int CoutP, float* wd, hipStream_t st) {
  return launch_pack_dgrad_job(dgrad_job(wp, K, CinP, CoutP, wd), st);
}
// (one layer: the spectrogram discriminators, disc.hip; a model's layers go through the table)
int launch_pack_dgrad2d(const float* wp, int KW, int KH, int Cin, int Cout, int CinP, int CoutP, int CinPd, int CoutPd,
                        float* wd, hipStream_t st) {
  return launch_pack_dgrad_job(dgrad2d_job(wp, KW, KH, Cin, Cout, CinP, CoutP, CinPd, CoutPd, wd), st);
}
int launch_dgrad_pack_table(const JobTable<DgradPackJob>& t, hipStream_t st) {
  if (t.blocks.n <= 0) return STY_OK;
  hipLaunchKernelGGL(pack_dgrad_multi_kernel, dim3(t.blocks.n), dim3(256), 0, st, t.jobs, t.blocks.dev);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------
// Split-mode fragments of a packed 32 x 32 conv (conv32p.hip, conv32p_split_kernel): every weight as three bf16 pieces
// h = bf16(w), m = bf16(w - h), l = bf16(w - h - m), each piece in the lane order of v_mfma_f32_32x32x16_bf16's A operand: lane
// (co = l31, k-block = hi) of k-step s holds the input channels 16 s + 8 hi .. + 7.  One block per tap, one thread per
// (k-step, lane).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack_split3_body(const SplitPackJob& j, int k) {
  const int s = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const int co = ln & 31, ci0 = 16 * s + 8 * (ln >> 5);
  float h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float w = j.wp[((size_t)k * 32 + ci0 + e) * 32 + co];
    h[e] = sty_round_bf16(w);
    m[e] = sty_round_bf16(w - h[e]);
    l[e] = (w - h[e]) - m[e];
  }
  bf16x8* out = static_cast<bf16x8*>(j.w3) + ((size_t)(k * 2 + s) * 3) * 64 + ln;
  out[0] = sty_pack_bf16(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
  out[64] = sty_pack_bf16(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]);
  out[128] = sty_pack_bf16(l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7]);
}
__global__ __launch_bounds__(128) void pack_split3_kernel(SplitPackJob j) { pack_split3_body(j, blockIdx.x); }
__global__ __launch_bounds__(128) void pack_split3_multi_kernel(const SplitPackJob* __restrict__ jobs,
                                                                const int* __restrict__ job_of_block) {
  const SplitPackJob j = jobs[job_of_block[blockIdx.x]];
  pack_split3_body(j, blockIdx.x - j.blk0);
}
int launch_pack_split3(const float* wp, int K, void* w3, hipStream_t st) {
  SplitPackJob j;
  j.wp = wp, j.w3 = w3, j.K = K;
  hipLaunchKernelGGL(pack_split3_kernel, dim3(K), dim3(128), 0, st, j);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
int launch_split3_pack_table(const JobTable<SplitPackJob>& t, hipStream_t st) {
  if (t.blocks.n <= 0) return STY_OK;
  hipLaunchKernelGGL(pack_split3_multi_kernel, dim3(t.blocks.n), dim3(128), 0, st, t.jobs, t.blocks.dev);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------
// Packed gradient -> parameter gradients (+=); one block per output channel co.
//   plain:        dW[co][ci][k] += gwp[k][ci][co]
//   weight_norm:  w = g v/|v|:  dg[co] += <gw, v>/|v|,  dv += g/|v| (gw - v <gw, v>/|v|^2)
//   bias:         db[co] += gbp[co]
// (GLU-ordered packs have no un-pack: the training graph runs on their plain-ordered copies.)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void unpack_grad_body(const GradUnpackJob& j, int co) {
  __shared__ float r1[256], r2[256];
  const int n = j.Cin * j.K;
  const int cp = co;
  if (threadIdx.x == 0 && j.db && j.gbp) j.db[co] += j.gbp[cp];
  if (!j.v) {
    if (!j.dW) return;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int ci = i / j.K, k = i % j.K;
      j.dW[(size_t)co * n + i] += j.gwp[((size_t)k * j.CinP + ci) * j.CoutP + cp];
    }
    return;
  }
  if (!j.dg || !j.dv) return;
  float dot = 0.f, nn = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int ci = i / j.K, k = i % j.K;
    const float v = j.v[(size_t)co * n + i];
    dot = fmaf(j.gwp[((size_t)k * j.CinP + ci) * j.CoutP + cp], v, dot);
    nn = fmaf(v, v, nn);
  }
  r1[threadIdx.x] = dot;
  r2[threadIdx.x] = nn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      r1[threadIdx.x] += r1[threadIdx.x + o];
      r2[threadIdx.x] += r2[threadIdx.x + o];
    }
    __syncthreads();
  }
  const float norm = sqrtf(r2[0]), d = r1[0], gg = j.g[co];
  if (threadIdx.x == 0) j.dg[co] += d / norm;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int ci = i / j.K, k = i % j.K;
    const float v = j.v[(size_t)co * n + i];
    j.dv[(size_t)co * n + i] += gg / norm * (j.gwp[((size_t)k * j.CinP + ci) * j.CoutP + cp] - v * d / (norm * norm));
  }
}
__global__ __launch_bounds__(256) void unpack_grad_kernel(GradUnpackJob j) { unpack_grad_body(j, blockIdx.x); }
__global__ __launch_bounds__(256) void unpack_grad_multi_kernel(const GradUnpackJob* __restrict__ jobs,
                                                                const int* __restrict__ job_of_block, int blk_base) {
  const int blk = (int)blockIdx.x + blk_base;  // a launch may cover a sub-range of the table (one gradient segment)
  const GradUnpackJob j = jobs[job_of_block[blk]];
  unpack_grad_body(j, blk - j.blk0);
}
int launch_unpack_grad(const float* gwp, const float* g, const float* v, int Cout, int Cin, int K, int CinP, int CoutP,
                       float* dW, float* dg, float* dv, hipStream_t st) {
  GradUnpackJob j;
  j.gwp = gwp, j.g = g, j.v = v, j.dW = dW, j.dg = dg, j.dv = dv;
  j.Cout = Cout, j.Cin = Cin, j.K = K, j.CinP = CinP, j.CoutP = CoutP;
  hipLaunchKernelGGL(unpack_grad_kernel, dim3(Cout), dim3(256), 0, st, j);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
int launch_grad_unpack_table(const JobTable<GradUnpackJob>& t, int blk_base, int nblocks, hipStream_t st) {
  if (nblocks <= 0) return STY_OK;
  hipLaunchKernelGGL(unpack_grad_multi_kernel, dim3(nblocks), dim3(256), 0, st, t.jobs, t.blocks.dev, blk_base);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------
// spectral norm (fixed u, v within a step): W_eff = W / sigma, sigma = u^T W v
//   dW[co][i] += G[co][i]/sigma - (<G, W>/sigma^2) u[co] v[i],   G taken from the packed gradient.
// t[co] = u[co] <W[co,:], v> (sn_rowdot_multi_kernel) gives sigma = sum t.  Two steps: <G,W> per row, then apply -- for EVERY
// spectral-norm conv of a model in two launches (one block per output row of every layer;
// the style encoder has 13 such layers, and its un-pack is the last thing of the c3 step: 40 serial launches before).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_gw_rowdot_multi_kernel(const SnUnpackJob* __restrict__ jobs,
                                                                 const int* __restrict__ job_of_block) {
  __shared__ float red[256];
  const SnUnpackJob j = jobs[job_of_block[blockIdx.x]];
  const int co = (int)blockIdx.x - j.blk0;
  const int KW = j.K, KH = j.KH, n = j.Cin * KH * KW;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int kw = i % KW, kh = (i / KW) % KH, ci = i / (KW * KH);
    s = fmaf(j.gwp[((size_t)kw * j.CinP + kh * j.Cin + ci) * j.CoutP + co], j.w[(size_t)co * n + i], s);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) j.gw_rows[co] = red[0];
}
__global__ __launch_bounds__(256) void sn_unpack_multi_kernel(const SnUnpackJob* __restrict__ jobs,
                                                              const int* __restrict__ job_of_block) {
  __shared__ float sig, dot;
  const SnUnpackJob j = jobs[job_of_block[blockIdx.x]];
  const int co = (int)blockIdx.x - j.blk0;
  if (threadIdx.x == 0) {
    float s = 0.f, d = 0.f;
    for (int i = 0; i < j.Cout; ++i) {
      s += j.t[i];
      d += j.gw_rows[i];
    }
    sig = s;
    dot = d;
    if (j.db && j.gbp) j.db[co] += j.gbp[co];
  }
  __syncthreads();
  if (!j.dW) return;
  const int KW = j.K, KH = j.KH, n = j.Cin * KH * KW;
  const float inv = 1.0f / sig, k = dot * inv * inv;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int kw = i % KW, kh = (i / KW) % KH, ci = i / (KW * KH);
    j.dW[(size_t)co * n + i] += j.gwp[((size_t)kw * j.CinP + kh * j.Cin + ci) * j.CoutP + co] * inv - k * j.u[co] * j.v[i];
  }
}
int launch_sn_unpack_table(const JobTable<SnUnpackJob>& t, hipStream_t st) {
  if (t.blocks.n <= 0) return STY_OK;
  hipLaunchKernelGGL(sn_gw_rowdot_multi_kernel, dim3(t.blocks.n), dim3(256), 0, st, t.jobs, t.blocks.dev);
  hipLaunchKernelGGL(sn_unpack_multi_kernel, dim3(t.blocks.n), dim3(256), 0, st, t.jobs, t.blocks.dev);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ConvNeXt pwconv2 bias folding b2eff = b2 + W2 . beta (convnext.hip): g = d loss / d b2eff [C]
// grid: x = 64-channel slice of the 4C axis (dbeta, one wave-quarter of the co loop each, summed through LDS),
// plus C*4C/256 blocks for the rank-1 dW2 update
__global__ __launch_bounds__(256) void b2eff_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w2,
                                                        const float* __restrict__ beta, int C, int nbeta_blocks,
                                                        float* __restrict__ db2, float* __restrict__ dbeta,
                                                        float* __restrict__ dW2) {
  __shared__ float red[4][64];
  const int C4 = 4 * C;
  if ((int)blockIdx.x < nbeta_blocks) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ch = blockIdx.x * 64 + lane;
    float acc = 0.f;
    if (ch < C4)
      for (int co = wave; co < C; co += 4) acc = fmaf(w2[(size_t)co * C4 + ch], g[co], acc);
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && ch < C4 && dbeta) dbeta[ch] += red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
    if (blockIdx.x == 0 && db2)
      for (int i = threadIdx.x; i < C; i += 256) db2[i] += g[i];
    return;
  }
  const int i = (blockIdx.x - nbeta_blocks) * 256 + threadIdx.x;
  if (i < C * C4 && dW2) {
    const int co = i / C4, ch = i % C4;
    dW2[i] += g[co] * beta[ch];
  }
}
int launch_b2eff_bwd(const float* g, const float* w2, const float* beta, int C, float* db2, float* dbeta, float* dW2,
                     hipStream_t st) {
  const int nb = cdiv(4 * C, 64);
  hipLaunchKernelGGL(b2eff_bwd_kernel, dim3(nb + cdiv(4 * C * C, 256)), dim3(256), 0, st, g, w2, beta, C, nb, db2, dbeta,
                     dW2);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---------------------------------------------------------------------------------------------
// The device tables of a model, from its PackJob list.
// Gradient segments: the pack jobs [0, seg_job_split) belong to the module whose backward runs LAST; their un-pack jobs are
// the first of the `unpack` table, so that table splits at the block where job seg_job_split begins (seg_blk_split; the whole
// table when there is no such job).  No other table is split: packs run for the whole model, and no model has a
// spectral-norm layer in segment 1.
// ---------------------------------------------------------------------------------------------
namespace {
template <typename Job>
struct HostTable {
  std::vector<Job> jobs;
  std::vector<int> job_of_block;
  void add(Job j, int nblocks) {
    j.blk0 = (int)job_of_block.size();
    job_of_block.insert(job_of_block.end(), nblocks, (int)jobs.size());
    jobs.push_back(j);
  }
};
}  // namespace

int weights_build_tables(sty_model* m) {
  HostTable<ConvPackJob> pack;
  HostTable<DgradPackJob> dgrad;
  HostTable<SplitPackJob> split3;
  HostTable<GradUnpackJob> unpack;
  HostTable<SnPrepJob> sn_prep;
  HostTable<SnUnpackJob> sn_unpack;
  std::vector<int> sn_wtu;
  auto PG = [&](const float* p) -> float* {
    auto it = p ? m->pgrad.find(p) : m->pgrad.end();
    return it == m->pgrad.end() ? nullptr : it->second;
  };
  auto GA = [&](const float* packed) -> float* {
    return (packed && m->garena) ? reinterpret_cast<float*>(m->garena + (reinterpret_cast<const char*>(packed) - m->arena))
                                 : nullptr;
  };
  WeightTables& wt = m->wt;
  size_t job_index = 0;
  int split = -1;
  for (const PackJob& j : m->jobs) {
    if (job_index++ == m->seg_job_split) split = (int)unpack.job_of_block.size();
    const bool has_bias = j.bias && j.bp;
    if (j.kind == PK_CONV || j.kind == PK_CONV_WN || j.kind == PK_CONV_GLU) {
      ConvPackJob a;
      a.w = j.w, a.g = j.g, a.v = j.v, a.bias = j.bias, a.wp = j.wp, a.bp = j.bp;
      a.Cout = j.Cout, a.Cin = j.Cin, a.K = j.K, a.CinP = j.CinP, a.CoutP = j.CoutP;
      a.glu = j.kind == PK_CONV_GLU;
      pack.add(a, j.Cout);
      if (m->garena && j.kind != PK_CONV_GLU) {  // GLU-ordered packs are not used by the training graph
        const bool wn = j.kind == PK_CONV_WN;
        GradUnpackJob u;
        u.gwp = GA(j.wp), u.g = j.g, u.v = wn ? j.v : nullptr, u.gbp = has_bias ? GA(j.bp) : nullptr;
        u.dW = wn ? nullptr : PG(j.w), u.dg = wn ? PG(j.g) : nullptr, u.dv = wn ? PG(j.v) : nullptr;
        u.db = has_bias ? PG(j.bias) : nullptr;
        u.Cout = j.Cout, u.Cin = j.Cin, u.K = j.K, u.CinP = j.CinP, u.CoutP = j.CoutP;
        if (u.dW || (u.dg && u.dv) || u.db) unpack.add(u, j.Cout);
      }
    } else if (j.kind == PK_DGRAD) {
      const DgradPackJob a = dgrad_job(j.w, j.K, j.CinP, j.CoutP, j.wp);
      dgrad.add(a, dgrad_job_blocks(a));
    } else if (j.kind == PK_SPLIT3) {  // (source: the conv pack, launched before this table)
      SplitPackJob a;
      a.wp = j.w, a.w3 = j.wp, a.K = j.K;
      split3.add(a, j.K);
    } else if (j.kind == PK_DGRAD2D) {  // (source: the spectral-norm pack, launched before this table)
      const DgradPackJob a = dgrad2d_job(j.w, j.K, j.KH, j.Cin, j.Cout, j.CinP, j.CoutP,
                                         (int)align_up(j.KH * j.Cout, CI_CHUNK), (int)align_up(j.Cin, 32), j.wp);
      dgrad.add(a, dgrad_job_blocks(a));
    } else if (j.kind == PK_CONV2D_SN || j.kind == PK_DW2D_SN) {
      SnPrepJob a;
      a.w = j.w, a.bias = j.bias, a.u = const_cast<float*>(j.g), a.v = const_cast<float*>(j.v);  // bound buffers, not parameters
      a.t = j.scratch, a.power = j.scratch2, a.wp = j.wp, a.bp = j.kind == PK_CONV2D_SN ? j.bp : nullptr;
      a.Cout = j.Cout, a.Cin = j.Cin, a.K = j.K, a.KH = j.KH, a.CinP = j.CinP, a.CoutP = j.CoutP;
      a.depthwise = j.kind == PK_DW2D_SN;
      a.wtu0 = (int)sn_wtu.size();
      sn_wtu.insert(sn_wtu.end(), sn_wtu_blocks(a.depthwise ? 9 : j.Cin * j.KH * j.K), (int)sn_prep.jobs.size());
      sn_prep.add(a, j.Cout);
      if (j.kind == PK_CONV2D_SN && m->garena) {
        SnUnpackJob u;
        u.gwp = GA(j.wp), u.w = j.w, u.u = j.g, u.v = j.v, u.t = j.scratch, u.gbp = has_bias ? GA(j.bp) : nullptr;
        u.dW = PG(j.w), u.db = has_bias ? PG(j.bias) : nullptr;
        u.gw_rows = GA(j.scratch);  // the gradient-arena twin of the sigma scratch holds the <G, W> row sums
        u.Cout = j.Cout, u.Cin = j.Cin, u.K = j.K, u.KH = j.KH, u.CinP = j.CinP, u.CoutP = j.CoutP;
        if (u.dW || u.db) sn_unpack.add(u, j.Cout);
      }
    }
  }
  wt.seg_blk_split = split >= 0 ? split : (int)unpack.job_of_block.size();
  int rc;
  if ((rc = wt.pack.upload(pack.jobs, pack.job_of_block))) return rc;
  if ((rc = wt.dgrad.upload(dgrad.jobs, dgrad.job_of_block))) return rc;
  if ((rc = wt.split3.upload(split3.jobs, split3.job_of_block))) return rc;
  if ((rc = wt.unpack.upload(unpack.jobs, unpack.job_of_block))) return rc;
  if ((rc = wt.sn_prep.upload(sn_prep.jobs, sn_prep.job_of_block))) return rc;
  if ((rc = wt.sn_wtu.upload(sn_wtu))) return rc;
  if ((rc = wt.sn_unpack.upload(sn_unpack.jobs, sn_unpack.job_of_block))) return rc;
  wt.ready = true;
  return STY_OK;
}
static int tables_ready(sty_model* m) { return m->wt.ready ? STY_OK : weights_build_tables(m); }

int weights_sn_power_iter(sty_model* m, hipStream_t st) {
  int r = tables_ready(m);
  if (r != STY_OK) return r;
  return launch_sn_prep_table(m->wt.sn_prep, m->wt.sn_wtu, true, false, st);  // every layer in four launches
}

// ---- WavLM (kind "wavlm", frozen: nothing to un-pack) ----
// nrm[k] = || v[:, :, k] || over the n = Cout Cin rows of v [n][K] (weight-norm dim = 2 of the positional conv): one workgroup
// per tap, float64 partials added in a fixed order
__global__ __launch_bounds__(256) void wavlm_tap_norm_kernel(const float* __restrict__ v, int n, int K, float* __restrict__ nrm) {
  __shared__ double red[256];
  const int k = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double x = (double)v[(size_t)i * K + k];
    acc += x * x;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) nrm[k] = (float)sqrt(red[0]);
}
// one workgroup per output channel of the job (WavlmPackJob, model.h)
__global__ __launch_bounds__(256) void wavlm_pack_kernel(WavlmPackJob j) {
  const int co = blockIdx.x, n = j.Cin * j.K;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int ci = i / j.K, kk = i - ci * j.K;
    const int kp = kk / j.s, p = kk - kp * j.s;
    float v = j.w[(size_t)(j.co0 + co) * n + i];
    if (j.g) v *= j.g[kk] / j.nrm[kk];
    j.wp[((size_t)kp * j.CinP + (size_t)p * j.Cin + ci) * j.CoutP + co] = v;
  }
  if (threadIdx.x == 0 && j.bp) j.bp[co] = j.bias ? j.bias[j.co0 + co] : 0.f;
}
int launch_wavlm_pack(const WavlmPackJob& j, hipStream_t st) {
  hipLaunchKernelGGL(wavlm_pack_kernel, dim3(j.Cout), dim3(256), 0, st, j);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
int wavlm_prepare(const WavlmPlan& p, hipStream_t st) {
  if (p.pos_nrm)
    hipLaunchKernelGGL(wavlm_tap_norm_kernel, dim3(p.pos_k), dim3(256), 0, st, p.pos_v, p.hidden * (p.hidden / p.pos_groups), p.pos_k,
                       p.pos_nrm);
  for (const WavlmPackJob& j : p.packs) hipLaunchKernelGGL(wavlm_pack_kernel, dim3(j.Cout), dim3(256), 0, st, j);
  STY_LAUNCH_CHECK();
  // the input-gradient weights of these packs (taps flipped, channels transposed), once per model: the backward to the wave
  int r;
  for (int i = 1; i < p.n_conv; ++i)
    if (p.conv_d[i].wp &&
        (r = launch_pack_dgrad(p.conv[i].wp, p.conv[i].K, p.conv[i].CinP, p.conv[i].CoutP, const_cast<float*>(p.conv_d[i].wp), st)) != STY_OK)
      return r;
  for (size_t g = 0; g < p.pos_d.size(); ++g)
    if ((r = launch_pack_dgrad(p.pos[g].wp, p.pos[g].K, p.pos[g].CinP, p.pos[g].CoutP, const_cast<float*>(p.pos_d[g].wp), st)) != STY_OK)
      return r;
  return STY_OK;
}

int weights_prepare(sty_model* m, hipStream_t st) {
  int r = tables_ready(m);
  if (r != STY_OK) return r;
  // every plain / weight-norm / GLU conv pack in one launch
  if ((r = launch_conv_pack_table(m->wt.pack, st)) != STY_OK) return r;
  {  // the pwconv2 fragment packs of the fused ConvNeXt blocks: one launch per W2A_MAXJ blocks (every other kind is batched
     // through the device-side job tables above / below)
    W2aJobs wj;
    for (const PackJob& j : m->jobs) {
      if (j.kind != PK_W2A) continue;
      const int k = wj.n++;
      wj.w2[k] = j.w;
      wj.b2[k] = j.bias;
      wj.gb[k] = j.extra;
      wj.w2a[k] = j.wp;
      wj.b2eff[k] = j.bp;
      wj.C[k] = j.Cout;
      if (wj.n == W2A_MAXJ) {
        if ((r = launch_pack_w2a_multi(wj, st)) != STY_OK) return r;
        wj.n = 0;
      }
    }
    if ((r = launch_pack_w2a_multi(wj, st)) != STY_OK) return r;
  }
  // sigma and W / sigma of every spectral-norm layer: two launches.  Before the input-gradient table: the 2-D input-gradient
  // weights are made from these packed weights.
  if ((r = launch_sn_prep_table(m->wt.sn_prep, m->wt.sn_wtu, false, true, st)) != STY_OK) return r;
  if ((r = launch_dgrad_pack_table(m->wt.dgrad, st)) != STY_OK) return r;
  if ((r = launch_split3_pack_table(m->wt.split3, st)) != STY_OK) return r;  // (the split mode's fragments, from the conv packs)
  if (m->kind == "speech_predictor") {
    const DecoderPlan& d = m->dec;
    if ((r = launch_prep_fnv(d.f0_g, d.f0_v, d.f0_b, d.n_g, d.n_v, d.n_b, d.v_g, d.v_v, d.v_b, d.fnv_w, st)) != STY_OK) return r;
  }
  if (m->kind == "text_aligner" || m->kind == "text_aligner_train") {
    // BatchNorm1d(affine=False) on running statistics -> one scale / shift pair per layer
    const AlignerPlan& a = m->ali;
    for (int i = 0; i < 3; ++i)
      if ((r = launch_aligner_bn_prep(a.rm[i], a.rv[i], a.hidden, 1e-5f, a.bn_scale[i], a.bn_shift[i], st)) != STY_OK) return r;
    // (bn_zero is the arena's zero fill)
    if (a.bn_one && (r = launch_fill_f32(a.bn_one, a.hidden, 1.0f, st)) != STY_OK) return r;
  }
  // RMVPE: the BatchNorm-folding packs, W_hh^T and the input BatchNorm's scale / shift (rmvpe.hip)
  if (m->kind == "rmvpe" && (r = rmvpe_prepare(m->rmv, st)) != STY_OK) return r;
  // WavLM: the strided feature convs packed for their s-frames-at-a-time view, the positional conv's weight norm folded per group
  if (m->kind == "wavlm" && (r = wavlm_prepare(m->wav, st)) != STY_OK) return r;
  // the bf16 fragment buffers the persistent kernels read the packed weights through (bf16 mode)
  if (m->arena && (r = convp16_repack_range(m->arena, m->arena + m->arena_bytes, st)) != STY_OK) return r;
  return STY_OK;
}

int weights_unpack(sty_model* m, hipStream_t st, int seg) {
  auto PG = [&](const float* p) -> float* {
    auto it = m->pgrad.find(p);
    return it == m->pgrad.end() ? nullptr : it->second;
  };
  auto GA = [&](const float* packed) -> float* {
    return reinterpret_cast<float*>(m->garena + (reinterpret_cast<const char*>(packed) - m->arena));
  };
  int r = tables_ready(m);
  if (r != STY_OK) return r;
  {  // every plain / weight-norm conv (weights and biases) of the segment in one launch
    const int b0 = seg == 0 ? m->wt.seg_blk_split : 0;
    const int b1 = seg == 1 ? m->wt.seg_blk_split : m->wt.unpack.blocks.n;
    if ((r = launch_grad_unpack_table(m->wt.unpack, b0, b1 - b0, st)) != STY_OK) return r;
  }
  size_t job_index = 0;
  for (const PackJob& j : m->jobs) {  // the kinds without a table
    const bool in_seg1 = job_index++ < m->seg_job_split;
    if ((seg == 0 && in_seg1) || (seg == 1 && !in_seg1)) continue;
    if (j.kind == PK_DW2D_SN) {
      float* dW = PG(j.w);
      if (dW && (r = launch_dw2d_sn_unpack(GA(j.wp), j.w, j.g, j.v, j.scratch, j.Cout, dW, st))) return r;
    } else if (j.kind == PK_W2A) {
      // b2eff = b2 + W2 . grn_beta:  db2 += g, dbeta += W2^T g, dW2 += g beta^T   (g = gradient of b2eff)
      if ((r = launch_b2eff_bwd(GA(j.bp), j.w, j.extra, j.Cout, PG(j.bias), PG(j.extra), PG(j.w), st))) return r;
    }
  }
  // every spectral-norm conv (weights and biases) in two launches; no model has them in segment 1
  if (seg != 1 && (r = launch_sn_unpack_table(m->wt.sn_unpack, st)) != STY_OK) return r;
  if (m->kind == "speech_predictor" && m->dec.fnv_w && seg != 1) {
    const DecoderPlan& d = m->dec;
    r = launch_fnv_unpack(GA(d.fnv_w), d.f0_g, d.f0_v, d.n_g, d.n_v, d.v_g, d.v_v, PG(d.f0_g), PG(d.f0_v), PG(d.f0_b),
                          PG(d.n_g), PG(d.n_v), PG(d.n_b), PG(d.v_g), PG(d.v_v), PG(d.v_b), st);
    if (r) return r;
  }
  return STY_OK;
}

}  // namespace sty
