// CTC loss with its gradient on the device (train/losses.py:478-653 CTCLossWithLabelPriors, which asks k2.ctc_loss for it on
// the CPU).  Exact CTC, the semantics of torch.nn.functional.ctc_loss(reduction="mean", zero_infinity=False): every valid
// path counts.  k2 prunes its lattice with output_beam = 10; that pruning is not reproduced.
//
// One workgroup per utterance, lane = state, as forced_align_kernel (align.hip): S = 2 U_b + 1 states "blank, tok, blank,
// ..., blank", the frame's log-prob row staged in LDS and double-buffered through registers, one barrier per frame.
// The recurrences run in float64 log-space (the reference passes use_double_scores=True): at T = 1030 and nll = 6e3 one
// fp32 ulp of alpha is 5e-4 nats, and alpha + beta - nll goes straight into the occupancies.
//   forward   alpha[t][s] = lse(alpha[t-1][s], alpha[t-1][s-1], skip(s) ? alpha[t-1][s-2]) + e[t][cls s], every frame's row
//             stored to the workspace [B][T][2 U + 1] double; nll = -lse(alpha[T_b-1][S-1], alpha[T_b-1][S-2])
//   backward  beta[t][s]  = lse(beta[t+1][s], beta[t+1][s+1], skip(s+2) ? beta[t+1][s+2]) + e[t][cls s] in two LDS rows;
//             occ_t[v] = sum over the states of class v of exp(alpha + beta - e + nll)
// with e[t][v] = lp[t][v] - prior_scale * log_priors[v] (the priors are constants).  Several states share a class (every
// blank state, every repeated token), so the occupancies are summed with LDS atomics -- on 64-bit FIXED-POINT cells
// (2^-44 steps): integer adds commute, so a row's result does not depend on the order the waves arrive in, nor on the batch
// the row is in.  The cells are one tile [V1][TT + 1] of TT frames; when the sweep leaves a tile, it is turned into
//   d_logits[b][v][t] = weight / (B max(U_b, 1)) * (exp(lp[b][t][v]) - occ_t[v])
// (the log-softmax backward folded in: sum_v occ_t = 1) and written channel-major with t fastest, the layout the output
// Linear's GEMM wrote the logits in.  Frames at or beyond a row's length get zeros.
// Every index is derived from values the kernel has range-checked: a row whose lengths or targets are out of range gets
// status 2, a row without a valid path status 1; both get nll = +inf, a zero gradient and touch nothing else.
#include "sty_common.h"

namespace sty {

constexpr int CTC_THREADS = 256;
constexpr int CTC_MAX_U = 512;  // as sty_forced_align
constexpr int CTC_MAX_S = 2 * CTC_MAX_U + 1;
constexpr int CTC_ROW_REGS = 4;  // the next frame's row in registers: V1 <= CTC_ROW_REGS * CTC_THREADS
constexpr int CTC_SKIP = 1 << 30;  // cls[] flag: the state may be entered from s - 2
constexpr double CTC_FIX = 17592186044416.0;  // 2^44: one occupancy (<= 1) in fixed point
constexpr size_t CTC_LDS_STATIC = 2 * (CTC_MAX_S + 4) * sizeof(double) + CTC_MAX_S * sizeof(int) + 64;
constexpr size_t CTC_LDS_MAX = 64 * 1024;

__device__ __forceinline__ double ctc_lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

static inline size_t ctc_dyn_lds(int V1, int TT) {  // pri double [V1], tile u64 [V1][TT + 1], rows float [2][V1]
  return (size_t)V1 * 8 + (size_t)V1 * (TT + 1) * 8 + (size_t)2 * V1 * 4;
}

__global__ __launch_bounds__(CTC_THREADS) void ctc_loss_kernel(int B, int T, int V1, int U, const float* __restrict__ lp,
                                                               const float* __restrict__ log_priors, float prior_scale,
                                                               const int64_t* __restrict__ targets,
                                                               const int64_t* __restrict__ in_len,
                                                               const int64_t* __restrict__ tg_len, int blank, float weight,
                                                               double* __restrict__ nll, int32_t* __restrict__ status,
                                                               float* __restrict__ d_logits, double* __restrict__ alpha_ws,
                                                               int TT) {
  extern __shared__ double ctc_dyn[];
  double* pri = ctc_dyn;                                                                     // [V1]
  unsigned long long* tile = reinterpret_cast<unsigned long long*>(ctc_dyn + V1);            // [V1][TT + 1]
  float* rows = reinterpret_cast<float*>(tile + (size_t)V1 * (TT + 1));                      // [2][V1]
  __shared__ double ab[2][CTC_MAX_S + 4];  // state s at [s + 2]: two -inf cells on either side stand in for s - 2 .. s + 2
  __shared__ int cls[CTC_MAX_S];
  __shared__ int s_bad, s_rep;
  __shared__ double s_ll;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t Tb64 = in_len[b], Ub64 = tg_len[b];
  const float* lpb = lp + (size_t)b * T * V1;
  float* dl = d_logits ? d_logits + (size_t)b * V1 * T : nullptr;
  const bool bad_len = Tb64 < 0 || Tb64 > T || Ub64 < 0 || Ub64 > U;  // (uniform)
  const int Tb = bad_len ? 0 : (int)Tb64, Ub = bad_len ? 0 : (int)Ub64;
  const int S = 2 * Ub + 1, Sg = 2 * U + 1;
  if (tid == 0) {
    s_bad = bad_len ? 1 : 0;
    s_rep = 0;
  }
  __syncthreads();
  for (int s = tid; s < S; s += CTC_THREADS) {
    int c = blank;
    if (s & 1) {
      const int i = s >> 1;
      const int64_t tk = targets[(size_t)b * U + i];
      if (tk < 0 || tk >= V1 || tk == blank) {
        atomicOr(&s_bad, 1);
      } else {
        c = (int)tk;
        if (i > 0) {
          if (targets[(size_t)b * U + i - 1] == tk)
            atomicAdd(&s_rep, 1);
          else
            c |= CTC_SKIP;
        }
      }
    }
    cls[s] = c;
  }
  __syncthreads();
  int st_code = s_bad ? 2 : (Tb < Ub + s_rep ? 1 : 0);
  double ll = 0.0;  // log p(target | input); an empty input with an empty target has the one empty path
  if (st_code == 0 && Tb > 0) {
    // ---- forward sweep ----
    for (int v = tid; v < V1; v += CTC_THREADS) {
      pri[v] = log_priors ? (double)prior_scale * (double)log_priors[v] : 0.0;
      rows[v] = lpb[v];
    }
    for (int s = tid; s < 2 * (CTC_MAX_S + 4); s += CTC_THREADS) (&ab[0][0])[s] = -INFINITY;
    __syncthreads();
    if (tid < 2 && tid < S) {
      const int c = cls[tid] & ~CTC_SKIP;
      ab[0][tid + 2] = (double)rows[c] - pri[c];
    }
    if (Tb > 1)
      for (int v = tid; v < V1; v += CTC_THREADS) rows[V1 + v] = lpb[(size_t)V1 + v];
    __syncthreads();
    double* aw = dl ? alpha_ws + (size_t)b * T * Sg : nullptr;
    if (aw)
      for (int s = tid; s < S; s += CTC_THREADS) aw[s] = ab[0][s + 2];
    for (int t = 1; t < Tb; ++t) {
      const int cur = t & 1;
      const float* rw = rows + cur * V1;
      float* rnext = rows + (cur ^ 1) * V1;
      const double* ap = ab[cur ^ 1];
      double* ac = ab[cur];
      float nx[CTC_ROW_REGS];
      const bool more = t + 1 < Tb;
      if (more) {
        const float* src = lpb + (size_t)(t + 1) * V1;
#pragma unroll
        for (int k = 0; k < CTC_ROW_REGS; ++k) {
          const int v = tid + k * CTC_THREADS;
          nx[k] = v < V1 ? src[v] : 0.f;
        }
      }
      for (int s = tid; s < S; s += CTC_THREADS) {
        const int cl = cls[s], c = cl & ~CTC_SKIP;
        const double x2 = (cl & CTC_SKIP) ? ap[s] : -INFINITY;
        const double a = ctc_lse3(ap[s + 2], ap[s + 1], x2) + ((double)rw[c] - pri[c]);
        ac[s + 2] = a;
        if (aw) aw[(size_t)t * Sg + s] = a;
      }
      if (more) {
#pragma unroll
        for (int k = 0; k < CTC_ROW_REGS; ++k) {
          const int v = tid + k * CTC_THREADS;
          if (v < V1) rnext[v] = nx[k];
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double* al = ab[(Tb - 1) & 1];
      s_ll = ctc_lse3(al[S - 1 + 2], S >= 2 ? al[S - 2 + 2] : -INFINITY, -INFINITY);
    }
    __syncthreads();
    ll = s_ll;
    if (!(ll > -INFINITY && ll < INFINITY)) st_code = 1;  // every path runs through a -inf (or a NaN) score
  }
  if (st_code != 0 || Tb == 0) {  // refused row (or nothing to sum over): no other access
    if (tid == 0) {
      nll[b] = st_code ? (double)INFINITY : 0.0;
      status[b] = st_code;
    }
    if (dl)
      for (size_t i = tid; i < (size_t)V1 * T; i += CTC_THREADS) dl[i] = 0.f;
    return;
  }
  if (tid == 0) {
    nll[b] = -ll;
    status[b] = 0;
  }
  if (!dl) return;
  // ---- backward sweep ----
  const double* aw = alpha_ws + (size_t)b * T * Sg;
  const float gs = weight / ((float)B * (float)(Ub > 1 ? Ub : 1));
  const int TW = TT + 1;
  __syncthreads();  // (thread 0 has read the last alpha row)
  for (int s = tid; s < 2 * (CTC_MAX_S + 4); s += CTC_THREADS) (&ab[0][0])[s] = -INFINITY;
  for (int i = tid; i < V1 * TW; i += CTC_THREADS) tile[i] = 0ull;
  if (Tb < T) {  // frames at and beyond the row's length
    const int nz = T - Tb;
    for (size_t i = tid; i < (size_t)V1 * nz; i += CTC_THREADS) dl[(i / nz) * T + Tb + (i % nz)] = 0.f;
  }
  if (Tb > 1) {  // frame T_b - 1's row is where the forward sweep left it; frame T_b - 2's goes into the other buffer
    float* rn = rows + ((Tb - 2) & 1) * V1;
    for (int v = tid; v < V1; v += CTC_THREADS) rn[v] = lpb[(size_t)(Tb - 2) * V1 + v];
  }
  __syncthreads();
  for (int t = Tb - 1; t >= 0; --t) {
    const int cur = t & 1;
    const float* rw = rows + cur * V1;
    float* rnext = rows + (cur ^ 1) * V1;
    const double* bn = ab[cur ^ 1];
    double* bc = ab[cur];
    float nx[CTC_ROW_REGS];
    const bool more = t >= 1 && t < Tb - 1;  // frame t - 1's row (frame T_b - 2's is already staged)
    if (more) {
      const float* src = lpb + (size_t)(t - 1) * V1;
#pragma unroll
      for (int k = 0; k < CTC_ROW_REGS; ++k) {
        const int v = tid + k * CTC_THREADS;
        nx[k] = v < V1 ? src[v] : 0.f;
      }
    }
    const int tt = t % TT;
    const bool last = t == Tb - 1;
    for (int s = tid; s < S; s += CTC_THREADS) {
      const int c = cls[s] & ~CTC_SKIP;
      const double e = (double)rw[c] - pri[c];
      double v;
      if (last) {
        v = s >= S - 2 ? e : -INFINITY;
      } else {
        const double y2 = (s + 2 < S && (cls[s + 2] & CTC_SKIP)) ? bn[s + 4] : -INFINITY;
        v = ctc_lse3(bn[s + 2], bn[s + 3], y2) + e;
      }
      bc[s + 2] = v;
      const double w = exp(aw[(size_t)t * Sg + s] + v - e - ll);
      if (w > 0.0) atomicAdd(&tile[c * TW + tt], (unsigned long long)__double2ll_rn(w * CTC_FIX));
    }
    if (more) {
#pragma unroll
      for (int k = 0; k < CTC_ROW_REGS; ++k) {
        const int v = tid + k * CTC_THREADS;
        if (v < V1) rnext[v] = nx[k];
      }
    }
    __syncthreads();
    if (tt == 0) {  // (uniform) the sweep leaves the tile of frames [t, t + ntt)
      const int ntt = Tb - t < TT ? Tb - t : TT;
      for (int i = tid; i < ntt * V1; i += CTC_THREADS) {  // v fastest: the log-probs are read as they lie
        const int j = i / V1, v = i - j * V1;
        unsigned long long* cell = tile + v * TW + j;
        const float occ = (float)((double)*cell * (1.0 / CTC_FIX));
        *reinterpret_cast<float*>(cell) = gs * (expf(lpb[(size_t)(t + j) * V1 + v]) - occ);
      }
      __syncthreads();
      for (int i = tid; i < ntt * V1; i += CTC_THREADS) {  // t fastest: the gradient is written as it lies
        const int v = i / ntt, j = i - v * ntt;
        dl[(size_t)v * T + t + j] = *reinterpret_cast<const float*>(tile + v * TW + j);
      }
      __syncthreads();
      for (int i = tid; i < V1 * TW; i += CTC_THREADS) tile[i] = 0ull;
      __syncthreads();
    }
  }
}

// loss = mean_b(nll_b / max(U_b, 1)), summed in row order by one thread
__global__ void ctc_loss_mean_kernel(int B, int U, const double* __restrict__ nll, const int64_t* __restrict__ tg_len,
                                     float* __restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    const int64_t u = tg_len[b];
    s += nll[b] / (double)(u > 1 && u <= U ? u : 1);
  }
  *loss = (float)(s / (double)B);
}

}  // namespace sty

extern "C" int sty_ctc_loss_workspace_bytes(int B, int T, int V1, int U, size_t* bytes) {
  using namespace sty;
  if (!bytes || B < 1 || T < 1 || V1 < 2 || V1 > CTC_ROW_REGS * CTC_THREADS || U < 0 || U > CTC_MAX_U) {
    set_error("sty_ctc_loss_workspace_bytes: bad argument (B, T >= 1, 2 <= V1 <= %d, 0 <= U <= %d)",
              CTC_ROW_REGS * CTC_THREADS, CTC_MAX_U);
    return STY_EINVAL;
  }
  *bytes = (size_t)B * T * (2 * (size_t)U + 1) * sizeof(double) + 256;
  return STY_OK;
}

extern "C" int sty_ctc_loss_fwd_bwd(int B, int T, int V1, int U, const float* log_probs, const float* log_priors,
                                    float prior_scale, const int64_t* targets, const int64_t* input_lengths,
                                    const int64_t* target_lengths, int blank, float weight, double* nll, float* loss,
                                    int32_t* status, float* d_logits, void* workspace, size_t ws_bytes, void* stream) {
  using namespace sty;
  size_t need = 0;
  int rc = sty_ctc_loss_workspace_bytes(B, T, V1, U, &need);
  if (rc) return rc;
  if (blank < 0 || blank >= V1 || !log_probs || (U > 0 && !targets) || !input_lengths || !target_lengths || !nll || !loss ||
      !status || (d_logits && !workspace)) {
    set_error("sty_ctc_loss_fwd_bwd: bad argument (0 <= blank < V1, no null buffer but log_priors / d_logits)");
    return STY_EINVAL;
  }
  if (d_logits && ws_bytes < need) {
    set_error("sty_ctc_loss_fwd_bwd: workspace too small: need %zu bytes, have %zu", need, ws_bytes);
    return STY_ENOMEM;
  }
  // the gradient tile: as many frames (a power of two, at most 32) as the LDS beside the state rows holds
  int TT = 1;
  if (d_logits) {
    TT = 32;
    while (TT > 1 && CTC_LDS_STATIC + ctc_dyn_lds(V1, TT) > CTC_LDS_MAX) TT >>= 1;
  }
  const size_t lds = ctc_dyn_lds(V1, TT);
  if (CTC_LDS_STATIC + lds > CTC_LDS_MAX) {
    set_error("sty_ctc_loss_fwd_bwd: %d classes do not fit the LDS", V1);
    return STY_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const double cells = (double)B * T * (2.0 * U + 1);
  ProfScope prof("ctc_loss_kernel", (d_logits ? 60.0 : 25.0) * cells,
                 4.0 * B * T * V1 * (d_logits ? 3.0 : 1.0) + (d_logits ? 16.0 : 0.0) * cells, st);
  hipLaunchKernelGGL(ctc_loss_kernel, dim3(B), dim3(CTC_THREADS), lds, st, B, T, V1, U, log_probs, log_priors, prior_scale,
                     targets, input_lengths, target_lengths, blank, weight, nll, status, d_logits,
                     reinterpret_cast<double*>(workspace), TT);
  hipLaunchKernelGGL(ctc_loss_mean_kernel, dim3(1), dim3(64), 0, st, B, U, nll, target_lengths, loss);
  STY_LAUNCH_CHECK();
  return STY_OK;
}
