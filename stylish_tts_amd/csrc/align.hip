// The alignment stage's device code (train/dataprep/align_text.py, train/models/text_aligner.py): the inference forward's
// glue and the forced alignment.  The training graph is in train.hip (Trainer::aligner), the CTC loss in ctc.hip.
//
// (1) Element-wise / row kernels of the TextAligner forward (the convs and Linears run on launch_conv1d):
//       aligner_bn_prep_kernel   running_mean / running_var -> scale = 1 / sqrt(var + eps), shift = -mean * scale   (prepare)
//       aligner_bn_kernel        y = x * scale[c] + shift[c] behind a conv whose epilogue already applied the ReLU
//       log_softmax_rows_kernel  logits [B][V][T] (channel-major, as the GEMM writes them) -> log_probs [B][T][V]
// (2) CTC forced alignment (torchaudio.functional.forced_align as align_text.py:317 calls it): Viterbi over the
//     S = 2 U_b + 1 states "blank, tok, blank, ..., blank" of one utterance per workgroup.
//
// The dynamic programme.  alpha[t][s] = best score of a path that ends in state s at frame t; fp32 max and + only, so a
// host restatement with the same recurrence gives the same bits.  Per frame a workgroup
//   - holds alpha of frame t - 1 and of frame t in two LDS rows (two leading -inf cells stand in for states -1 and -2),
//   - holds frame t's log-prob row in LDS (staged once per frame: frame t + 1's row is loaded into registers at the top of
//     frame t and stored to the other LDS row at its end, so the one barrier per frame also publishes it),
//   - lane = state: x0 = stay, x1 = from s - 1, x2 = from s - 2 (token states whose token differs from the previous token);
//     x2 if x2 > x1 && x2 > x0, else x1 if x1 > x0 && x1 > x2, else x0,
//   - packs the 2-bit back-pointers of 64 states into two 64-bit ballots (bit 0 / bit 1) that lane 0 of the wave stores:
//     workspace [B][T][ceil((2 U + 1) / 64)][2] uint64.
// One thread then walks the back-pointers from the end state (S - 1 if alpha[S - 1] > alpha[S - 2], else S - 2) and leaves
// the state path in `labels`; the workgroup turns it into classes and gathers the scores in one coalesced pass.
// Every index is derived from values the kernel has range-checked: a row whose lengths or targets are out of range gets
// status 2, a row with input_length < target_length + repeats status 1; both get labels -1 and touch nothing else.
#include "sty_common.h"

namespace sty {

// ---- TextAligner glue ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aligner_bn_prep_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                              int C, float eps, float* __restrict__ scale,
                                                              float* __restrict__ shift) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float s = 1.0f / sqrtf(var[c] + eps);
  scale[c] = s;
  shift[c] = -mean[c] * s;
}
int launch_aligner_bn_prep(const float* mean, const float* var, int C, float eps, float* scale, float* shift,
                           hipStream_t st) {
  hipLaunchKernelGGL(aligner_bn_prep_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, mean, var, C, eps, scale, shift);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

__global__ __launch_bounds__(256) void fill_f32_kernel(float* __restrict__ x, int n, float v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = v;
}
int launch_fill_f32(float* x, int n, float v, hipStream_t st) {
  hipLaunchKernelGGL(fill_f32_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, x, n, v);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// one thread per element of [B][C][T], in place
__global__ __launch_bounds__(256) void aligner_bn_kernel(float* __restrict__ x, size_t n, int C, int T,
                                                         const float* __restrict__ scale, const float* __restrict__ shift) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)((i / T) % C);
  x[i] = x[i] * scale[c] + shift[c];
}
int launch_aligner_bn(float* x, int B, int C, int T, const float* scale, const float* shift, hipStream_t st) {
  const size_t n = (size_t)B * C * T;
  ProfScope prof("aligner_bn_kernel", 2.0 * n, 8.0 * n, st);
  hipLaunchKernelGGL(aligner_bn_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n, C, T, scale, shift);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// log_softmax over the V channels of logits [B][V][T] -> out [B][T][V].  A workgroup takes LS_TT frames of one batch row:
// the tile is read with t fastest (coalesced), transposed through LDS, and each wave reduces whole frames with shuffles
// (max, then sum of exp), lanes striding over the classes, and writes the frame's V values contiguously.
constexpr int LS_TT = 32;
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__global__ __launch_bounds__(256) void log_softmax_rows_kernel(const float* __restrict__ x, int V, int T,
                                                               float* __restrict__ out) {
  extern __shared__ float tile[];  // [V][LS_TT + 1]
  const int b = blockIdx.y, t0 = blockIdx.x * LS_TT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tt = tid & (LS_TT - 1);
  for (int v = tid / LS_TT; v < V; v += 256 / LS_TT) {
    const int t = t0 + tt;
    tile[v * (LS_TT + 1) + tt] = t < T ? x[((size_t)b * V + v) * T + t] : 0.f;
  }
  __syncthreads();
  for (int r = wave; r < LS_TT; r += 4) {
    const int t = t0 + r;
    if (t >= T) break;  // (wave-uniform)
    float mx = -INFINITY;
    for (int v = lane; v < V; v += 64) mx = fmaxf(mx, tile[v * (LS_TT + 1) + r]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(tile[v * (LS_TT + 1) + r] - mx);
    s = wave_sum(s);
    const float lse = mx + logf(s);
    float* o = out + ((size_t)b * T + t) * V;
    for (int v = lane; v < V; v += 64) o[v] = tile[v * (LS_TT + 1) + r] - lse;
  }
}
int launch_log_softmax_rows(const float* x, int B, int V, int T, float* out, hipStream_t st) {
  const size_t lds = (size_t)V * (LS_TT + 1) * sizeof(float);
  if (lds > 64 * 1024) {
    set_error("log_softmax_rows: %d classes do not fit the LDS tile (at most %d)", V, (int)(64 * 1024 / ((LS_TT + 1) * 4)));
    return STY_EINVAL;
  }
  ProfScope prof("log_softmax_rows_kernel", 4.0 * B * V * T, 8.0 * B * V * T, st);
  hipLaunchKernelGGL(log_softmax_rows_kernel, dim3(cdiv(T, LS_TT), B), dim3(256), lds, st, x, V, T, out);
  STY_LAUNCH_CHECK();
  return STY_OK;
}

// ---- CTC forced alignment -----------------------------------------------------------------------------------------
constexpr int FA_THREADS = 256;
constexpr int FA_MAX_U = 512;                 // S = 2 U + 1 <= 1025 states
constexpr int FA_MAX_S = 2 * FA_MAX_U + 1;
constexpr int FA_ROW_REGS = 4;                // frame t + 1's row in registers: V1 <= FA_ROW_REGS * FA_THREADS
constexpr int FA_SKIP = 1 << 30;              // cls[] flag: the state may be entered from s - 2

static inline int fa_chunks(int U) { return (2 * U + 1 + 63) / 64; }

__global__ __launch_bounds__(FA_THREADS) void forced_align_kernel(int T, int V1, int U, const float* __restrict__ lp,
                                                                  const int64_t* __restrict__ targets,
                                                                  const int64_t* __restrict__ in_len,
                                                                  const int64_t* __restrict__ tg_len, int blank,
                                                                  int32_t* __restrict__ labels, float* __restrict__ scores,
                                                                  int32_t* __restrict__ status,
                                                                  unsigned long long* __restrict__ bp, int nchunk) {
  extern __shared__ float rows[];  // [2][V1]
  __shared__ float alpha[2][FA_MAX_S + 2];
  __shared__ int cls[FA_MAX_S];
  __shared__ int s_bad, s_rep;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t Tb64 = in_len[b], Ub64 = tg_len[b];
  int32_t* lab = labels + (size_t)b * T;
  float* sc = scores + (size_t)b * T;
  const float* lpb = lp + (size_t)b * T * V1;
  const bool bad_len = Tb64 < 0 || Tb64 > T || Ub64 < 0 || Ub64 > U;  // (uniform)
  const int Tb = bad_len ? 0 : (int)Tb64, Ub = bad_len ? 0 : (int)Ub64;
  const int S = 2 * Ub + 1;
  if (tid == 0) {
    s_bad = bad_len ? 1 : 0;
    s_rep = 0;
  }
  __syncthreads();
  // states: class and whether the skip transition is allowed; repeats and target range on the way
  for (int s = tid; s < S; s += FA_THREADS) {
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
            c |= FA_SKIP;
        }
      }
    }
    cls[s] = c;
  }
  __syncthreads();
  const int st_code = s_bad ? 2 : (Tb < Ub + s_rep ? 1 : 0);
  if (st_code != 0 || Tb == 0) {  // refused row (or nothing to align): labels -1, scores 0, no other access
    for (int t = tid; t < T; t += FA_THREADS) {
      lab[t] = -1;
      sc[t] = 0.f;
    }
    if (tid == 0) status[b] = st_code;
    return;
  }
  float* row0 = rows;
  float* row1 = rows + V1;
  for (int v = tid; v < V1; v += FA_THREADS) row0[v] = lpb[v];
  for (int s = tid; s < FA_MAX_S + 2; s += FA_THREADS) {
    alpha[0][s] = -INFINITY;
    alpha[1][s] = -INFINITY;
  }
  __syncthreads();
  if (tid < 2 && tid < S) alpha[0][tid + 2] = row0[cls[tid] & ~FA_SKIP];
  if (Tb > 1)
    for (int v = tid; v < V1; v += FA_THREADS) row1[v] = lpb[(size_t)V1 + v];
  __syncthreads();
  const int nch = (S + 63) >> 6;
  for (int t = 1; t < Tb; ++t) {
    const int cur = t & 1;
    const float* rw = cur ? row1 : row0;
    float* rnext = cur ? row0 : row1;
    const float* ap = alpha[cur ^ 1];
    float* ac = alpha[cur];
    float nx[FA_ROW_REGS];
    const bool more = t + 1 < Tb;
    if (more) {
      const float* src = lpb + (size_t)(t + 1) * V1;
#pragma unroll
      for (int k = 0; k < FA_ROW_REGS; ++k) {
        const int v = tid + k * FA_THREADS;
        nx[k] = v < V1 ? src[v] : 0.f;
      }
    }
    unsigned long long* bpt = bp + ((size_t)b * T + t) * nchunk * 2;
    for (int c = wave; c < nch; c += FA_THREADS / 64) {  // (wave-uniform bounds: the ballots see whole waves)
      const int s = c * 64 + lane;
      int back = 0;
      if (s < S) {
        const int cl = cls[s];
        const float x0 = ap[s + 2], x1 = ap[s + 1];
        const float x2 = (cl & FA_SKIP) ? ap[s] : -INFINITY;
        float best;
        if (x2 > x1 && x2 > x0) {
          best = x2;
          back = 2;
        } else if (x1 > x0 && x1 > x2) {
          best = x1;
          back = 1;
        } else {
          best = x0;
        }
        ac[s + 2] = best + rw[cl & ~FA_SKIP];
      }
      const unsigned long long b0 = __ballot(back & 1), b1 = __ballot(back & 2);
      if (lane == 0) {
        bpt[c * 2] = b0;
        bpt[c * 2 + 1] = b1;
      }
    }
    if (more) {
#pragma unroll
      for (int k = 0; k < FA_ROW_REGS; ++k) {
        const int v = tid + k * FA_THREADS;
        if (v < V1) rnext[v] = nx[k];
      }
    }
    __syncthreads();
  }
  // back-track: one thread walks the chain and leaves the STATE path in `labels`
  if (tid == 0) {
    const float* al = alpha[(Tb - 1) & 1];
    int s = (S >= 2 && !(al[S - 1 + 2] > al[S - 2 + 2])) ? S - 2 : S - 1;
    for (int t = Tb - 1; t >= 0; --t) {
      lab[t] = s;
      if (t > 0) {
        const unsigned long long* w = bp + (((size_t)b * T + t) * nchunk + (s >> 6)) * 2;
        const int back = (int)((w[0] >> (s & 63)) & 1ull) | ((int)((w[1] >> (s & 63)) & 1ull) << 1);
        s -= back;  // (a back-pointer of 1 / 2 is only ever stored for s >= 1 / s >= 2: alpha of states -1, -2 is -inf)
        if (s < 0) s = 0;
      }
    }
    status[b] = 0;
  }
  __syncthreads();
  for (int t = tid; t < T; t += FA_THREADS) {
    if (t < Tb) {
      const int c = cls[lab[t]] & ~FA_SKIP;
      lab[t] = c;
      sc[t] = lpb[(size_t)t * V1 + c];
    } else {
      lab[t] = -1;
      sc[t] = 0.f;
    }
  }
}

}  // namespace sty

extern "C" int sty_forced_align_workspace_bytes(int B, int T, int U, size_t* bytes) {
  using namespace sty;
  if (!bytes || B <= 0 || T <= 0 || U < 0 || U > FA_MAX_U) {
    set_error("sty_forced_align_workspace_bytes: bad argument (B, T >= 1, 0 <= U <= %d)", FA_MAX_U);
    return STY_EINVAL;
  }
  *bytes = (size_t)B * T * fa_chunks(U) * 2 * sizeof(unsigned long long) + 256;
  return STY_OK;
}

extern "C" int sty_forced_align(int B, int T, int V1, int U, const float* log_probs, const int64_t* targets,
                                const int64_t* input_lengths, const int64_t* target_lengths, int blank, int32_t* labels,
                                float* scores, int32_t* status, void* workspace, size_t ws_bytes, void* stream) {
  using namespace sty;
  if (B <= 0 || T <= 0 || V1 <= 0 || U < 0 || U > FA_MAX_U || V1 > FA_ROW_REGS * FA_THREADS || blank < 0 || blank >= V1 ||
      !log_probs || (U > 0 && !targets) || !input_lengths || !target_lengths || !labels || !scores || !status || !workspace) {
    set_error("sty_forced_align: bad argument (B, T >= 1, 0 <= U <= %d, 1 <= V1 <= %d, 0 <= blank < V1, no null buffer)",
              FA_MAX_U, FA_ROW_REGS * FA_THREADS);
    return STY_EINVAL;
  }
  size_t need = 0;
  int rc = sty_forced_align_workspace_bytes(B, T, U, &need);
  if (rc) return rc;
  if (ws_bytes < need) {
    set_error("sty_forced_align: workspace too small: need %zu bytes, have %zu", need, ws_bytes);
    return STY_ENOMEM;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t lds = (size_t)2 * V1 * sizeof(float);
  ProfScope prof("forced_align_kernel", 6.0 * B * T * (2.0 * U + 1), 4.0 * B * T * V1 + 0.5 * B * T * (2.0 * U + 1), st);
  hipLaunchKernelGGL(forced_align_kernel, dim3(B), dim3(FA_THREADS), lds, st, T, V1, U, log_probs, targets, input_lengths,
                     target_lengths, blank, labels, scores, status, reinterpret_cast<unsigned long long*>(workspace),
                     fa_chunks(U));
  STY_LAUNCH_CHECK();
  return STY_OK;
}
