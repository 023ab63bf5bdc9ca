// Dense convs with FEW OUTPUT COLUMNS in the bf16 compute mode: the text encoder's q / k / v / o / proj convs (128 -> 128, K = 1), its
// feed-forward convs (128 <-> 512, K = 3), the pre-net (128 -> 128, K = 5) and their input-gradient convs, all at B L = 3 200 columns
// on c3 (reference call sites: text_encoder.py:79-86,214-223,325-330).  150-170 of these launches follow one another on the chain
// that ends the training step, so what counts is the time from launch to last store, not the rate of any one unit:
//   * many small workgroups, none persistent: a 64 (cout) x 32 (columns) tile per workgroup, 200 workgroups for 128 x 3 200;
//   * ONE stage: the whole Cin x (32 + K - 1) input tile goes into LDS at once (<= 37 KB), every global load of the workgroup --
//     the packed weight fragments included -- is in flight before the first wait, one barrier;
//   * a thread loads the eight consecutive CHANNELS of one column (dword loads, a wave covers 32 consecutive columns of two channel
//     octets: 128-byte rows), applies the prologue, rounds once with v_cvt_pk_bf16_f32 and writes ONE 16-byte LDS word that already
//     is the B operand of v_mfma_f32_32x32x16_bf16 for every tap (tap k reads the word of column + k): no transposition;
//   * the A operands are the bf16 fragments of convp16.hip (frag_pack_kernel), 16 bytes per lane straight from L2;
//   * the four waves split the REDUCTION (each a quarter of the input channels, all taps, both 32-row cout blocks); the partial
//     tiles are summed through LDS in the fixed order wave 0 + 1 + 2 + 3 (no atomics: two runs give the same bits), each wave
//     finishing a quarter of the tile;
//   * wide outputs over a short reduction (CoutP >= 256 and Cin K <= 384: the feed-forward's 128 -> 512, K = 3) split the COUTS
//     instead (CS: a wave takes 64 of a 256-row tile and the whole reduction; no partial tiles): with 64-row tiles eight workgroups
//     staged the same input tile, and the launch lost to convp16_kernel from 3 200 columns on (18.1 against 16.0 us);
//   * the output stage works on the accumulator layout: lanes along time, 128-byte rows per store instruction, no LDS staging.
// K = 1 has no halo: its 32 columns are taken from the flattened (batch, time) axis, as convk1_kernel does.  K = 3 / 5: tiles per
// utterance with their halo.
#include <stdlib.h>

#include "sty_common.h"

namespace sty {

constexpr int SC_CO = 64;       // output channels per workgroup (CS: per wave, four times that per workgroup)
constexpr int SC_TT = 32;       // output columns per workgroup
constexpr int SC_MAXCOLS = 3200;  // default of STY_CONVSC_MAX_COLS: the largest count of the sweep at which every shape wins
constexpr int SC_OOB = 0x7FFFFF00;  // a vector offset outside every descriptor: the load returns zeros

// NIT: most (column, channel octet) units a thread stages; QA / QB: most (channel sixteen, tap) steps of a wave whose weight
// fragments are requested at the start / behind the staging (when its registers are free again)
template <int NIT, int QA, int QB, bool CS>
__global__ __launch_bounds__(256) void convsc_kernel(ConvArgs a, int ncot, int ntiles, int per_xcd, int tiles_per_row) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, hi = lane >> 5;
  // workgroup ids go round-robin over the 8 XCDs: an XCD takes a contiguous range of tiles, the cout tiles of a column tile
  // (adjacent tile numbers) read their input through one L2
  const int tile = ((int)blockIdx.x & 7) * per_xcd + ((int)blockIdx.x >> 3);
  if (tile >= ntiles) return;
  const int cot = tile % ncot, ct = tile / ncot;
  const int T = a.T, K = a.w.K, Cin = a.w.Cin, Cout = a.w.Cout, CinP = a.w.CinP;
  const int NMB = a.w.CoutP / 32, J = 2 * K;
  const int LW = SC_TT + K - 1;
  const int P2 = CinP * 2 + 16;  // bytes between the LDS rows of two columns (dwords = 4 mod 64: conflict-free 16-byte reads)
  const int NTOT = a.B * T;
  const int bt = K == 1 ? 0 : ct / tiles_per_row;                     // K > 1: the tile's utterance
  const int t0 = K == 1 ? ct * SC_TT : (ct - bt * tiles_per_row) * SC_TT;  // first column (K == 1: of the flattened axis)

  // ---- weight fragments of this wave's steps: step i = (channel sixteen c_lo + i / K, tap i % K) ----
  const int n16 = CinP / 16;
  const int c_lo = CS ? 0 : wave * n16 / 4, c_hi = CS ? n16 : (wave + 1) * n16 / 4;
  const int q = (c_hi - c_lo) * K;
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w.wf), 0, K * CinP * a.w.CoutP * 2, 0x00020000);
  const int mb0 = CS ? cot * 8 + wave * 2 : cot * 2;  // this wave's two 32-row cout blocks
  int wv[2];  // fragments past CoutP: outside -> zeros
#pragma unroll
  for (int m = 0; m < 2; ++m) wv[m] = mb0 + m < NMB ? lane * 16 + m * 1024 : SC_OOB;
  bf16x8 fa[QA][2];
  bf16x8 fb[QB > 0 ? QB : 1][2];
  int fc16 = c_lo, fk = 0;  // (wave-uniform counters: no division per step)
  auto frag_load = [&](bf16x8* dst, bool on) {
    const int f = (((fc16 >> 1) * J + 2 * fk + (fc16 & 1)) * NMB + mb0) * 1024;
#pragma unroll
    for (int m = 0; m < 2; ++m)
      dst[m] = __builtin_bit_cast(
          bf16x8, __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rw, on ? wv[m] : SC_OOB, on ? f : 0, 0)));
    if (++fk == K) {
      fk = 0;
      ++fc16;
    }
  };
#pragma unroll
  for (int i = 0; i < QA; ++i) frag_load(fa[i], i < q);

  // ---- staging: unit u = tid + 256 it = (column j = u % LW, channel octet c8 = u / LW) ----
  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x[0]), 0, (unsigned)((size_t)a.B * Cin * T * 4), 0x00020000);
  const float* maskp = a.pro == PRO_MASK ? a.mask : nullptr;
  float xv[NIT][8];
  float mk[NIT];
  int ldst[NIT];
  {
    int j = tid % LW, c8 = tid / LW;
    const int dj = 256 % LW, dc = 256 / LW, nc8 = CinP / 8;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const bool live = c8 < nc8;
      int b, tin;
      bool cv;
      if (K == 1) {
        const int n = t0 + j;
        cv = n < NTOT;
        b = cv ? n / T : 0;
        tin = n - b * T;
      } else {
        b = bt;
        tin = t0 - a.pad + j;
        cv = tin >= 0 && tin < T;
      }
      cv = cv && live;
      const int base = ((b * Cin + 8 * c8) * T + tin) * 4;
#pragma unroll
      for (int e = 0; e < 8; ++e)  // (channels past Cin of the last octets and columns outside the utterance: zeros)
        xv[it][e] = __builtin_bit_cast(
            float, __builtin_amdgcn_raw_buffer_load_b32(rx, cv && 8 * c8 + e < Cin ? base + e * T * 4 : SC_OOB, 0, 0));
      mk[it] = 1.f;
      if (maskp) mk[it] = cv ? maskp[(size_t)b * T + tin] : 0.f;
      ldst[it] = live ? j * P2 + 16 * c8 : -1;
      j += dj;
      c8 += dc;
      if (j >= LW) {
        j -= LW;
        ++c8;
      }
    }
  }
  // ---- this lane's share of the output stage: element e of a wave = fragment element (cout block, r); its bias, residual and
  // mask are requested now, beside the input tile (behind the accumulation each residual load was a round trip of its own
  // between two stores: 20.4 us for 128 -> 512, K = 3 at 3 200 columns) ----
  constexpr int NV = CS ? 32 : 8;
  float val[NV], rs[NV], bi[NV], om = 1.f;
  int yo[NV];  // element offset of the output (convsc_eligible: below 2^31), -1: outside
  {
    int b, t;
    bool cv;
    if (K == 1) {
      const int n = t0 + l31;
      cv = n < NTOT;
      b = cv ? n / T : 0;
      t = n - b * T;
    } else {
      b = bt;
      t = t0 + l31;
      cv = t < T;
    }
    if (a.out_mask && cv) om = a.out_mask[(size_t)b * T + t];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
      const int mb = CS ? mb0 + (e >> 4) : mb0 + (wave >> 1), r = CS ? e & 15 : (wave & 1) * 8 + e;
      const int co = mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const bool ok = cv && co < Cout;
      yo[e] = ok ? (b * Cout + co) * T + t : -1;
      rs[e] = ok && a.residual ? a.residual[yo[e]] : 0.f;
      bi[e] = ok && a.w.bias ? a.w.bias[co] : 0.f;
    }
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (ldst[it] < 0) continue;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = maskp ? xv[it][e] * mk[it] : xv[it][e];
    *reinterpret_cast<bf16x8*>(sc_lds + ldst[it]) = sty_pack_bf16(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
  }
  if constexpr (QB > 0) {
#pragma unroll
    for (int i = 0; i < QB; ++i) frag_load(fb[i], QA + i < q);
  }
  __syncthreads();

  // ---- MFMA: lane (column l31, half hi) reads channels 16 c16 + 8 hi .. + 7 of column l31 + k ----
  f32x16 acc[2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
  const unsigned char* brow = sc_lds + l31 * P2 + hi * 16;
  int c16 = c_lo, k = 0;
  auto step = [&](const bf16x8* av) {
    const bf16x8 bv = *reinterpret_cast<const bf16x8*>(brow + k * P2 + c16 * 32);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[0], bv, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[1], bv, acc[1], 0, 0, 0);
    if (++k == K) {
      k = 0;
      ++c16;
    }
  };
#pragma unroll
  for (int i = 0; i < QA; ++i)
    if (i < q) step(fa[i]);
  if constexpr (QB > 0) {
#pragma unroll
    for (int i = 0; i < QB; ++i)
      if (QA + i < q) step(fb[i]);
  }

  // ---- output stage: bias, ReLU, scale, mask, residual, mask; lane = column, 128-byte rows per store instruction ----
  if constexpr (CS) {
#pragma unroll
    for (int e = 0; e < NV; ++e) val[e] = acc[e >> 4][e & 15];
  } else {
    // the waves' partial tiles, summed in a fixed order; wave w finishes cout block w >> 1, fragment rows 8 (w & 1) .. + 7
    __syncthreads();  // every wave is done with the input tile: its LDS holds the partial tiles [wave][32 values][64 lanes] now
    float* red = reinterpret_cast<float*>(sc_lds);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(wave * 32 + m * 16 + r) * 64 + lane] = acc[m][r];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NV; ++e) {
      const float* p = red + ((wave >> 1) * 16 + (wave & 1) * 8 + e) * 64 + lane;
      val[e] = ((p[0] + p[32 * 64]) + p[2 * 32 * 64]) + p[3 * 32 * 64];
    }
  }
  const bool post = a.out_mask && a.out_mask_post, relu = a.act == ACT_RELU;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    if (yo[e] < 0) continue;
    float x = val[e] + bi[e];
    if (relu) x = fmaxf(x, 0.f);
    x *= a.out_scale;
    if (a.out_mask && !post) x *= om;
    x += rs[e];
    if (post) x *= om;
    a.y[yo[e]] = x;
  }
}

int convp16_frags(const ConvArgs& a, hipStream_t st, const void** out);  // convp16.hip

// staging iterations of a thread and steps of the busiest wave
static int sc_nit(const ConvArgs& a) { return cdiv((SC_TT + a.w.K - 1) * (a.w.CinP / 8), 256); }
static bool sc_cs(const ConvArgs& a) { return a.w.CoutP >= 256 && a.w.CinP * a.w.K <= 384 && sc_nit(a) <= 3; }  // waves split the couts
static int sc_q(const ConvArgs& a) { return (sc_cs(a) ? a.w.CinP / 16 : cdiv(a.w.CinP / 16, 4)) * a.w.K; }

bool convsc_eligible(const ConvArgs& a) {
  if (!a.bf16 || getenv("STY_NO_CONVSC")) return false;  // (read per call: the parity tests toggle it)
  // an explicit threshold of a neighbouring family names that family: it keeps the convs it asks for
  if (getenv("STY_CONVK1_MIN_TILES") || getenv("STY_CONVP16_MIN_TILES")) return false;
  if (!(a.w.K == 1 || a.w.K == 3 || a.w.K == 5) || a.dil != 1 || a.pad != (a.w.K - 1) / 2) return false;
  if (a.nsrc != 1 || a.flatW || a.Tin || a.in_shuffle > 1 || a.shuffle != 1 || a.ln_out || a.y_split || a.stat_part) return false;
  if (a.x16 || a.y16 || a.xh || a.yh || a.rh || a.up_g) return false;
  if (!(a.pro == PRO_NONE || (a.pro == PRO_MASK && a.mask)) || !(a.act == ACT_NONE || a.act == ACT_RELU)) return false;
  if (a.T % 4 || a.w.CinP < 64 || a.w.CinP % 32) return false;  // (T % 4: the set the tests cover, not a need of the kernel)
  if (sc_nit(a) > 9 || sc_q(a) > 24) return false;             // the largest instantiation: Cin 512 at K = 3
  // one buffer descriptor over the input, 31-bit byte offsets; 32-bit element offsets into the output
  if ((size_t)a.B * a.w.Cin * a.T * 4 >= (size_t)1 << 31 || (size_t)a.B * a.w.Cout * a.T * 4 >= (size_t)1 << 31) return false;
  const char* mc = getenv("STY_CONVSC_MAX_COLS");  // read per call
  return (long)a.B * a.T <= (mc ? atol(mc) : SC_MAXCOLS);
}

template <int NIT, int QA, int QB, bool CS = false>
static void sc_launch(const ConvArgs& a, int ncot, int ntiles, int tpr, size_t lds, hipStream_t st) {
  const int per = cdiv(ntiles, 8);
  hipLaunchKernelGGL((convsc_kernel<NIT, QA, QB, CS>), dim3(per * 8), dim3(256), lds, st, a, ncot, ntiles, per, tpr);
}

int launch_convsc(const ConvArgs& a0, hipStream_t st) {
  ConvArgs a = a0;
  int rc = convp16_frags(a0, st, &a.w.wf);
  if (rc) return rc;
  const int K = a.w.K, LW = SC_TT + K - 1;
  const bool cs = sc_cs(a);
  const int tpr = cdiv(a.T, SC_TT), ncot = cdiv(a.w.CoutP, cs ? 4 * SC_CO : SC_CO);
  const int ncol = K == 1 ? cdiv(a.B * a.T, SC_TT) : tpr * a.B;
  const int ntiles = ncol * ncot;
  size_t lds = (size_t)LW * (a.w.CinP * 2 + 16);
  if (lds < 4 * 32 * 64 * sizeof(float)) lds = 4 * 32 * 64 * sizeof(float);  // the partial tiles
  const double outs = (double)a.B * a.w.Cout * a.T;
  char detail[40];
  snprintf(detail, sizeof(detail), "ci%d co%d k%d T%d W0", a.w.Cin, a.w.Cout, K, a.T);
  ProfScope prof("convsc_kernel<true>", 2.0 * a.w.Cin * K * outs,
                 4.0 * ((double)a.B * a.w.Cin * a.T + outs * (a.residual ? 2.0 : 1.0)) + 2.0 * a.w.Cout * a.w.Cin * K, st, detail);
  const int nit = sc_nit(a), q = sc_q(a);
  if (cs)  // (sc_cs: nit <= 3, q <= 24)
    sc_launch<3, 12, 12, true>(a, ncot, ntiles, tpr, lds, st);
  else if (nit <= 2 && q <= 2)
    sc_launch<2, 2, 0>(a, ncot, ntiles, tpr, lds, st);
  else if (nit <= 3 && q <= 10)
    sc_launch<3, 10, 0>(a, ncot, ntiles, tpr, lds, st);
  else if (nit <= 9 && q <= 24)
    sc_launch<9, 12, 12>(a, ncot, ntiles, tpr, lds, st);
  else {
    set_error("convsc: Cin %d K %d is beyond the kernel's instantiations", a.w.Cin, K);
    return STY_EINVAL;
  }
  STY_LAUNCH_CHECK();
  return STY_OK;
}

}  // namespace sty
