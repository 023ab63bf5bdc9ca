// The weight side of a model (weights.hip): bound parameters -> prepared (packed) weights before a forward, packed gradients ->
// the caller's gradient buffers after a backward.  The Builder (builder.hip) describes the work as a list of PackJob; five device
// tables, one typed record each, let every step cover all layers of a model in one launch.  See DESIGN.md section 4.
#pragma once
#include <vector>

#include "sty_common.h"

struct sty_model;

namespace sty {

// ---- host side: what the Builder emits, one entry per prepared tensor ----
enum PackKind { PK_CONV, PK_CONV_WN, PK_CONV_GLU, PK_W2A, PK_CONV2D_SN, PK_DW2D_SN, PK_DGRAD, PK_DGRAD2D, PK_SPLIT3 };
struct PackJob {
  PackKind kind;
  const float *w = nullptr, *g = nullptr, *v = nullptr, *bias = nullptr, *extra = nullptr;
  int Cout = 0, Cin = 0, K = 1, CinP = 0, CoutP = 0, KH = 1;
  float* wp = nullptr;
  float* bp = nullptr;
  float* scratch = nullptr;
  float* scratch2 = nullptr;  // spectral norm, training: n + Cout floats for the power iteration

  // dense conv / linear with the dims of `pc`: plain (w) or weight norm (w == nullptr, g, v); kind PK_CONV_GLU: GLU channel order
  static PackJob conv(PackKind kind, const PackedConv& pc, const float* w, const float* g, const float* v, const float* bias,
                      float* wp, float* bp) {
    PackJob j;
    j.kind = kind, j.w = w, j.g = g, j.v = v, j.bias = bias, j.wp = wp, j.bp = bp;
    j.Cout = pc.Cout, j.Cin = pc.Cin, j.K = pc.K, j.CinP = pc.CinP, j.CoutP = pc.CoutP;
    return j;
  }
  // input-gradient weights of the packed conv `fwd` -> wd
  static PackJob dgrad(const PackedConv& fwd, float* wd) {
    PackJob j;
    j.kind = PK_DGRAD, j.w = fwd.wp, j.K = fwd.K, j.CinP = fwd.CinP, j.CoutP = fwd.CoutP, j.wp = wd;
    return j;
  }
  // bf16 A-fragment triples of the packed 32 x 32 conv `pc` -> w3 (the split mode of conv32p.hip)
  static PackJob split3(const PackedConv& pc, float* w3) {
    PackJob j;
    j.kind = PK_SPLIT3, j.w = pc.wp, j.K = pc.K, j.CinP = pc.CinP, j.CoutP = pc.CoutP, j.wp = w3;
    return j;
  }
  // ... of a 2-D conv packed as `fwd` (reduction index (kh, ci), K = KW) -> wd
  static PackJob dgrad2d(const PackedConv& fwd, int Cin, int KH, float* wd) {
    PackJob j = dgrad(fwd, wd);
    j.kind = PK_DGRAD2D, j.Cout = fwd.Cout, j.Cin = Cin, j.KH = KH;
    return j;
  }
  // ConvNeXt pwconv2 [C][4C]: chained-GEMM fragments w2a and b2eff = b2 + W2 . grn_beta
  static PackJob w2a(const float* w2, const float* b2, const float* grn_beta, int C, float* w2a, float* b2eff) {
    PackJob j;
    j.kind = PK_W2A, j.w = w2, j.bias = b2, j.extra = grn_beta, j.Cout = C, j.wp = w2a, j.bp = b2eff;
    return j;
  }
  // spectral-normed Conv2d [Cout][Cin][KH][KW] -> packed as `pc`; t: sigma row terms [Cout], power: power-iteration scratch
  static PackJob conv2d_sn(const PackedConv& pc, int Cin, int KH, const float* w, const float* u, const float* v,
                           const float* bias, float* wp, float* bp, float* t, float* power) {
    PackJob j = conv(PK_CONV2D_SN, pc, w, u, v, bias, wp, bp);
    j.Cin = Cin, j.KH = KH, j.scratch = t, j.scratch2 = power;
    return j;
  }
  // spectral-normed depthwise 3 x 3 [C][1][3][3] -> w9 [C][9]
  static PackJob dw2d_sn(int C, const float* w, const float* u, const float* v, float* w9, float* t, float* power) {
    PackJob j;
    j.kind = PK_DW2D_SN, j.w = w, j.g = u, j.v = v, j.Cout = C, j.wp = w9, j.scratch = t, j.scratch2 = power;
    return j;
  }
};

// ---- device side: one record per job of a table.  blk0 = the job's first block in the table's block list ----
struct ConvPackJob {  // plain weight w, or (g, v) of weight norm, [Cout][Cin][K] -> wp [K][CinP][CoutP]; bias -> bp (0 without one)
  const float *w = nullptr, *g = nullptr, *v = nullptr, *bias = nullptr;
  float *wp = nullptr, *bp = nullptr;
  int Cout = 0, Cin = 0, K = 1, CinP = 0, CoutP = 0;
  int glu = 0;  // output channels interleaved in 32-blocks (value block, gate block) for ACT_GLU
  int blk0 = 0;
};
struct DgradPackJob {  // packed weights wp -> input-gradient weights wd
  const float* wp = nullptr;
  float* wd = nullptr;
  int K = 1, CinP = 0, CoutP = 0;                    // of the forward conv (K = KW in 2-D)
  int two_d = 0;                                     // flat 2-D layout: rows (kh', co), columns ci, taps flipped both ways
  int KH = 1, Cin = 0, Cout = 0, CinPd = 0, CoutPd = 0;  // two_d only: the layer's dims and the padded extents of wd
  int blk0 = 0;
};
struct SplitPackJob {  // packed weights wp [K][32][32] -> w3: the three bf16 pieces of every weight as MFMA A fragments
  const float* wp = nullptr;
  void* w3 = nullptr;  // [K][2 k-steps][3 pieces][64 lanes] x 16 B (split3_bytes)
  int K = 1;
  int blk0 = 0;
};
struct GradUnpackJob {  // packed gradient gwp (+ packed bias gradient gbp) -> dW, or (dg, dv) of weight norm, and db; all +=
  const float *gwp = nullptr, *g = nullptr, *v = nullptr, *gbp = nullptr;  // v != nullptr: weight norm
  float *dW = nullptr, *dg = nullptr, *dv = nullptr, *db = nullptr;
  int Cout = 0, Cin = 0, K = 1, CinP = 0, CoutP = 0;
  int blk0 = 0;
};
struct SnPrepJob {  // spectral norm: W [Cout][Cin][KH][KW] (depthwise: [C][9]), u, v -> t (sigma row terms), wp = packed W / sigma
  const float *w = nullptr, *bias = nullptr;
  float *u = nullptr, *v = nullptr;  // written by the training-mode power iteration
  float *t = nullptr, *power = nullptr, *wp = nullptr, *bp = nullptr;  // power: SN_SLICES n + Cout floats (conv2d.hip)
  int Cout = 0, Cin = 0, K = 1, KH = 1, CinP = 0, CoutP = 0;
  int depthwise = 0;
  int blk0 = 0;   // in the row list (one block per output channel)
  int wtu0 = 0;   // in the W^T u block list of the power iteration
};
struct SnUnpackJob {  // dW[co][i] += G[co][i] / sigma - (<G, W> / sigma^2) u[co] v[i], G from the packed gradient gwp; db += gbp
  const float *gwp = nullptr, *w = nullptr, *u = nullptr, *v = nullptr, *t = nullptr, *gbp = nullptr;
  float *dW = nullptr, *gw_rows = nullptr, *db = nullptr;  // gw_rows: <G, W> row sums [Cout] (scratch)
  int Cout = 0, Cin = 0, K = 1, KH = 1, CinP = 0, CoutP = 0;
  int blk0 = 0;
};

// a device int list: which job a block of a table's grid works on
struct BlockList {
  int* dev = nullptr;
  int n = 0;
  int upload(const std::vector<int>& host) {
    free();
    n = (int)host.size();
    if (!n) return STY_OK;
    STY_HIP(hipMalloc((void**)&dev, host.size() * sizeof(int)));
    STY_HIP(hipMemcpy(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));
    return STY_OK;
  }
  void free() {
    if (dev) (void)hipFree(dev);
    dev = nullptr;
    n = 0;
  }
};
// one device table: the jobs and the job of every block
template <typename Job>
struct JobTable {
  Job* jobs = nullptr;
  int njobs = 0;
  BlockList blocks;
  int upload(const std::vector<Job>& host, const std::vector<int>& job_of_block) {
    free();
    njobs = (int)host.size();
    if (!njobs) return STY_OK;
    STY_HIP(hipMalloc((void**)&jobs, host.size() * sizeof(Job)));
    STY_HIP(hipMemcpy(jobs, host.data(), host.size() * sizeof(Job), hipMemcpyHostToDevice));
    return blocks.upload(job_of_block);
  }
  void free() {
    if (jobs) (void)hipFree(jobs);
    jobs = nullptr;
    njobs = 0;
    blocks.free();
  }
};
// the tables of a model, built from its PackJob list on first use after a finalize (weights_build_tables)
struct WeightTables {
  JobTable<ConvPackJob> pack;
  JobTable<DgradPackJob> dgrad;
  JobTable<SplitPackJob> split3;  // (only while sty_model_set_fp32_split is on at the finalize)
  JobTable<GradUnpackJob> unpack;
  JobTable<SnPrepJob> sn_prep;
  BlockList sn_wtu;  // sn_prep's second grid: the W^T u blocks of the power iteration
  JobTable<SnUnpackJob> sn_unpack;
  int seg_blk_split = 0;  // `unpack` blocks [0, seg_blk_split) belong to gradient segment 1 (sty_model::seg_job_split)
  bool ready = false;
  void free() {
    pack.free(), dgrad.free(), split3.free(), unpack.free(), sn_prep.free(), sn_wtu.free(), sn_unpack.free();
    ready = false;
  }
};

int weights_build_tables(sty_model* m);
// bound parameters -> prepared weights, every kind, on `st`
int weights_prepare(sty_model* m, hipStream_t st);
// the training-mode power iteration of every spectral-norm layer (u, v in the caller's buffers); weights_prepare follows
int weights_sn_power_iter(sty_model* m, hipStream_t st);
// packed gradients -> the caller's parameter gradients (+=)
// seg: -1 = every parameter; 1 = the pack jobs before seg_job_split (text encoder of a speech predictor); 0 = everything else
int weights_unpack(sty_model* m, hipStream_t st, int seg = -1);

// one launch per table
int launch_conv_pack_table(const JobTable<ConvPackJob>& t, hipStream_t st);
int launch_dgrad_pack_table(const JobTable<DgradPackJob>& t, hipStream_t st);
int launch_split3_pack_table(const JobTable<SplitPackJob>& t, hipStream_t st);
int launch_grad_unpack_table(const JobTable<GradUnpackJob>& t, int blk_base, int nblocks, hipStream_t st);  // a block sub-range
int launch_sn_unpack_table(const JobTable<SnUnpackJob>& t, hipStream_t st);
// conv2d.hip: spectral-norm weight preparation of EVERY spectral-norm layer of a model in a few launches (power_iter: the
// training-mode power iteration; pack: sigma and the packed W / sigma)
int launch_sn_prep_table(const JobTable<SnPrepJob>& t, const BlockList& wtu, bool power_iter, bool pack, hipStream_t st);
int sn_wtu_blocks(int n);  // W^T u blocks of a layer with n weights per output channel

// one job, outside a model (discriminators, the sty_conv1d_* unit entries)
int launch_pack_conv(const float* w, const float* g, const float* v, const float* bias, int Cout, int Cin, int K,
                     float* wp, float* bp, int CinP, int CoutP, hipStream_t st);
int launch_pack_dgrad(const float* wp, int K, int CinP, int CoutP, float* wd, hipStream_t st);
int launch_pack_split3(const float* wp, int K, void* w3, hipStream_t st);  // wp [K][32][32] -> split3_bytes(K) at w3
int launch_pack_dgrad2d(const float* wp, int KW, int KH, int Cin, int Cout, int CinP, int CoutP, int CinPd, int CoutPd,
                        float* wd, hipStream_t st);
int launch_unpack_grad(const float* gwp, const float* g, const float* v, int Cout, int Cin, int K, int CinP, int CoutP,
                       float* dW, float* dg, float* dv, hipStream_t st);
int launch_b2eff_bwd(const float* g, const float* w2, const float* beta, int C, float* db2, float* dbeta, float* dW2,
                     hipStream_t st);

}  // namespace sty
