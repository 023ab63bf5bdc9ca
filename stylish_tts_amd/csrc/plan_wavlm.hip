// The WavLM graph of the slm loss: forward (with its keep mode), backward to the wave, the strided feature conv pair and its
// unit entry, the resampler and the loss entries (wavlm.hip has the kernels, weights.hip the packs).  See include/stylish_hip.h.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "run.h"

namespace sty {

// frames after conv layer i of N16 samples: floor((n - k) / s) + 1; 0 when a layer is left without a frame
static int wavlm_frames_at(const WavlmPlan& p, int N16, int layer) {
  long long n = N16;
  for (int i = 0; i <= layer; ++i) {
    if (n < p.kern[i]) return 0;
    n = (n - p.kern[i]) / p.stride[i] + 1;
  }
  return (int)n;
}
// What the forward and the backward size their buffers by: Tl[i], the frames behind conv layer i; Tp[i] = Tl[i] + K - 1, the
// columns of the staged view conv i >= 1 reads; the largest layer output and the largest staged view, in floats (bf16 mode: an
// output's rows may be Tp columns wide -- the padded rows a twin family leaves, or those of a gradient twin)
struct WavlmDims {
  int Tl[WAVLM_MAX_CONV], Tp[WAVLM_MAX_CONV];
  size_t max_out = 0, max_stage = 0;
};
static WavlmDims wavlm_dims(const WavlmPlan& p, int B, int N16, bool bf16) {
  WavlmDims d{};
  for (int i = 0; i < p.n_conv; ++i) {
    d.Tl[i] = wavlm_frames_at(p, N16, i);
    d.max_out = std::max(d.max_out, (size_t)B * p.dim[i] * d.Tl[i]);
    if (i) {
      d.Tp[i] = d.Tl[i] + p.conv[i].K - 1;
      d.max_stage = std::max(d.max_stage, (size_t)B * p.conv[i].Cin * d.Tp[i]);
      if (bf16) d.max_out = std::max(d.max_out, (size_t)B * p.dim[i] * d.Tp[i]);
    }
  }
  return d;
}
// one encoder layer's attention with the gated relative position bias, as the forward and the backward launch it (lse: where the
// row log-sum-exp is kept, or nullptr; the backward adds rel_dgate)
static AttnArgs wavlm_attn_args(const sty_model* m, int T, const float* q, const float* k, const float* v, float* o, const float* tab,
                                const float* gate, float* lse) {
  const int H = m->wav.hidden, NH = m->wav.heads, DH = H / NH;
  AttnArgs at;
  at.q = q, at.k = k, at.v = v, at.o = o;
  at.qbs = at.kbs = at.vbs = at.obs = (size_t)H * T;
  at.T = T, at.H = NH;
  at.scale = 1.0f / sqrtf((float)DH);
  at.lengths = nullptr;
  at.lse = lse;
  at.rel_tab = tab, at.rel_gate = gate;
  at.bf16 = m->wav_bf16 && DH == 64;  // (head dim 16, the small test config: the fp32 kernels in both modes)
  return at;
}
// ---- one strided feature conv of the plan, both directions (wavlm_forward / wavlm_backward and the unit entry
//      sty_wavlm_strided_conv_fwd_bwd run these) ----
// bf16 mode: does this conv over T columns run on a family that reads source 0 as its bf16 twin alone (convp16 / convq)?  Asked
// with a placeholder twin, so that sizing calls and launches decide alike.
static bool wavlm_twin_route(const Run& r, ConvArgs a, ConvKernel* kernel = nullptr, bool offer_twin = true) {
  a.bf16 = r.m->wav_bf16;
  if (a.bf16 && offer_twin) a.x16 = reinterpret_cast<const __bf16*>(sizeof(__bf16));
  const ConvRoute rt = conv1d_route(a);
  if (kernel) *kernel = rt.kernel;
  return a.bf16 && rt.x16_only;
}
// Forward: `below` [B][C] rows of xrs floats with Tin frames (layer 0's output with (ga, gs) set: its norm and GELU on the way;
// gelu_in: a pre-activation) -> y.  fp32 mode, and bf16 mode where no twin family takes the conv: the fp32 view in `stg` and the
// valid conv over its Tp = Tl + K - 1 columns (rows of Tl frames; keep_pre: the pre-activation, else GELU in the epilogue).  bf16
// mode otherwise: the view is written once, as the bf16 operand twin, and the conv runs as a SAME-LENGTH conv over the Tp columns
// (pad 0: the reads past the row's end are the zero padding) -- the twin families take no separate input length -- leaving the
// pre-activation on rows of Tp floats whose last K - 1 columns are partial sums nobody reads (may_pad says the caller's buffers
// and readers allow such rows).  Returns y's row stride; *left_pre: y holds pre-activations.
static int wavlm_strided_fwd(Run& r, const PackedConv& w, const float* below, int xrs, int C, int Tin, int S, int Tl, const float* ga,
                             const float* gs, int gelu_in, bool keep_pre, bool may_pad, float* stg, float* y, bool* left_pre,
                             ConvKernel* kernel = nullptr, bool* twin = nullptr) {
  const int Tp = Tl + w.K - 1;
  ConvArgs a = r.base(w, stg, Tl, y);
  a.pad = 0;
  ConvArgs c = a;
  c.T = Tp;
  if ((Tp == Tl || may_pad) && wavlm_twin_route(r, c, kernel)) {
    r.chk(launch_wavlm_stage_rs(below, ga, gs, r.B, C, Tin, xrs, S, Tp, stg, 1, r.st, gelu_in));
    c.x16 = reinterpret_cast<const __bf16*>(stg);
    r.conv(c);
    *left_pre = true;
    if (twin) *twin = true;
    return Tp;
  }
  if (twin) *twin = false;
  if (xrs != Tin)
    r.chk(launch_wavlm_stage_rs(below, ga, gs, r.B, C, Tin, xrs, S, Tp, stg, 0, r.st, gelu_in));
  else
    r.chk(launch_wavlm_stage(below, ga, gs, r.B, C, Tin, S, Tp, stg, r.st, gelu_in));
  a.Tin = Tp != Tl ? Tp : 0;
  a.act = keep_pre ? ACT_NONE : ACT_GELU;
  if (kernel) wavlm_twin_route(r, a, kernel, false);
  r.conv(a);
  *left_pre = keep_pre;
  return Tl;
}
// Backward: the transposed conv (full correlation: pad K - 1) from the gradient at the conv's pre-activation to the gradient
// of its view, dvw [B][S C][Tp].  cur16 set: that gradient comes as its bf16 twin on rows of Tp columns, zero from Tl on, and the
// conv is a same-length conv over them; else cur is the fp32 tensor on rows of Tl floats.
static void wavlm_strided_dgrad(Run& r, const PackedConv& wd, int K, const float* cur, const __bf16* cur16, int Tl, float* dvw) {
  const int Tp = Tl + K - 1;
  ConvArgs a = r.base(wd, cur, Tp, dvw);
  a.pad = K - 1;
  if (cur16)
    a.x16 = cur16;
  else
    a.Tin = Tp != Tl ? Tl : 0;
  r.conv(a);
}
// ... and whether it takes the twin (asked by whoever produces the gradient, ahead of producing it)
static bool wavlm_dgrad_twin(const Run& r, const PackedConv& wd, int K, int Tl, ConvKernel* kernel = nullptr) {
  Run& rr = const_cast<Run&>(r);
  ConvArgs a = rr.base(wd, nullptr, Tl + K - 1, nullptr);
  a.pad = K - 1;
  if (wavlm_twin_route(r, a, kernel)) return true;
  if (kernel) {  // (the route the fp32 tensor takes)
    a.Tin = K > 1 ? Tl : 0;
    wavlm_twin_route(r, a, kernel, false);
  }
  return false;
}

// WavLMModel.forward(output_hidden_states=True) in eval mode (modeling_wavlm.py): audio16 [B][N16] -> hidden [layers + 1][B][T][H].
// Every activation is channel-major [B][C][T]; wavlm.hip says what each of its kernels does.
// kp (sty_wavlm_fwd_keep): the same launches on the same operands, so the same bits, except that (a) every tensor the backward
// reads gets a buffer of its own at the front of the workspace, (b) a conv followed by GELU leaves its pre-activation and the
// GELU runs behind it (wavlm_stage_kernel / wavlm_gelu_kernel: the conv epilogue's expression on the same fp32 value),
// (c) the attention keeps its row log-sum-exp.
void wavlm_forward(Run& r, int N16, const float* audio, float* hidden, WavlmKeep* kp) {
  sty_model* m = r.m;
  const WavlmPlan& p = m->wav;
  const int B = r.B, nc = p.n_conv, H = p.hidden, NH = p.heads, DH = H / NH;
  if (kp) {
    *kp = WavlmKeep();
    const size_t bc0 = (size_t)B * p.dim[0], nn = (size_t)B * H * wavlm_frames_at(p, N16, nc - 1);
    const size_t nh = nn / H * NH, nf = nn / H * p.layers[0].f1.Cout;
    kp->out0 = r.ws.take<float>(bc0 * wavlm_frames_at(p, N16, 0));
    kp->ga = r.ws.take<float>(bc0), kp->gs = r.ws.take<float>(bc0), kp->gmean = r.ws.take<float>(bc0), kp->grstd = r.ws.take<float>(bc0);
    // (bf16 mode: rows of Tp = T + K - 1 columns where the conv ran over its padded view)
    for (int i = 1; i < nc; ++i)
      kp->pre[i] = r.ws.take<float>((size_t)B * p.dim[i] * (wavlm_frames_at(p, N16, i) + (m->wav_bf16 ? p.conv[i].K - 1 : 0)));
    kp->feat = r.ws.take<float>(nn / H * p.dim[nc - 1]);
    kp->pre_pos = r.ws.take<float>(nn), kp->xa_enc = r.ws.take<float>(nn);
    kp->tab = r.ws.take<float>((size_t)NH * (2 * (nn / H / B) - 1));
    for (size_t l = 0; l <= p.layers.size(); ++l) kp->x.push_back(r.ws.take<float>(nn));
    for (size_t l = 0; l < p.layers.size(); ++l) {
      WavlmKeepLayer y;
      y.q = r.ws.take<float>(nn), y.k = r.ws.take<float>(nn), y.v = r.ws.take<float>(nn), y.o = r.ws.take<float>(nn);
      y.a1 = r.ws.take<float>(nn), y.a2 = r.ws.take<float>(nn);
      y.lse = r.ws.take<float>(nh), y.gate = r.ws.take<float>(nh);
      y.pre = r.ws.take<float>(nf);
      kp->layers.push_back(y);
    }
    kp->saved_end = r.ws.off;
  }
  const WavlmDims dm = wavlm_dims(p, B, N16, m->wav_bf16);
  const int* Tl = dm.Tl;
  const int T = Tl[nc - 1], Cl = p.dim[nc - 1];
  const size_t max_out = dm.max_out, max_stage = std::max(dm.max_stage, (size_t)B * Cl * T);
  const size_t n = (size_t)B * H * T;
  float* x = r.ws.take<float>(n);
  {  // ---- feature encoder and projection ----
    Run::Scope sc(r);
    float* out = r.ws.take<float>(max_out);
    float* stg = r.ws.take<float>(max_stage);
    const int nt = wavlm_conv0_ntiles(Tl[0]);
    double* part = r.ws.take<double>((size_t)B * p.dim[0] * nt * 2);
    float* ga = r.ws.take<float>((size_t)B * p.dim[0]);
    float* gs = r.ws.take<float>((size_t)B * p.dim[0]);
    if (kp) ga = kp->ga, gs = kp->gs;
    if (r.live()) {
      r.chk(launch_wavlm_conv0(audio, p.conv0_w, B, N16, p.dim[0], p.kern[0], p.stride[0], Tl[0], kp ? kp->out0 : out, part, r.st));
      r.chk(launch_wavlm_gn_finalize(part, nt, p.gn_w, p.gn_b, B * p.dim[0], p.dim[0], Tl[0], 1e-5f, ga, gs, r.st,
                                     kp ? kp->gmean : nullptr, kp ? kp->grstd : nullptr));
    }
    int xrs = Tl[0];        // row stride of the layer below's output
    bool pre_below = false;  // ... which holds pre-activations: the GELU runs in the staging pass
    for (int i = 1; i < nc && r.live(); ++i) {
      const float* below = !kp ? out : (i == 1 ? kp->out0 : kp->pre[i - 1]);
      // (the last conv's output goes to an element-wise pass and a LayerNorm over dense rows: no padded rows there)
      xrs = wavlm_strided_fwd(r, p.conv[i], below, xrs, p.dim[i - 1], Tl[i - 1], p.stride[i], Tl[i], i == 1 ? ga : nullptr, gs,
                              i > 1 && pre_below, kp != nullptr, i < nc - 1, stg, kp ? kp->pre[i] : out, &pre_below);
      if (kp) kp->prs[i] = xrs;
    }
    if (r.live()) {
      if (kp)
        r.chk(launch_wavlm_gelu(kp->pre[nc - 1], nullptr, (size_t)B * Cl * T, kp->feat, r.st));
      float *ln_in = kp ? kp->feat : out, *ln_out = stg;
      if (!kp && pre_below) {  // (bf16 mode: the twin families leave the pre-activation; the view in stg has been consumed)
        r.chk(launch_wavlm_gelu(out, nullptr, (size_t)B * Cl * T, stg, r.st));
        ln_in = stg, ln_out = out;
      }
      r.chk(launch_chan_layernorm(ln_in, ln_out, B, Cl, T, p.ln_eps, 0, p.fp_ln_w, p.fp_ln_b, nullptr, 0, nullptr, r.st));
      r.conv(r.base(p.proj, ln_out, T, x));
    }
  }
  // ---- encoder ----
  const int G = p.pos_groups, Cg = H / G, FF = p.layers[0].f1.Cout;
  float* xa = r.ws.take<float>(n);
  float* xb = r.ws.take<float>(n);
  float* q = r.ws.take<float>(n);
  float* k = r.ws.take<float>(n);
  float* v = r.ws.take<float>(n);
  float* o = r.ws.take<float>(n);
  float* big = r.ws.take<float>((size_t)B * FF * T);
  float* gate = r.ws.take<float>((size_t)B * NH * T);
  float* tab = r.ws.take<float>((size_t)NH * (2 * T - 1));
  if (kp) tab = kp->tab;
  r.note_peak();
  if (!r.live()) return;
  {  // x + GELU(pos_conv(x)) in the group-major layout (q, k as scratch), then the LayerNorm
    r.chk(launch_wavlm_group_perm(x, B, G, Cg, T, 1, q, r.st));
    for (int g = 0; g < G && r.live(); ++g) {
      const size_t off = (size_t)g * B * Cg * T;
      ConvArgs a = r.base(p.pos[g], q + off, T, (kp ? kp->pre_pos : k) + off);
      a.pad = p.pos_k / 2;
      if (!kp) {
        a.act = ACT_GELU;
        a.residual = q + off;
      }
      r.conv(a);
    }
    if (!r.live()) return;
    if (kp) r.chk(launch_wavlm_gelu(kp->pre_pos, q, n, k, r.st));
    float* ln_in = kp ? kp->xa_enc : xa;
    if (kp) x = kp->x[0];
    r.chk(launch_wavlm_group_perm(k, B, G, Cg, T, 0, ln_in, r.st));
    r.chk(launch_chan_layernorm(ln_in, x, B, H, T, p.ln_eps, 0, p.enc_ln_w, p.enc_ln_b, nullptr, 0, nullptr, r.st));
    r.chk(launch_wavlm_transpose_out(x, B, H, T, hidden, r.st));
  }
  {  // the position bias table of this frame count, shared by every layer.  The bucket table is one per model: sized for the
     // largest frame count seen (at least 2 048 frames, 41 s), so a validation split of many lengths allocates once
    if (T > m->wav_bucket_T) {
      const int Tm = std::max(T, 2048);
      std::vector<int32_t> host(2 * Tm - 1);
      wavlm_rel_buckets(Tm, p.num_buckets, p.max_distance, host.data());
      int32_t* dev = nullptr;
      if (hipMalloc((void**)&dev, host.size() * sizeof(int32_t)) != hipSuccess ||
          hipMemcpy(dev, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {  // (pageable: complete on return)
        if (dev) (void)hipFree(dev);
        set_error("wavlm: the bucket table of %d frames could not be placed on the device", Tm);
        r.rc = STY_EHIP;
        return;
      }
      if (m->wav_bucket_dev) (void)hipFree(m->wav_bucket_dev);  // (hipFree waits for the launches that still read it)
      m->wav_bucket_dev = dev;
      m->wav_bucket_T = Tm;
    }
    r.chk(launch_wavlm_rel_table(p.rel_embed, m->wav_bucket_dev + (m->wav_bucket_T - T), NH, T, tab, r.st));
  }
  for (size_t l = 0; l < p.layers.size() && r.live(); ++l) {
    const WavlmLayer& y = p.layers[l];
    float* a2 = xa;
    if (kp) {  // this layer's kept tensors in the scratch buffers' places; x = its input, xo its output
      const WavlmKeepLayer& kl = kp->layers[l];
      q = kl.q, k = kl.k, v = kl.v, o = kl.o, gate = kl.gate, xa = kl.a1, a2 = kl.a2;
      x = kp->x[l];
    }
    float* xo = kp ? kp->x[l + 1] : x;
    r.chk(launch_wavlm_gate(x, y.gate_w, y.gate_b, y.gate_c, B, NH, DH, T, gate, r.st));
    r.conv(r.base(y.q, x, T, q));
    r.conv(r.base(y.k, x, T, k));
    r.conv(r.base(y.v, x, T, v));
    if (!r.live()) return;
    const AttnArgs at = wavlm_attn_args(m, T, q, k, v, o, tab, gate, kp ? kp->layers[l].lse : nullptr);
    r.chk(launch_attention(at, B, DH, r.st));
    ConvArgs ao = r.base(y.o, o, T, xa);
    ao.residual = x;
    r.conv(ao);
    if (!r.live()) return;
    r.chk(launch_chan_layernorm(xa, xb, B, H, T, p.ln_eps, 0, y.ln1_w, y.ln1_b, nullptr, 0, nullptr, r.st));
    ConvArgs f1 = r.base(y.f1, xb, T, kp ? kp->layers[l].pre : big);
    f1.act = kp ? ACT_NONE : ACT_GELU;
    r.conv(f1);
    if (kp && r.live()) r.chk(launch_wavlm_gelu(kp->layers[l].pre, nullptr, (size_t)B * FF * T, big, r.st));
    ConvArgs f2 = r.base(y.f2, big, T, a2);
    f2.residual = xb;
    r.conv(f2);
    if (!r.live()) return;
    r.chk(launch_chan_layernorm(a2, xo, B, H, T, p.ln_eps, 0, y.ln2_w, y.ln2_b, nullptr, 0, nullptr, r.st));
    r.chk(launch_wavlm_transpose_out(xo, B, H, T, hidden + (l + 1) * n, r.st));
  }
}

// The backward of wavlm_forward to the wave: d_hidden [layers + 1][B][T][H] -> d_audio [B][N16] (and the optional tap d_enc_in
// [B][H][T] in front of the positional conv), on the tensors a keep-mode forward left.  Input gradients only (the network is
// frozen); the steps cite modeling_wavlm.py as the forward does.  Scratch starts behind the kept tensors.
void wavlm_backward(Run& r, int N16, const WavlmKeep& kp, const float* d_hidden, float* d_audio, float* d_enc_in) {
  sty_model* m = r.m;
  const WavlmPlan& p = m->wav;
  const int B = r.B, nc = p.n_conv, H = p.hidden, NH = p.heads, DH = H / NH;
  const WavlmDims dm = wavlm_dims(p, B, N16, m->wav_bf16);
  const int *Tl = dm.Tl, *Tp = dm.Tp;
  const size_t max_out = dm.max_out, max_stage = dm.max_stage;
  const int T = Tl[nc - 1], Cl = p.dim[nc - 1], G = p.pos_groups, Cg = H / G, FF = p.layers[0].f1.Cout;
  const int L = (int)p.layers.size();
  const size_t n = (size_t)B * H * T;
  r.ws.off = kp.saved_end;
  float* g = r.ws.take<float>(n);   // gradient at the current layer's output
  float* t1 = r.ws.take<float>(n);
  float* t2 = r.ws.take<float>(n);
  float* dq = r.ws.take<float>(n);
  float* dk = r.ws.take<float>(n);
  float* dv = r.ws.take<float>(n);
  float* dbig = r.ws.take<float>((size_t)B * FF * T);
  float* dpre = r.ws.take<float>((size_t)B * FF * T);
  float* dgate = r.ws.take<float>((size_t)B * NH * T);
  float* aws = r.ws.take<float>(attention_bwd_ws_floats(B, NH, T));
  float* mu = r.ws.take<float>((size_t)B * std::max(T, 64));
  float* rt = r.ws.take<float>((size_t)B * std::max(T, 64));
  float* fa = r.ws.take<float>(max_out);
  float* fb = r.ws.take<float>(max_out);
  float* dvw = r.ws.take<float>(max_stage);
  const int gnt = wavlm_gn_bwd_ntiles(Tl[0]);
  double* gpart = r.ws.take<double>((size_t)B * p.dim[0] * gnt * 2);
  float* gcoef = r.ws.take<float>((size_t)B * p.dim[0] * 2);
  r.note_peak();
  if (!r.live()) return;
  static const PackedConv none;
  auto D = [&](const PackedConv& w) -> const PackedConv& {  // the input-gradient weights of a conv of the dgrad table
    auto it = m->dgrad.find(w.wp);
    if (it != m->dgrad.end()) return it->second;
    if (r.rc == STY_OK) {
      set_error("wavlm_backward: a conv without input-gradient weights (the model was not finalized for the kind)");
      r.rc = STY_ESTATE;
    }
    return none;
  };
  auto ln_bwd = [&](const float* x, const float* dy, int C, const float* w, float* dx) {  // input gradient alone
    r.chk(launch_chan_ln_bwd(x, dy, nullptr, B, C, T, p.ln_eps, 0, w, nullptr, 0, nullptr, dx, 0, mu, rt, nullptr, nullptr, nullptr, r.st));
  };
  auto zero = [&](float* x, size_t cnt) {
    if (r.live() && hipMemsetAsync(x, 0, cnt * sizeof(float), r.st) != hipSuccess) {
      set_error("wavlm_backward: hipMemsetAsync failed");
      r.rc = STY_EHIP;
    }
  };
  // (1) cotangent of the last hidden state; every other one is added where its layer's gradient is complete
  r.chk(launch_wavlm_intake(d_hidden + (size_t)L * n, B, H, T, 0, g, r.st));
  // (2) encoder layers, post-norm: x_out = LN2(xb + f2(GELU(f1(xb)))), xb = LN1(x + out_proj(attn(x)))
  for (int l = L - 1; l >= 0 && r.live(); --l) {
    const WavlmLayer& y = p.layers[l];
    const WavlmKeepLayer& kl = kp.layers[l];
    ln_bwd(kl.a2, g, H, y.ln2_w, t1);                      // t1 = d (xb + f2(..))
    r.conv(r.base(D(y.f2), t1, T, dbig));
    if (!r.live()) return;
    r.chk(launch_act_bwd(ACT_GELU, kl.pre, dbig, nullptr, B, FF, T, dpre, 0, nullptr, r.st));
    ConvArgs f1 = r.base(D(y.f1), dpre, T, t2);
    f1.residual = t1;
    r.conv(f1);                                            // t2 = d xb
    if (!r.live()) return;
    ln_bwd(kl.a1, t2, H, y.ln1_w, t1);                     // t1 = d (x + out_proj(attn))
    r.conv(r.base(D(y.o), t1, T, t2));                     // t2 = d attn output
    zero(dq, n), zero(dk, n), zero(dv, n);                 // (the attention backward accumulates)
    if (!r.live()) return;
    // (3) attention with the gated relative position bias: dq, dk, dv and d gate, no [B H][T][T] bias tensor
    AttnArgs at = wavlm_attn_args(m, T, kl.q, kl.k, kl.v, kl.o, kp.tab, kl.gate, kl.lse);
    at.rel_dgate = dgate;
    r.chk(launch_attention_bwd(at, t2, dq, dk, dv, at.qbs, at.kbs, at.vbs, at.obs, B, DH, aws, r.st));
    // dx = residual + q / k / v projections' input gradients (+ the gate path, + this layer input's own cotangent)
    ConvArgs cq = r.base(D(y.q), dq, T, t2);
    cq.residual = t1;
    r.conv(cq);
    ConvArgs ck = r.base(D(y.k), dk, T, t1);
    ck.residual = t2;
    r.conv(ck);
    ConvArgs cv = r.base(D(y.v), dv, T, g);
    cv.residual = t1;
    r.conv(cv);
    if (!r.live()) return;
    // (4) gate backward into the head slices
    r.chk(launch_wavlm_gate_bwd(kp.x[l], y.gate_w, y.gate_b, y.gate_c, dgate, B, NH, DH, T, g, r.st));
    r.chk(launch_wavlm_intake(d_hidden + (size_t)l * n, B, H, T, 1, g, r.st));
  }
  if (!r.live()) return;
  // (5) encoder LayerNorm, then x + GELU(pos_conv(x)): GELU' in front of the grouped dgrad, the residual around it.  The forward
  // pads k / 2 and never computes the even kernel's last frame, so the flipped taps are padded k / 2 - 1.
  ln_bwd(kp.xa_enc, g, H, p.enc_ln_w, t1);
  r.chk(launch_wavlm_group_perm(t1, B, G, Cg, T, 1, t2, r.st));
  r.chk(launch_act_bwd(ACT_GELU, kp.pre_pos, t2, nullptr, G * B, Cg, T, dq, 0, nullptr, r.st));
  for (int gi = 0; gi < G && r.live(); ++gi) {
    const size_t off = (size_t)gi * B * Cg * T;
    ConvArgs a = r.base(p.pos_d[gi], dq + off, T, dk + off);
    a.pad = p.pos_k - 1 - p.pos_k / 2;
    a.residual = t2 + off;
    r.conv(a);
  }
  if (!r.live()) return;
  r.chk(launch_wavlm_group_perm(dk, B, G, Cg, T, 0, t1, r.st));  // t1 = gradient at the feature projection's output
  if (d_enc_in && hipMemcpyAsync(d_enc_in, t1, n * sizeof(float), hipMemcpyDeviceToDevice, r.st) != hipSuccess) {
    set_error("wavlm_backward: the copy of the tap failed");
    r.rc = STY_EHIP;
    return;
  }
  // (6) feature projection: 1x1 dgrad, LayerNorm, then the GELU' of the last feature conv
  r.conv(r.base(D(p.proj), t1, T, fa));
  if (!r.live()) return;
  ln_bwd(kp.feat, fa, Cl, p.fp_ln_w, fb);
  r.chk(launch_act_bwd(ACT_GELU, kp.pre[nc - 1], fb, nullptr, B, Cl, T, fa, 0, nullptr, r.st));
  // (7) strided feature convs: the stride-1 conv over the s-frames-at-a-time view, transposed (full correlation: pad K - 1), then
  // the un-staging permutation with the GELU' of the layer below; (8) behind layer 0 the GroupNorm backward takes its place
  float *cur = fa, *other = fb;
  // bf16 mode: a layer whose transposed conv runs on a twin family gets its gradient from the un-staging above it as the bf16
  // twin on zero-padded rows (the top layer's comes from the GELU' pass in fp32)
  bool cur_twin = false;
  for (int i = nc - 1; i >= 1 && r.live(); --i) {
    wavlm_strided_dgrad(r, p.conv_d[i], p.conv[i].K, cur, cur_twin ? reinterpret_cast<const __bf16*>(cur) : nullptr, Tl[i], dvw);
    if (!r.live()) return;
    if (i > 1 && m->wav_bf16) {
      cur_twin = wavlm_dgrad_twin(r, p.conv_d[i - 1], p.conv[i - 1].K, Tl[i - 1]);
      r.chk(launch_wavlm_unstage_rs(dvw, kp.pre[i - 1], B, p.dim[i - 1], Tl[i - 1], kp.prs[i - 1], p.stride[i], Tp[i],
                                    cur_twin ? Tp[i - 1] : Tl[i - 1], other, cur_twin, r.st));
    } else if (i > 1)
      r.chk(launch_wavlm_unstage(dvw, kp.pre[i - 1], B, p.dim[i - 1], Tl[i - 1], p.stride[i], Tp[i], other, r.st));
    else
      r.chk(launch_wavlm_gn_bwd(kp.out0, dvw, kp.ga, kp.gs, kp.gmean, kp.grstd, B, p.dim[0], Tl[0], p.stride[1], Tp[1], gpart, gcoef, other,
                                r.st));
    std::swap(cur, other);
  }
  if (!r.live()) return;
  // (9) layer 0 transposed: the whole d_audio, the tail no frame reads included (zero)
  r.chk(launch_wavlm_conv0_bwd(cur, p.conv0_w, B, N16, p.dim[0], p.kern[0], p.stride[0], Tl[0], d_audio, r.st));
}

}  // namespace sty

using namespace sty;

extern "C" {

// ---- slm loss value: resampler, WavLM forward, mean |a - b| (train/losses.py:376-394; wavlm.hip) ----
static int gcd_(int a, int b) { return b ? gcd_(b, a % b) : a; }
static bool resample_rates_ok(int orig, int nw) { return orig > 0 && nw > 0 && orig / gcd_(orig, nw) <= 1024 && nw / gcd_(orig, nw) <= 1024; }
int sty_wavlm_set_config(sty_model* m, int n_conv, const int* conv_stride, int max_bucket_distance, float layer_norm_eps) {
  if (!m || m->kind != "wavlm" || !conv_stride || n_conv < 2 || n_conv > WAVLM_MAX_CONV || max_bucket_distance < 2 || !(layer_norm_eps > 0.f)) {
    set_error("sty_wavlm_set_config: bad argument (kind 'wavlm', 2 to %d conv layers)", WAVLM_MAX_CONV);
    return STY_EINVAL;
  }
  for (int i = 0; i < n_conv; ++i)
    if (conv_stride[i] < 1 || conv_stride[i] > 16) {
      set_error("sty_wavlm_set_config: conv stride %d of layer %d (1 to 16 are built)", conv_stride[i], i);
      return STY_EINVAL;
    }
  WavlmPlan& p = m->wav;
  p.n_conv = n_conv;
  for (int i = 0; i < n_conv; ++i) p.stride[i] = conv_stride[i];
  p.max_distance = max_bucket_distance;
  p.ln_eps = layer_norm_eps;
  m->finalized = false;
  return STY_OK;
}
// The kind's own operand mode (sty_model_set_train_opts(compute_bf16) keeps refusing it, as every inference-only kind's does).
// Nothing is re-packed here: the bf16 fragments of a packed weight are made at its first bf16 launch and live beside the fp32
// pack for the life of the arena (convp16.hip), so switching back and forth costs nothing after the first call of each mode.
int sty_wavlm_set_compute(sty_model* m, int bf16) {
  if (!m) {
    set_error("sty_wavlm_set_compute: null model");
    return STY_EINVAL;
  }
  if (m->kind != "wavlm") {
    set_error("sty_wavlm_set_compute: model kind '%s' (the operand mode of kind 'wavlm' alone is set here)", m->kind.c_str());
    return STY_EINVAL;
  }
  if (bf16 != 0 && bf16 != 1) {
    set_error("sty_wavlm_set_compute: mode %d (0 = fp32 operands, 1 = bf16 operands)", bf16);
    return STY_EINVAL;
  }
  m->wav_bf16 = bf16;
  return STY_OK;
}
int sty_slm_resample_len(int N, int orig, int new_rate) {
  if (N <= 0 || !resample_rates_ok(orig, new_rate)) return -1;
  const int g = gcd_(orig, new_rate);
  return (int)(((long long)N * (new_rate / g) + orig / g - 1) / (orig / g));
}
int sty_slm_resample_kernel_host(int orig, int new_rate, float* out) {
  if (!resample_rates_ok(orig, new_rate)) return -1;
  const int g = gcd_(orig, new_rate), o = orig / g, n = new_rate / g;
  if (out) build_resample_kernel(o, n, 6.0, out);
  return n * (2 * resample_width(o, n, 6.0) + o);
}
// the forward (d_accumulate < 0: x = audio [B][N] -> y = out [B][M]) and its adjoint (y = d_out -> x = d_audio, written or added to)
static int slm_resample_run(const char* who, int B, int N, int orig, int new_rate, const float* src, float* dst, int d_accumulate,
                            void* stream) {
  if (!src || !dst || B <= 0 || N <= 0 || !resample_rates_ok(orig, new_rate)) {
    set_error("%s: bad argument", who);
    return STY_EINVAL;
  }
  const int g = gcd_(orig, new_rate), o = orig / g, n = new_rate / g, width = resample_width(o, n, 6.0);
  const size_t floats = (size_t)n * (2 * width + o);
  if (floats * sizeof(float) > 48 * 1024) {
    set_error("%s: %d -> %d needs a table of %zu taps (more than the kernel keeps)", who, orig, new_rate, floats);
    return STY_EINVAL;
  }
  // device tables by (device, reduced rate pair), built on first use under a lock; a table is cached only once it is filled
  static std::mutex mu;
  static std::map<std::tuple<int, int, int>, float*> tables;
  int device = 0;
  STY_HIP(hipGetDevice(&device));
  float* dev = nullptr;
  {
    std::lock_guard<std::mutex> lock(mu);
    float*& slot = tables[std::make_tuple(device, o, n)];
    if (!slot) {
      std::vector<float> host(floats);
      build_resample_kernel(o, n, 6.0, host.data());
      float* fresh = nullptr;
      STY_HIP(hipMalloc((void**)&fresh, floats * sizeof(float)));
      const hipError_t e = hipMemcpy(fresh, host.data(), floats * sizeof(float), hipMemcpyHostToDevice);  // (pageable: complete on return)
      if (e != hipSuccess) {
        (void)hipFree(fresh);
        return hip_fail(e, "hipMemcpy of the resample table");
      }
      slot = fresh;
    }
    dev = slot;
  }
  const int M = sty_slm_resample_len(N, orig, new_rate);
  if (d_accumulate >= 0) return launch_resample_fir_bwd(src, dev, B, N, M, o, n, width, d_accumulate, dst, S(stream));
  return launch_resample_fir(src, dev, B, N, M, o, n, width, dst, S(stream));
}
int sty_slm_resample_fwd(int B, int N, int orig, int new_rate, const float* audio, float* out, void* stream) {
  return slm_resample_run("sty_slm_resample_fwd", B, N, orig, new_rate, audio, out, -1, stream);
}
int sty_slm_resample_bwd(int B, int N, int orig, int new_rate, const float* d_out, float* d_audio, int accumulate, void* stream) {
  return slm_resample_run("sty_slm_resample_bwd", B, N, orig, new_rate, d_out, d_audio, accumulate ? 1 : 0, stream);
}
int sty_wavlm_frames(const sty_model* m, int N16, int* T) {
  int rc = entry_ready(m, "wavlm", nullptr, !T || N16 <= 0, "sty_wavlm_frames: bad argument");
  if (rc) return rc;
  *T = wavlm_frames_at(m->wav, N16, m->wav.n_conv - 1);
  if (*T < 1) {
    set_error("wavlm: %d samples leave no frame behind the feature encoder", N16);
    return STY_ESHAPE;
  }
  return STY_OK;
}
static int wavlm_run(sty_model* m, int B, int N16, const float* audio, float* hidden, void* ws, size_t ws_bytes, void* stream,
                     size_t* need) {
  Run r(m, B, ws, ws_bytes, stream);
  wavlm_forward(r, N16, audio, hidden);
  return r.finish(need, ws, ws_bytes);
}
int sty_wavlm_workspace_bytes(const sty_model* m, int B, int N16, size_t* bytes) {
  int T = 0, rc = sty_wavlm_frames(m, N16, &T);
  if (rc) return rc;
  if (!bytes || B <= 0) {
    set_error("sty_wavlm_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  return wavlm_run(const_cast<sty_model*>(m), B, N16, nullptr, nullptr, nullptr, 0, nullptr, bytes);
}
int sty_wavlm_fwd(sty_model* m, int B, int N16, const float* audio16, float* hidden, void* workspace, size_t ws_bytes, void* stream) {
  int T = 0, rc = sty_wavlm_frames(m, N16, &T);
  if (rc) return rc;
  if (!audio16 || !hidden || !workspace || B <= 0) {
    set_error("sty_wavlm_fwd: bad argument");
    return STY_EINVAL;
  }
  if ((rc = ensure_prepared(m, stream))) return rc;
  return wavlm_run(m, B, N16, audio16, hidden, workspace, ws_bytes, stream, nullptr);
}
// ---- the backward to the wave: forward that keeps, then sty_wavlm_bwd on the same workspace ----
static int wavlm_grad_need(sty_model* m, int B, int N16, size_t* need) {
  Run r(m, B, nullptr, 0, nullptr);
  WavlmKeep kp;
  wavlm_forward(r, N16, nullptr, nullptr, &kp);
  wavlm_backward(r, N16, kp, nullptr, nullptr, nullptr);
  return r.finish(need, nullptr, 0);
}
int sty_wavlm_grad_workspace_bytes(const sty_model* m, int B, int N16, size_t* bytes) {
  int T = 0, rc = sty_wavlm_frames(m, N16, &T);
  if (rc) return rc;
  if (!bytes || B <= 0) {
    set_error("sty_wavlm_grad_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  return wavlm_grad_need(const_cast<sty_model*>(m), B, N16, bytes);
}
int sty_wavlm_fwd_keep(sty_model* m, int B, int N16, const float* audio16, float* hidden, void* workspace, size_t ws_bytes, void* stream) {
  int T = 0, rc = sty_wavlm_frames(m, N16, &T);
  if (rc) return rc;
  if (!audio16 || !hidden || !workspace || B <= 0) {
    set_error("sty_wavlm_fwd_keep: bad argument");
    return STY_EINVAL;
  }
  m->wav_keep.valid = false;
  size_t need = 0;
  if ((rc = wavlm_grad_need(m, B, N16, &need))) return rc;
  if (ws_bytes < need) {  // refused on the host: nothing is launched into a workspace that cannot hold the kept tensors
    set_error("sty_wavlm_fwd_keep: workspace too small: need %zu bytes, have %zu", need, ws_bytes);
    return STY_ENOMEM;
  }
  if ((rc = ensure_prepared(m, stream))) return rc;
  Run r(m, B, workspace, ws_bytes, stream);
  wavlm_forward(r, N16, audio16, hidden, &m->wav_keep);
  rc = r.finish(nullptr, workspace, ws_bytes);
  if (rc == STY_OK) {
    m->wav_keep.valid = true;
    m->wav_keep.B = B, m->wav_keep.N16 = N16, m->wav_keep.ws = workspace;
    m->wav_keep.bf16 = m->wav_bf16;
  }
  return rc;
}
int sty_wavlm_bwd(sty_model* m, int B, int N16, const float* d_hidden, float* d_audio16, float* d_enc_in, void* workspace,
                  size_t ws_bytes, void* stream) {
  int rc = entry_ready(m, "wavlm", nullptr, !d_hidden || !d_audio16 || !workspace || B <= 0 || N16 <= 0, "sty_wavlm_bwd: bad argument");
  if (rc) return rc;
  WavlmKeep& kp = m->wav_keep;
  if (!kp.valid) {
    set_error("sty_wavlm_bwd: no sty_wavlm_fwd_keep call precedes it (a backward consumes its forward's workspace)");
    return STY_ESTATE;
  }
  if (kp.B != B || kp.N16 != N16 || kp.ws != workspace) {
    set_error("sty_wavlm_bwd: (B, N16) = (%d, %d) on this workspace, but the forward kept (%d, %d)%s", B, N16, kp.B, kp.N16,
              kp.ws != workspace ? " in another workspace" : "");
    return STY_ESHAPE;
  }
  if (kp.bf16 != m->wav_bf16) {
    set_error("sty_wavlm_bwd: the model runs %s operands now, but the forward kept in %s mode (sty_wavlm_set_compute between the two)",
              m->wav_bf16 ? "bf16" : "fp32", kp.bf16 ? "bf16" : "fp32");
    return STY_ESTATE;
  }
  size_t need = 0;
  if ((rc = wavlm_grad_need(m, B, N16, &need))) return rc;
  if (ws_bytes < need) {
    set_error("sty_wavlm_bwd: workspace too small: need %zu bytes, have %zu", need, ws_bytes);
    return STY_ENOMEM;
  }
  kp.valid = false;  // consumed: the scratch of this call overwrites nothing kept, but a second backward is not the contract
  Run r(m, B, workspace, ws_bytes, stream);
  wavlm_backward(r, N16, kp, d_hidden, d_audio16, d_enc_in);
  return r.finish(nullptr, workspace, ws_bytes);
}
// ---- one strided feature conv alone, forward and input gradient: the stage + conv / dgrad + un-stage pair of the plan ----
// x [B][Cin][Nin] is a pre-activation (what the layer below leaves in keep mode): y = conv1d(GELU(x), w, stride s) [B][Cout][T],
// T = (Nin - k) / s + 1, no activation; dx = GELU'(x) * (the transposed conv of gy) [B][Cin][Nin], zero where no frame reads.
static int wavlm_strided_unit(int B, int Cin, int Cout, int k, int s, int Nin, const float* x, const float* w, int compute_bf16,
                              float* y, const float* gy, float* dx, float* view, void* view16, int* routes, void* ws, size_t ws_bytes,
                              void* stream, size_t* need) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || k < 1 || s < 1 || s > 16 || Nin < k || (compute_bf16 != 0 && compute_bf16 != 1)) {
    set_error("sty_wavlm_strided_conv: bad argument (k >= 1, stride 1 to 16, Nin >= k, compute_bf16 0 or 1)");
    return STY_EINVAL;
  }
  sty_model tmp;
  tmp.kind = "wavlm";
  tmp.wav_bf16 = compute_bf16;
  Run r(&tmp, B, ws, ws_bytes, stream);
  const int Tl = (Nin - k) / s + 1;
  PackedConv pc;
  pc.Cin = s * Cin, pc.Cout = Cout, pc.K = cdiv(k, s);
  pc.CinP = (int)align_up(pc.Cin, CI_CHUNK), pc.CoutP = (int)align_up(Cout, 32);
  const int Tp = Tl + pc.K - 1;
  const size_t wn = (size_t)pc.K * pc.CinP * pc.CoutP, nv = (size_t)B * pc.Cin * Tp, ny = (size_t)B * Cout * Tp;
  float* wp = r.ws.take<float>(wn);
  float* wd = r.ws.take<float>(wn);
  float* stg = r.ws.take<float>(nv);
  float* ybuf = r.ws.take<float>(ny);
  float* gpad = r.ws.take<float>(ny);
  __bf16* g16 = r.ws.take<__bf16>(ny);
  float* dvw = r.ws.take<float>(nv);
  r.note_peak();
  if (!r.live()) return r.finish(need, ws, ws_bytes);
  pc.wp = wp;
  PackedConv pd;
  pd.Cin = pc.Cout, pd.CinP = pc.CoutP, pd.Cout = pc.Cin, pd.CoutP = pc.CinP, pd.K = pc.K, pd.wp = wd;
  STY_HIP(hipMemsetAsync(wp, 0, wn * sizeof(float), r.st));
  WavlmPackJob j;
  j.w = w, j.wp = wp;
  j.Cout = Cout, j.Cin = Cin, j.K = k, j.s = s, j.CinP = pc.CinP, j.CoutP = pc.CoutP;
  r.chk(launch_wavlm_pack(j, r.st));
  r.chk(launch_pack_dgrad(wp, pc.K, pc.CinP, pc.CoutP, wd, r.st));
  if (!r.live()) return r.rc;
  ConvKernel kf = CONV_TILED, kd = CONV_TILED;
  bool left_pre = false, ftwin = false;
  const int yrs = wavlm_strided_fwd(r, pc, x, Nin, Cin, Nin, s, Tl, nullptr, nullptr, 1, true, true, stg, ybuf, &left_pre, &kf, &ftwin);
  if (!r.live()) return r.rc;
  STY_HIP(hipMemcpy2DAsync(y, (size_t)Tl * sizeof(float), ybuf, (size_t)yrs * sizeof(float), (size_t)Tl * sizeof(float), (size_t)B * Cout,
                           hipMemcpyDeviceToDevice, r.st));
  if (view16) {
    if (!ftwin) {
      set_error("sty_wavlm_strided_conv: the bf16 twin of the view was asked for, but this conv does not run on a twin family");
      return STY_EINVAL;
    }
    STY_HIP(hipMemcpyAsync(view16, stg, nv * sizeof(__bf16), hipMemcpyDeviceToDevice, r.st));
  }
  // the gradient as the plan's producers leave it: the twin on zero-padded rows where the transposed conv takes it
  const bool dtwin = wavlm_dgrad_twin(r, pd, pc.K, Tl, &kd);
  if (dtwin) {
    STY_HIP(hipMemsetAsync(gpad, 0, ny * sizeof(float), r.st));
    STY_HIP(hipMemcpy2DAsync(gpad, (size_t)Tp * sizeof(float), gy, (size_t)Tl * sizeof(float), (size_t)Tl * sizeof(float), (size_t)B * Cout,
                             hipMemcpyDeviceToDevice, r.st));
    r.chk(launch_twin_cast(gpad, nullptr, PRO_NONE, B, Cout, Tp, g16, r.st));
  }
  wavlm_strided_dgrad(r, pd, pc.K, gy, dtwin ? g16 : nullptr, Tl, dvw);
  if (!r.live()) return r.rc;
  if (compute_bf16)
    r.chk(launch_wavlm_unstage_rs(dvw, x, B, Cin, Nin, Nin, s, Tp, Nin, dx, 0, r.st));
  else
    r.chk(launch_wavlm_unstage(dvw, x, B, Cin, Nin, s, Tp, dx, r.st));
  if (view && r.live()) r.chk(launch_wavlm_stage(x, nullptr, nullptr, B, Cin, Nin, s, Tp, view, r.st, 1));  // (the fp32 mode's view)
  if (routes) routes[0] = (int)kf, routes[1] = (int)kd, routes[2] = ftwin, routes[3] = dtwin;
  return r.rc;
}
int sty_wavlm_strided_conv_workspace_bytes(int B, int Cin, int Cout, int k, int s, int Nin, size_t* bytes) {
  if (!bytes) {
    set_error("sty_wavlm_strided_conv_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  return wavlm_strided_unit(B, Cin, Cout, k, s, Nin, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                            nullptr, bytes);
}
int sty_wavlm_strided_conv_fwd_bwd(int B, int Cin, int Cout, int k, int s, int Nin, const float* x, const float* w, int compute_bf16,
                                   float* y, const float* gy, float* dx, float* view, void* view16, int* routes, void* workspace,
                                   size_t ws_bytes, void* stream) {
  if (!x || !w || !y || !gy || !dx || !workspace) {
    set_error("sty_wavlm_strided_conv_fwd_bwd: bad argument");
    return STY_EINVAL;
  }
  size_t need = 0;
  int rc = sty_wavlm_strided_conv_workspace_bytes(B, Cin, Cout, k, s, Nin, &need);
  if (rc) return rc;
  if (ws_bytes < need) {
    set_error("sty_wavlm_strided_conv_fwd_bwd: workspace too small: need %zu bytes, have %zu", need, ws_bytes);
    return STY_ENOMEM;
  }
  return wavlm_strided_unit(B, Cin, Cout, k, s, Nin, x, w, compute_bf16, y, gy, dx, view, view16, routes, workspace, ws_bytes, stream,
                            nullptr);
}
int sty_wavlm_rel_buckets_host(int T, int num_buckets, int max_distance, int32_t* out) {
  if (T < 1 || num_buckets < 4 || max_distance < 2 || !out || max_distance <= num_buckets / 4) {
    set_error("sty_wavlm_rel_buckets_host: bad argument");
    return STY_EINVAL;
  }
  wavlm_rel_buckets(T, num_buckets, max_distance, out);
  return STY_OK;
}
int sty_slm_loss_workspace_bytes(size_t n, size_t* bytes) {
  if (!bytes || n == 0) {
    set_error("sty_slm_loss_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  *bytes = (size_t)slm_loss_groups(n) * sizeof(double);
  return STY_OK;
}
int sty_slm_loss_fwd(size_t n, const float* a, const float* b, float* loss, void* workspace, size_t ws_bytes, void* stream) {
  if (!a || !b || !loss || !workspace || n == 0 || ((uintptr_t)workspace & 7)) {
    set_error("sty_slm_loss_fwd: bad argument");
    return STY_EINVAL;
  }
  if (ws_bytes < (size_t)slm_loss_groups(n) * sizeof(double)) {
    set_error("sty_slm_loss_fwd: workspace too small");
    return STY_ENOMEM;
  }
  return launch_slm_loss(n, a, b, loss, (double*)workspace, S(stream));
}
int sty_slm_loss_fwd_bwd(size_t n, const float* a, const float* b, float scale, float* loss, float* d_b, void* workspace, size_t ws_bytes,
                         void* stream) {
  if (!a || !b || !loss || !d_b || !workspace || n == 0 || ((uintptr_t)workspace & 7)) {
    set_error("sty_slm_loss_fwd_bwd: bad argument");
    return STY_EINVAL;
  }
  if (ws_bytes < (size_t)slm_loss_groups(n) * sizeof(double)) {
    set_error("sty_slm_loss_fwd_bwd: workspace too small");
    return STY_ENOMEM;
  }
  // d mean|a - b| / d b = sign(b - a) / n, times scale: one magnitude, formed as torch's division by a host scalar is
  // (a multiplication by the fp32 reciprocal)
  const float mag = scale * (1.0f / (float)n);
  return launch_slm_loss(n, a, b, loss, (double*)workspace, S(stream), mag, d_b);
}

}  // extern "C"
