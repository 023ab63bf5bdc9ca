// The model-free unit entries: one kernel family or loss on the caller's buffers, for parity tests and kernel tuning.
#include "run.h"

using namespace sty;

extern "C" {

// softmax attention forward + backward on separate q / k / v [B][H*DH][T] (DH = 16: the text encoder's VALU backward with
// an optional length mask; DH = 64 / 96 / 160: the fp32 matrix-core backward -- the conformer's 8 x 64, the prosody encoder's
// 2 x 160 / 2 x 96 with the length mask)
int sty_attention_workspace_bytes(int B, int H, int T, size_t* bytes) {
  if (!bytes || B <= 0 || H <= 0 || T <= 0) {
    set_error("sty_attention_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  *bytes = (attention_bwd_ws_floats(B, H, T) + (size_t)B * H * T) * sizeof(float) + 1024;
  return STY_OK;
}
int sty_attention_fwd_bwd(int B, int H, int DH, int T, const float* q, const float* k, const float* v,
                          const int64_t* lengths, const float* d_o, float* o, float* dq, float* dk, float* dv,
                          void* workspace, size_t ws_bytes, void* stream) {
  size_t need = 0;
  if (sty_attention_workspace_bytes(B, H, T, &need)) return STY_EINVAL;
  if (!q || !k || !v || !d_o || !o || !dq || !dk || !dv || !workspace || ws_bytes < need ||
      (DH != 16 && DH != 64 && DH != 96 && DH != 160)) {
    set_error("sty_attention_fwd_bwd: bad argument (DH = 16, 64, 96 or 160, workspace >= %zu bytes)", need);
    return STY_EINVAL;
  }
  hipStream_t st = S(stream);
  const size_t n = (size_t)B * H * DH * T;
  AttnArgs at;
  at.q = q;
  at.k = k;
  at.v = v;
  at.o = o;
  at.qbs = at.kbs = at.vbs = at.obs = (size_t)H * DH * T;
  at.T = T;
  at.H = H;
  at.scale = 1.0f / sqrtf((float)DH);
  at.lengths = lengths;
  at.bf16 = getenv("STY_ATTN_UNIT_BF16") != nullptr;  // (read per call: the unit test of attn16.hip sets it)
  float* ws = static_cast<float*>(workspace);
  at.lse = ws;  // row log-sum-exp, kept for the MFMA backward
  float* w2 = ws + (size_t)B * H * T;
  STY_HIP(hipMemsetAsync(dq, 0, n * sizeof(float), st));
  STY_HIP(hipMemsetAsync(dk, 0, n * sizeof(float), st));
  STY_HIP(hipMemsetAsync(dv, 0, n * sizeof(float), st));
  int rc = launch_attention(at, B, DH, st);
  if (rc) return rc;
  return launch_attention_bwd(at, d_o, dq, dk, dv, at.qbs, at.kbs, at.vbs, at.obs, B, DH, w2, st);
}

// ... with WavLM's gated relative position bias: logit (i, j) = scale q_i . k_j + gate[b][h][i] * tab[h][j - i + T - 1]; the
// launches wavlm_forward (keep mode) and wavlm_backward make for one layer, in the mode asked for.  workspace: sty_attention_workspace_bytes
int sty_attention_rel_fwd_bwd(int B, int H, int DH, int T, const float* q, const float* k, const float* v, const float* gate,
                              const float* tab, const float* d_o, float* o, float* dq, float* dk, float* dv, float* d_gate,
                              int compute_bf16, void* workspace, size_t ws_bytes, void* stream) {
  size_t need = 0;
  if (sty_attention_workspace_bytes(B, H, T, &need)) return STY_EINVAL;
  if (!q || !k || !v || !gate || !tab || !d_o || !o || !dq || !dk || !dv || !d_gate || !workspace || ws_bytes < need ||
      (DH != 16 && DH != 64) || (compute_bf16 != 0 && compute_bf16 != 1)) {
    set_error("sty_attention_rel_fwd_bwd: bad argument (DH = 16 or 64, compute_bf16 0 or 1, workspace >= %zu bytes)", need);
    return STY_EINVAL;
  }
  if (compute_bf16 && DH != 64) {
    set_error("sty_attention_rel_fwd_bwd: head dim %d runs the fp32 kernels in both modes (the bf16 matrix-core variant is head dim 64)", DH);
    return STY_EINVAL;
  }
  hipStream_t st = S(stream);
  const size_t n = (size_t)B * H * DH * T;
  AttnArgs at;
  at.q = q, at.k = k, at.v = v, at.o = o;
  at.qbs = at.kbs = at.vbs = at.obs = (size_t)H * DH * T;
  at.T = T, at.H = H;
  at.scale = 1.0f / sqrtf((float)DH);
  at.lengths = nullptr;
  at.bf16 = compute_bf16;
  at.rel_tab = tab, at.rel_gate = gate, at.rel_dgate = d_gate;
  float* ws = static_cast<float*>(workspace);
  at.lse = ws;
  float* w2 = ws + (size_t)B * H * T;
  STY_HIP(hipMemsetAsync(dq, 0, n * sizeof(float), st));
  STY_HIP(hipMemsetAsync(dk, 0, n * sizeof(float), st));
  STY_HIP(hipMemsetAsync(dv, 0, n * sizeof(float), st));
  int rc = launch_attention(at, B, DH, st);
  if (rc) return rc;
  return launch_attention_bwd(at, d_o, dq, dk, dv, at.qbs, at.kbs, at.vbs, at.obs, B, DH, w2, st);
}

static float* g_bases = nullptr;  // default STFT(64) bases for the model-free entry points
static int ensure_bases() {
  if (g_bases) return STY_OK;
  float host[4 * 33 * 64];
  build_stft64_bases(host);
  STY_HIP(hipMalloc((void**)&g_bases, sizeof(host)));
  STY_HIP(hipMemcpy(g_bases, host, sizeof(host), hipMemcpyHostToDevice));
  return STY_OK;
}

void sty_stft64_bases_host(float* out) { build_stft64_bases(out); }

int sty_stft64_fwd(int B, int N, const float* wave, float* spec, float* phase, void* stream) {
  if (!wave || !spec || !phase || B <= 0 || N < 64 || N % 4) {
    set_error("sty_stft64_fwd: bad argument");
    return STY_EINVAL;
  }
  int rc = ensure_bases();
  if (rc) return rc;
  return launch_stft64(B, N, wave, g_bases, g_bases + 33 * 64, spec, phase, S(stream));
}

int sty_istft64_fwd(int B, int F, const float* logamp, const float* real, const float* imag, float* audio,
                    void* stream) {
  if (!logamp || !real || !imag || !audio || B <= 0 || F <= 0) {
    set_error("sty_istft64_fwd: bad argument");
    return STY_EINVAL;
  }
  int rc = ensure_bases();
  if (rc) return rc;
  return launch_istft64(B, F, logamp, real, imag, g_bases + 2 * 33 * 64, g_bases + 3 * 33 * 64, audio, S(stream));
}

int sty_source_workspace_bytes(int B, int T, size_t* bytes) {
  if (!bytes || B <= 0 || T <= 1) {
    set_error("sty_source_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  *bytes = (size_t)source_workspace_floats(B, T) * sizeof(float);
  return STY_OK;
}

int sty_source_fwd(int B, int T, const float* pitch, const float* voiced, const float* noise, uint64_t seed,
                   const float* lin_w, const float* lin_b, float* prior, void* workspace, size_t ws_bytes,
                   void* stream) {
  if (!pitch || !voiced || !lin_w || !lin_b || !prior || !workspace || B <= 0 || T <= 1) {
    set_error("sty_source_fwd: bad argument");
    return STY_EINVAL;
  }
  if (ws_bytes < (size_t)source_workspace_floats(B, T) * sizeof(float)) {
    set_error("sty_source_fwd: workspace too small");
    return STY_ENOMEM;
  }
  return launch_source(B, T, pitch, voiced, noise, seed, lin_w, lin_b, prior, (float*)workspace, S(stream));
}

int sty_alignment_fwd(int B, int L, int T, const float* durations, float* alignment, void* stream) {
  if (!durations || !alignment || B <= 0 || L <= 0 || T <= 0) {
    set_error("sty_alignment_fwd: bad argument");
    return STY_EINVAL;
  }
  return launch_alignment(durations, B, L, T, alignment, S(stream));
}

// ---- what the four sty_conv1d_* entries share: a caller's dense conv, packed into the front of the caller's workspace ----
static PackedConv unit_conv_dims(int Cin, int Cout, int K) {
  PackedConv pc;
  pc.Cin = Cin;
  pc.Cout = Cout;
  pc.K = K;
  pc.CinP = (int)align_up(Cin, CI_CHUNK);
  pc.CoutP = (int)align_up(Cout, 32);  // the model's padding rule (prepare_conv)
  return pc;
}
// floats of the packed weight [K][CinP][CoutP] with its bias row behind it
static size_t unit_conv_plane(const PackedConv& pc) { return (size_t)pc.K * pc.CinP * pc.CoutP + pc.CoutP; }
static float* unit_ws_front(void* workspace) { return reinterpret_cast<float*>(align_up(reinterpret_cast<size_t>(workspace), 256)); }
// w [Cout][Cin][K] (and bias, if any) -> pc.wp and the bias row at the workspace's front; `clear` floats from there are zeroed
// first (the padding, and whatever else of the caller's lies behind).  bias_row: pc.bias names the row.
static int unit_conv_pack(PackedConv& pc, const float* w, const float* bias, bool bias_row, void* workspace, size_t clear,
                          hipStream_t st) {
  float* wp = unit_ws_front(workspace);
  float* bp = wp + (size_t)pc.K * pc.CinP * pc.CoutP;
  STY_HIP(hipMemsetAsync(wp, 0, clear * sizeof(float), st));
  const int rc = launch_pack_conv(w, nullptr, nullptr, bias, pc.Cout, pc.Cin, pc.K, wp, bp, pc.CinP, pc.CoutP, st);
  if (rc) return rc;
  pc.wp = wp;
  pc.bias = bias_row ? bp : nullptr;
  return STY_OK;
}
// the dense conv with 'same' padding over x [B][Cin][T] -> y
static ConvArgs unit_conv_args(const PackedConv& w, int B, int T, int dil, const float* x, float* y, int bf16) {
  const int Cin = w.Cin, K = w.K;
  ConvArgs a;
  a.x[0] = x;
  a.xc[0] = Cin;
  a.nsrc = 1;
  a.B = B;
  a.T = T;
  a.w = w;
  a.dil = dil;
  a.pad = (K - 1) * dil / 2;
  a.y = y;
  a.bf16 = bf16;
  return a;
}
// the packed weight's share of the workspace, and behind it (compute mode 4) the split mode's fragment triples of a conv with
// one 32-channel chunk each way
static size_t unit_conv_base_bytes(int Cout, int Cin, int K) {
  return ((size_t)K * align_up(Cin, CI_CHUNK) * align_up(Cout, 128) + align_up(Cout, 128)) * sizeof(float) + 512;
}
static bool unit_conv_splittable(int Cout, int Cin) { return Cin <= CI_CHUNK && Cout <= 32; }
// ---- one dense Conv1d ('same' padding) on the MFMA conv kernel: unit parity and kernel tuning ----
int sty_conv1d_workspace_bytes(int Cout, int Cin, int K, size_t* bytes) {
  if (!bytes || Cout <= 0 || Cin <= 0 || K <= 0) {
    set_error("sty_conv1d_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  *bytes = unit_conv_base_bytes(Cout, Cin, K) + (unit_conv_splittable(Cout, Cin) ? split3_bytes(K) + 256 : 0);
  return STY_OK;
}
int sty_conv1d_fwd(int B, int Cin, int Cout, int K, int dil, int T, const float* x, const float* w, const float* bias,
                   float* y, void* workspace, size_t ws_bytes, int compute_bf16, void* stream) {
  size_t need = 0;
  int rc = sty_conv1d_workspace_bytes(Cout, Cin, K, &need);
  if (rc) return rc;
  if (!x || !w || !y || !workspace || B <= 0 || T <= 0 || dil <= 0 || (K - 1) * dil > 128 || ws_bytes < need) {
    set_error("sty_conv1d_fwd: bad argument, halo > 128 or workspace too small");
    return STY_EINVAL;
  }
  PackedConv pc = unit_conv_dims(Cin, Cout, K);
  if ((rc = unit_conv_pack(pc, w, bias, bias != nullptr, workspace, unit_conv_plane(pc), S(stream)))) return rc;
  if (compute_bf16 == 4 && unit_conv_splittable(Cout, Cin)) {  // the split mode's fragment triples, behind the packed weight
    void* w3 = reinterpret_cast<void*>(
        align_up(reinterpret_cast<size_t>(static_cast<char*>(workspace) + unit_conv_base_bytes(Cout, Cin, K)), 256));
    if ((rc = launch_pack_split3(pc.wp, K, w3, S(stream)))) return rc;
    pc.w3 = w3;
  }
  ConvArgs a = unit_conv_args(pc, B, T, dil, x, y, compute_bf16 != 0 && compute_bf16 != 4);
  a.split = compute_bf16 == 4;
  if (compute_bf16 == 2) {
    // the input as its bf16 operand twin (ConvArgs::x16), made here by the cast pass, and a twin of the OUTPUT written by
    // the conv's output stage (ConvArgs::y16), which is read back and checked against y by ... the caller: the twin
    // occupies the tail of the workspace, [B][Cin][T] then [B][Cout][T] bf16
    const size_t tw = ((size_t)B * (Cin + Cout) * T) * sizeof(__bf16) + 512;
    if (ws_bytes < need + tw) {
      set_error("sty_conv1d_fwd: compute_bf16 = 2 needs %zu more workspace bytes for the operand twins", tw);
      return STY_EINVAL;
    }
    __bf16* x16 = reinterpret_cast<__bf16*>(align_up(reinterpret_cast<size_t>(static_cast<char*>(workspace) + need), 256));
    if ((rc = launch_twin_cast(x, nullptr, PRO_NONE, B, Cin, T, x16, S(stream)))) return rc;
    a.x16 = x16;
    a.y16 = x16 + (size_t)B * Cin * T;
    a.y16_act = PRO_LRELU;
  }
  return launch_conv1d(a, S(stream));
}
// the generator's up-sampling conv: the output leaves pixel-shuffled, y [B][Cout / shuffle][T shuffle]
int sty_conv1d_fwd_shuffle(int B, int Cin, int Cout, int K, int dil, int T, int shuffle, const float* x, const float* w,
                           const float* bias, float* y, void* workspace, size_t ws_bytes, int compute_bf16, void* stream) {
  size_t need = 0;
  int rc = sty_conv1d_workspace_bytes(Cout, Cin, K, &need);
  if (rc) return rc;
  if (!x || !w || !y || !workspace || B <= 0 || T <= 0 || dil <= 0 || (K - 1) * dil > 128 || ws_bytes < need || shuffle < 1 ||
      Cout % shuffle || !(compute_bf16 == 0 || compute_bf16 == 1)) {
    set_error("sty_conv1d_fwd_shuffle: bad argument, halo > 128, Cout no multiple of shuffle, a compute mode other than 0 / 1 or "
              "workspace too small");
    return STY_EINVAL;
  }
  PackedConv pc = unit_conv_dims(Cin, Cout, K);
  if ((rc = unit_conv_pack(pc, w, bias, bias != nullptr, workspace, unit_conv_plane(pc), S(stream)))) return rc;
  ConvArgs a = unit_conv_args(pc, B, T, dil, x, y, compute_bf16);
  a.shuffle = shuffle;
  return launch_conv1d(a, S(stream));
}
// the same conv with the fused prologue / output stage the text encoder's convs use (fp32 tensors only)
int sty_conv1d_fwd_ex(int B, int Cin, int Cout, int K, int dil, int T, const float* x, const float* w, const float* bias,
                      const float* in_mask, const float* residual, const float* out_mask, int out_mask_post, int relu, float* y,
                      void* workspace, size_t ws_bytes, int compute_bf16, void* stream) {
  size_t need = 0;
  int rc = sty_conv1d_workspace_bytes(Cout, Cin, K, &need);
  if (rc) return rc;
  if (!x || !w || !y || !workspace || B <= 0 || T <= 0 || dil <= 0 || (K - 1) * dil > 128 || ws_bytes < need ||
      !(compute_bf16 == 0 || compute_bf16 == 1)) {
    set_error("sty_conv1d_fwd_ex: bad argument, halo > 128, a compute mode other than 0 / 1 or workspace too small");
    return STY_EINVAL;
  }
  PackedConv pc = unit_conv_dims(Cin, Cout, K);
  if ((rc = unit_conv_pack(pc, w, bias, bias != nullptr, workspace, unit_conv_plane(pc), S(stream)))) return rc;
  ConvArgs a = unit_conv_args(pc, B, T, dil, x, y, compute_bf16);
  if (in_mask) {
    a.pro = PRO_MASK;
    a.mask = in_mask;
  }
  a.act = relu ? ACT_RELU : ACT_NONE;
  a.residual = residual;
  a.out_mask = out_mask;
  a.out_mask_post = out_mask ? out_mask_post : 0;
  return launch_conv1d(a, S(stream));
}
// Which kernel family launch_conv1d picks for a conv of this shape (host only, nothing is launched): *kernel = the ConvKernel
// value, -1 where the conv is refused.  flags: STY_ROUTE_* of stylish_hip.h, operands the conv would carry.
int sty_conv1d_route(int B, int Cin, int Cout, int K, int dil, int T, int compute_bf16, int flags, int* kernel) {
  if (!kernel || B <= 0 || Cin <= 0 || Cout <= 0 || K <= 0 || T <= 0 || dil <= 0) {
    set_error("sty_conv1d_route: bad argument");
    return STY_EINVAL;
  }
  static_assert(STY_CONV_STEM2D == CONV_STEM2D && STY_CONV_32P == CONV_32P && STY_CONV_SC == CONV_SC && STY_CONV_K1 == CONV_K1 &&
                    STY_CONV_Q == CONV_Q && STY_CONV_P16 == CONV_P16 && STY_CONV_TILED == CONV_TILED,
                "stylish_hip.h lists the families in the order of ConvKernel");
  static float dummy_f[4];
  static double dummy_d[4];
  static __bf16 dummy_h[4];
  PackedConv pc = unit_conv_dims(Cin, Cout, K);
  pc.wp = dummy_f;
  if (compute_bf16 == 4 && unit_conv_splittable(Cout, Cin)) pc.w3 = dummy_f;
  ConvArgs a = unit_conv_args(pc, B, T, dil, dummy_f, dummy_f, compute_bf16 != 0 && compute_bf16 != 4);
  a.split = compute_bf16 == 4;
  if (flags & STY_ROUTE_IN_MASK) {
    a.pro = PRO_MASK;
    a.mask = dummy_f;
  }
  if (flags & STY_ROUTE_RESIDUAL) a.residual = dummy_f;
  if (flags & STY_ROUTE_OUT_MASK) a.out_mask = dummy_f;
  if (flags & STY_ROUTE_RELU) a.act = ACT_RELU;
  if (flags & STY_ROUTE_TWO_BYTE_X) a.xh = 1;
  if (flags & STY_ROUTE_STATS) a.stat_part = dummy_d;
  if (flags & STY_ROUTE_Y16) a.y16 = dummy_h;
  if (flags & STY_ROUTE_X16) a.x16 = dummy_h;
  if (flags & STY_ROUTE_FLAT_IMAGE) {
    if (Cin % 3) {
      set_error("sty_conv1d_route: flat-image mode needs Cin = 3 * image channels");
      return STY_EINVAL;
    }
    a.flatW = 4;  // (no family's predicate reads the pitch's value)
    a.hpad = 1;
    a.Cin2d = Cin / 3;
  }
  const int sf = (flags >> STY_ROUTE_SHUFFLE_SHIFT) & 15;  // the factor of a shuffled store / source
  if ((flags & (STY_ROUTE_SHUFFLE_STORE | STY_ROUTE_SHUFFLE_SOURCE)) && sf < 2) {
    set_error("sty_conv1d_route: a shuffled store / source needs its factor (2 .. 15) in bits %d .. %d of flags",
              STY_ROUTE_SHUFFLE_SHIFT, STY_ROUTE_SHUFFLE_SHIFT + 3);
    return STY_EINVAL;
  }
  if (flags & STY_ROUTE_SHUFFLE_STORE) a.shuffle = sf;
  if (flags & STY_ROUTE_SHUFFLE_SOURCE) a.in_shuffle = sf;
  const ConvRoute r = conv1d_route(a);
  *kernel = r.refusal == CONV_OK ? (int)r.kernel : -1;
  return STY_OK;
}
int sty_conv1d_bwd_workspace_bytes(int B, int Cin, int Cout, int K, int T, size_t* bytes) {
  if (!bytes || B <= 0 || Cin <= 0 || Cout <= 0 || K <= 0 || T <= 0) {
    set_error("sty_conv1d_bwd_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  const PackedConv pc = unit_conv_dims(Cin, Cout, K);
  *bytes = (3 * unit_conv_plane(pc) + wgrad_partial_floats(pc, B, T)) * sizeof(float) + 1024;  // weights, gradient, flipped weights
  *bytes += (size_t)B * (Cin + Cout) * T * sizeof(__bf16) + 512;                   // compute_bf16 = 2: the two operand twins
  return STY_OK;
}
// shuffle > 1: gy is the gradient of the pixel-shuffled output, [B][Cout / shuffle][T shuffle]; accumulate: dx += (the input-
// gradient conv takes dx as its residual, as conv_bwd does with a gradient buffer that already holds a term)
static int unit_conv_bwd(int B, int Cin, int Cout, int K, int dil, int T, int shuffle, const float* x, const float* w,
                         const float* gy, float* dw, float* dbias, float* dx, int accumulate, void* workspace, size_t ws_bytes,
                         int compute_bf16, void* stream) {
  size_t need = 0;
  int rc = sty_conv1d_bwd_workspace_bytes(B, Cin, Cout, K, T, &need);
  if (rc) return rc;
  if (!x || !w || !gy || !dw || !workspace || dil <= 0 || (K - 1) * dil > 128 || ws_bytes < need) {
    set_error("sty_conv1d_bwd: bad argument, halo > 128 or workspace too small");
    return STY_EINVAL;
  }
  hipStream_t st = S(stream);
  PackedConv pc = unit_conv_dims(Cin, Cout, K);
  const size_t plane = (size_t)K * pc.CinP * pc.CoutP;
  float* wp = unit_ws_front(workspace);
  float* gwp = wp + unit_conv_plane(pc);  // packed gradient: [K][CinP][CoutP] + bias tail
  float* gbp = gwp + plane;
  PackedConv pd;
  pd.Cin = Cout;
  pd.Cout = Cin;
  pd.K = K;
  pd.CinP = pc.CoutP;  // the flipped weights are the transposed packed block (add_dgrad)
  pd.CoutP = pc.CinP;
  float* wd = gbp + pc.CoutP;
  float* partial = wd + plane + pc.CoutP;
  // (the clear takes the gradient and the flipped weights with it: everything in front of the partial planes)
  if ((rc = unit_conv_pack(pc, w, nullptr, dbias != nullptr, workspace, (size_t)(partial - wp), st))) return rc;
  ConvArgs a = unit_conv_args(pc, B, T, dil, x, nullptr, compute_bf16 != 0);
  a.shuffle = shuffle;
  if (compute_bf16 == 3) {  // x is a bf16 TENSOR (two-byte storage, ConvArgs::xh): the weight gradient alone has a form for it here
    if (dx || T % 2) {
      set_error("sty_conv1d_bwd: a two-byte x (compute_bf16 = 3) is for dw / dbias only (dx == NULL), T even");
      return STY_EINVAL;
    }
    a.xh = 1;
  }
  if (compute_bf16 == 2) {  // bf16 operand twins of x and gy (ConvArgs::x16 / g16), made here by the cast pass
    __bf16* x16 = reinterpret_cast<__bf16*>(align_up(reinterpret_cast<size_t>(partial + wgrad_partial_floats(pc, B, T)), 256));
    __bf16* g16 = x16 + (size_t)B * Cin * T;
    if ((rc = launch_twin_cast(x, nullptr, PRO_NONE, B, Cin, T, x16, st))) return rc;
    if ((rc = launch_twin_cast(gy, nullptr, PRO_NONE, B, Cout, T, g16, st))) return rc;
    a.x16 = x16;
    a.g16 = g16;
  }
  bool bias_done = false;
  rc = launch_conv1d_wgrad(a, gy, nullptr, 1.0f, gwp, partial, dbias ? gbp : nullptr, &bias_done, st);
  if (rc) return rc;
  if (dbias && !bias_done) {
    set_error("sty_conv1d_bwd: this conv's bias gradient is a separate pass (launch_bias_grad), not wired here");
    return STY_EINVAL;
  }
  STY_HIP(hipMemsetAsync(dw, 0, (size_t)Cout * Cin * K * sizeof(float), st));
  rc = launch_unpack_grad(gwp, nullptr, nullptr, Cout, Cin, K, pc.CinP, pc.CoutP, dw, nullptr, nullptr, st);
  if (rc) return rc;
  if (dbias) STY_HIP(hipMemcpyAsync(dbias, gbp, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (dx) {
    PackedConv pdm = pd;
    rc = launch_pack_dgrad(wp, K, pc.CinP, pc.CoutP, wd, st);
    if (rc) return rc;
    pdm.wp = wd;
    pdm.bias = nullptr;
    ConvArgs d = unit_conv_args(pdm, B, T, dil, gy, dx, a.bf16);
    d.pad = (K - 1) * dil - a.pad;  // the other half of an even halo
    d.x16 = a.g16;  // (compute_bf16 = 2) the input-gradient conv reads the gradient's operand twin as well
    d.in_shuffle = shuffle > 1 ? shuffle : 0;
    d.residual = accumulate ? dx : nullptr;
    rc = launch_conv1d(d, st);
  }
  return rc;
}
int sty_conv1d_bwd(int B, int Cin, int Cout, int K, int dil, int T, const float* x, const float* w, const float* gy,
                   float* dw, float* dbias, float* dx, void* workspace, size_t ws_bytes, int compute_bf16,
                   void* stream) {
  return unit_conv_bwd(B, Cin, Cout, K, dil, T, 1, x, w, gy, dw, dbias, dx, 0, workspace, ws_bytes, compute_bf16, stream);
}
int sty_conv1d_bwd_shuffle(int B, int Cin, int Cout, int K, int dil, int T, int shuffle, const float* x, const float* w,
                           const float* gy, float* dw, float* dbias, float* dx, int accumulate, void* workspace, size_t ws_bytes,
                           int compute_bf16, void* stream) {
  if (shuffle < 1 || Cout <= 0 || Cout % shuffle || !(compute_bf16 == 0 || compute_bf16 == 1) || (accumulate && !dx)) {
    set_error("sty_conv1d_bwd_shuffle: Cout no multiple of shuffle, a compute mode other than 0 / 1, or accumulate without dx");
    return STY_EINVAL;
  }
  return unit_conv_bwd(B, Cin, Cout, K, dil, T, shuffle, x, w, gy, dw, dbias, dx, accumulate, workspace, ws_bytes, compute_bf16,
                       stream);
}
int sty_partial_sum(int dw_form, const float* part, int C, int K, int nblk, float* dw, float* db, void* stream) {
  if (!part || !db || C <= 0 || nblk <= 0 || (dw_form && (!dw || K <= 0))) {
    set_error("sty_partial_sum: bad argument");
    return STY_EINVAL;
  }
  return launch_partial_sum(dw_form, part, C, K, nblk, dw, db, S(stream));
}
// ---- unit entries of the backward's normalisation / activation kernels (tests/test_backward_chain.py) ----
static size_t grn_bwd_ws_bytes(int B, int C4, int T) {  // partials (doubles) | scale | gx
  return (size_t)B * C4 * row_stats_nseg(T) * 2 * sizeof(double) + (size_t)2 * B * C4 * sizeof(float);
}
int sty_grn_bwd_workspace_bytes(int B, int C4, int T, size_t* bytes) {
  if (!bytes || B <= 0 || C4 <= 0 || T <= 0) {
    set_error("sty_grn_bwd_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  *bytes = grn_bwd_ws_bytes(B, C4, T);
  return STY_OK;
}
int sty_grn_bwd(int B, int C4, int T, const float* h, const float* ds, const float* gamma, int from_gx, float* coef,
                float* dgamma, void* workspace, size_t ws_bytes, void* stream) {
  if (!h || !ds || !gamma || !coef || !dgamma || !workspace || B <= 0 || C4 <= 0 || T <= 0) {
    set_error("sty_grn_bwd: bad argument");
    return STY_EINVAL;
  }
  if (ws_bytes < grn_bwd_ws_bytes(B, C4, T)) {
    set_error("sty_grn_bwd: workspace too small");
    return STY_ENOMEM;
  }
  hipStream_t st = S(stream);
  const int nseg = row_stats_nseg(T);
  double* part = (double*)workspace;
  float* scale = (float*)(part + (size_t)B * C4 * nseg * 2);
  float* gx = scale + (size_t)B * C4;
  int rc = launch_row_stats(h, B * C4, T, part, st);
  if (rc) return rc;
  if ((rc = launch_grn_finalize(part, nseg, gamma, B, C4, scale, st, gx))) return rc;
  if (deterministic_mode() && B > 1) {
    // deterministic mode: one launch per utterance; the adds into dgamma then meet in stream order (this unit entry has no
    // room for slots in the workspace its callers size)
    for (int b = 0; b < B; ++b) {
      const size_t o = (size_t)b * C4;
      if ((rc = launch_grn_bwd(from_gx ? gx + o : nullptr, part + o * nseg * 2, nseg, gamma, ds + o, 1, C4, coef + o, dgamma, st)))
        return rc;
    }
    return STY_OK;
  }
  return launch_grn_bwd(from_gx ? gx : nullptr, part, nseg, gamma, ds, B, C4, coef, dgamma, st);
}
int sty_act_bwd(int kind, int B, int C, int T, const float* x, float* dy, const float* alpha, const float* h,
                const float* coef, int fused, float* dx, int accumulate, float* dalpha, void* stream) {
  if (!x || !dy || !dx || B <= 0 || C <= 0 || T <= 0 || (kind == ACT_SNAKE && !alpha) || ((h != nullptr) != (coef != nullptr))) {
    set_error("sty_act_bwd: bad argument");
    return STY_EINVAL;
  }
  hipStream_t st = S(stream);
  if (h && !fused) {  // the row term as a pass of its own: dy += coef[row] * h IN PLACE, then the plain activation backward
    const int rc = launch_row_scale_add(h, coef, 0.f, B * C, T, dy, st);
    if (rc) return rc;
    h = coef = nullptr;
  }
  if (deterministic_mode() && kind == ACT_SNAKE && dalpha && B > 1) {
    // deterministic mode: one launch per utterance, so that the rows' adds into d alpha meet in stream order
    for (int b = 0; b < B; ++b) {
      const size_t o = (size_t)b * C * T;
      const int rc = launch_act_bwd(kind, x + o, dy + o, alpha, 1, C, T, dx + o, accumulate, dalpha, st, h ? h + o : nullptr,
                                    coef ? coef + (size_t)b * C : nullptr);
      if (rc) return rc;
    }
    return STY_OK;
  }
  return launch_act_bwd(kind, x, dy, alpha, B, C, T, dx, accumulate, dalpha, st, h, coef);
}
int sty_adain_finalize(int B, int C, int T, int nseg, const double* part, const float* gb, float eps, float* a, float* s,
                       float* mean, float* rstd, void* stream) {
  if (!part || !gb || !a || !s || B <= 0 || C <= 0 || T <= 0 || nseg <= 0 || ((mean != nullptr) != (rstd != nullptr))) {
    set_error("sty_adain_finalize: bad argument");
    return STY_EINVAL;
  }
  return launch_adain_finalize(part, nseg, gb, B, C, T, eps, a, s, S(stream), mean, rstd);
}
int sty_mel_workspace_bytes(int B, int N, int n_fft, int hop, size_t* bytes) {
  if (!bytes || B <= 0 || N <= n_fft / 2 || n_fft <= 0 || hop <= 0) {
    set_error("sty_mel_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  *bytes = mel_workspace_floats(B, N, n_fft, hop, 80) * sizeof(float);
  return STY_OK;
}
int sty_mel_fwd(int B, int N, const float* audio, int n_fft, int win_length, int hop, float mean, float std_,
                float* mel, float* energy, void* workspace, size_t ws_bytes, void* stream) {
  if (!audio || !mel || !workspace || B <= 0 || N <= n_fft / 2 || win_length > n_fft || hop <= 0 || std_ == 0.f) {
    set_error("sty_mel_fwd: bad argument");
    return STY_EINVAL;
  }
  if (ws_bytes < mel_workspace_floats(B, N, n_fft, hop, 80) * sizeof(float)) {
    set_error("sty_mel_fwd: workspace too small");
    return STY_ENOMEM;
  }
  return launch_mel(B, N, audio, n_fft, win_length, hop, 80, 24000, mean, std_, mel, energy, (float*)workspace,
                    S(stream));
}
int sty_multispec_workspace_bytes(int B, int N, size_t* bytes) {
  if (!bytes || B <= 0 || N <= 1024) {
    set_error("sty_multispec_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  size_t mx = 0;
  const int res[3][2] = {{512, 128}, {1024, 256}, {2048, 512}};
  for (auto& r : res) {
    const size_t n = multispec_workspace_floats(B, N, r[0], r[1]);
    mx = n > mx ? n : mx;
  }
  *bytes = mx * sizeof(float);
  return STY_OK;
}
int sty_multispec_fwd(int B, int N, const float* audio, float* const* mag, float* const* phase, float* const* fft_mag,
                      void* workspace, size_t ws_bytes, void* stream) {
  if (!audio || !mag || !fft_mag || !workspace || B <= 0 || N <= 1024) {
    set_error("sty_multispec_fwd: bad argument");
    return STY_EINVAL;
  }
  size_t need = 0;
  int rc = sty_multispec_workspace_bytes(B, N, &need);
  if (rc) return rc;
  if (ws_bytes < need) {
    set_error("sty_multispec_fwd: workspace too small");
    return STY_ENOMEM;
  }
  const int res[3][2] = {{512, 128}, {1024, 256}, {2048, 512}};  // multi_spectrogram.py:13-20
  for (int i = 0; i < 3; ++i) {
    rc = launch_multispec_single(B, N, audio, res[i][0], res[i][1], 24000, mag[i], phase ? phase[i] : nullptr,
                                 fft_mag[i], (float*)workspace, S(stream));
    if (rc) return rc;
  }
  return STY_OK;
}

int sty_acoustic_loss_workspace_bytes(int B, int N, size_t* bytes) {
  if (!bytes || B <= 0 || N <= 1024) {
    set_error("sty_acoustic_loss_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  *bytes = acoustic_loss_workspace_floats(B, N) * sizeof(float);
  return STY_OK;
}
int sty_acoustic_loss_fwd_bwd(int B, int N, const float* audio_gt, const float* audio_pred, float w_mel, float w_phase,
                              float* losses, float* d_audio_pred, void* workspace, size_t ws_bytes, void* stream) {
  if (!audio_pred || !losses || !d_audio_pred || !workspace || B <= 0 || N <= 1024) {  // (audio_gt may be NULL: header)
    set_error("sty_acoustic_loss_fwd_bwd: bad argument");
    return STY_EINVAL;
  }
  if (ws_bytes < acoustic_loss_workspace_floats(B, N) * sizeof(float)) {
    set_error("sty_acoustic_loss_fwd_bwd: workspace too small");
    return STY_ENOMEM;
  }
  return launch_acoustic_loss(B, N, audio_gt, audio_pred, w_mel, w_phase, losses, d_audio_pred, (float*)workspace,
                              S(stream));
}

int sty_acoustic_loss_target(int B, int N, const float* audio_gt, void* workspace, size_t ws_bytes, void* stream) {
  if (!audio_gt || !workspace || B <= 0 || N <= 1024) {
    set_error("sty_acoustic_loss_target: bad argument");
    return STY_EINVAL;
  }
  if (ws_bytes < acoustic_loss_workspace_floats(B, N) * sizeof(float)) {
    set_error("sty_acoustic_loss_target: workspace too small");
    return STY_ENOMEM;
  }
  return launch_acoustic_loss(B, N, audio_gt, nullptr, 0.f, 0.f, nullptr, nullptr, (float*)workspace, S(stream));
}

int sty_acoustic_gan_workspace_bytes(int B, int N, int with_grads, size_t* bytes) {
  if (!bytes || B <= 0 || N <= 1024) {
    set_error("sty_acoustic_gan_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  *bytes = acoustic_gan_workspace_bytes(B, N, with_grads);
  return STY_OK;
}
int sty_acoustic_gan_loss_fwd_bwd(int B, int N, const float* audio_gt, const float* audio_pred, float w_mel, float w_phase,
                                  float w_gen, const sty_specdisc_params* mrd, float disc_scale,
                                  const sty_specdisc_grads* mrd_grads, int step_mask, float* losses, float* gan_losses,
                                  float* d_audio_pred, void* workspace, size_t ws_bytes, void* gan_workspace,
                                  size_t gan_ws_bytes, int compute_bf16, void* stream) {
  if (!audio_pred || !losses || !gan_losses || !d_audio_pred || !workspace || !gan_workspace || !mrd ||  // (audio_gt may
      B <= 0 || N <= 1024 || (step_mask && !mrd_grads)) {                                                 // be NULL: header)
    set_error("sty_acoustic_gan_loss_fwd_bwd: bad argument");
    return STY_EINVAL;
  }
  if (ws_bytes < acoustic_loss_workspace_floats(B, N) * sizeof(float) ||
      gan_ws_bytes < acoustic_gan_workspace_bytes(B, N, step_mask != 0)) {
    set_error("sty_acoustic_gan_loss_fwd_bwd: workspace too small");
    return STY_ENOMEM;
  }
  AcousticGan gan;
  for (int r = 0; r < 3; ++r) {
    for (int i = 0; i < 10; ++i)
      if (!mrd[r].g[i] || !mrd[r].v[i] || !mrd[r].bias[i] ||
          (((step_mask >> r) & 1) && (!mrd_grads[r].g[i] || !mrd_grads[r].v[i] || !mrd_grads[r].bias[i]))) {
        set_error("sty_acoustic_gan_loss_fwd_bwd: null parameter / gradient pointer (discriminator %d, conv %d)", r, i);
        return STY_EINVAL;
      }
    gan.p[r] = &mrd[r];
    gan.g[r] = ((step_mask >> r) & 1) ? &mrd_grads[r] : nullptr;
  }
  gan.w_gen = w_gen;
  gan.disc_scale = disc_scale;
  gan.out = gan_losses;
  gan.bf16 = compute_bf16;
  gan.ws = gan_workspace;
  gan.ws_bytes = gan_ws_bytes;
  STY_HIP(hipMemsetAsync(gan_losses, 0, 7 * sizeof(float), S(stream)));
  return launch_acoustic_loss_gan(B, N, audio_gt, audio_pred, w_mel, w_phase, losses, d_audio_pred, (float*)workspace, &gan,
                                  S(stream));
}

}  // extern "C"
