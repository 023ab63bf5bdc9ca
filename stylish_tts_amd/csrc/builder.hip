// Model objects: the Builder, which turns the bound state_dict into a model's plans and packed weights, the model life
// cycle entries around it, and the readiness checks every model-bound entry starts with (run.h).
#include "run.h"

namespace sty {

// ---------------------------------------------------------------------------------------------------
// parameter lookup
// ---------------------------------------------------------------------------------------------------
struct Builder {
  sty_model* m;
  bool dry;  // first pass: only measure the arena and collect the key list
  bool ok = true;

  const Param* get(const std::string& key, std::initializer_list<int64_t> shape = {}) {
    if (dry) m->requested.push_back(key);
    auto it = m->params.find(key);
    if (it == m->params.end()) {
      if (ok) m->missing = key;
      ok = false;
      return nullptr;
    }
    if (shape.size()) {
      std::vector<int64_t> want(shape);
      if (want != it->second.shape) {
        if (ok) m->missing = key + " (shape mismatch)";
        ok = false;
        return nullptr;
      }
    }
    return &it->second;
  }
  const float* ptr(const std::string& key, std::initializer_list<int64_t> shape = {}) {
    const Param* p = get(key, shape);
    return p ? p->p : nullptr;
  }
  bool has(const std::string& key) const { return m->params.count(key) != 0; }

  // dense conv / linear -> PackedConv (+ pack job).  wn: weight_norm parametrization.  glu: GLU channel order.
  PackedConv conv(const std::string& name, bool wn = false, bool bias = true, bool glu = false,
                  const float* bias_override_src = nullptr) {
    PackedConv pc;
    const Param* w = wn ? get(name + ".parametrizations.weight.original1") : get(name + ".weight");
    const Param* g = wn ? get(name + ".parametrizations.weight.original0") : nullptr;
    const float* b = bias ? ptr(name + ".bias") : nullptr;
    if (!w || (wn && !g)) return pc;
    const auto& s = w->shape;
    pc.Cout = (int)s[0];
    pc.Cin = (int)s[1];
    pc.K = s.size() > 2 ? (int)s[2] : 1;
    pc.CinP = (int)align_up(pc.Cin, CI_CHUNK);
    pc.CoutP = glu ? (int)align_up(pc.Cout, 64) : (int)align_up(pc.Cout, 32);
    float* wp = m->ab.take<float>((size_t)pc.K * pc.CinP * pc.CoutP);
    float* bp = m->ab.take<float>(pc.CoutP);
    pc.wp = wp;
    pc.bias = (bias || bias_override_src) ? bp : nullptr;
    float* w3 = nullptr;
    if (m->fp32_split && pc.CinP == CI_CHUNK && pc.CoutP == 32 && !glu) {  // the split mode's fragment triples (conv32p.hip)
      w3 = m->ab.take<float>(split3_bytes(pc.K) / sizeof(float));
      pc.w3 = w3;
    }
    if (!dry)
      m->jobs.push_back(PackJob::conv(glu ? PK_CONV_GLU : (wn ? PK_CONV_WN : PK_CONV), pc, wn ? nullptr : w->p,
                                      g ? g->p : nullptr, wn ? w->p : nullptr, b, wp, bp));
    if (!dry && w3) m->jobs.push_back(PackJob::split3(pc, w3));
    if (m->train_enabled || m->kind == "wavlm") {  // (wavlm: frozen, but its input-gradient chain is built)
      if (glu) {  // the training graph runs GLU as a separate op: it needs the plain channel order
        PackedConv pl = pc;
        pl.CoutP = (int)align_up(pc.Cout, 32);
        float* wp2 = m->ab.take<float>((size_t)pc.K * pc.CinP * pl.CoutP);
        float* bp2 = m->ab.take<float>(pl.CoutP);
        pl.wp = wp2;
        pl.bias = bias ? bp2 : nullptr;
        if (!dry) {
          m->jobs.push_back(PackJob::conv(PK_CONV, pl, w->p, nullptr, nullptr, b, wp2, bp2));
          m->plain_of[wp] = pl;
        }
        add_dgrad(pl);
      } else {
        add_dgrad(pc);
      }
    }
    return pc;
  }

  // input-gradient weights Wd[k'][co][ci] = Wp[K-1-k'][ci][co] of a packed conv (prepared after the pack jobs)
  PackedConv dgrad_shape(const PackedConv& pc) {
    PackedConv d;
    d.Cin = pc.Cout;
    d.CinP = pc.CoutP;
    d.Cout = pc.Cin;
    d.CoutP = pc.CinP;
    d.K = pc.K;
    d.wp = m->ab.take<float>((size_t)pc.K * pc.CinP * pc.CoutP);
    d.bias = nullptr;
    return d;
  }
  void add_dgrad(const PackedConv& pc) {
    const PackedConv d = dgrad_shape(pc);
    float* wd = const_cast<float*>(d.wp);
    if (!dry) {
      m->jobs.push_back(PackJob::dgrad(pc, wd));
      m->dgrad[pc.wp] = d;
    }
  }

  AdaFc fc(const std::string& name, int C) {
    AdaFc a;
    a.C = C;
    const float* W = ptr(name + ".fc.weight", {2 * C, m->style_dim});
    const float* b = ptr(name + ".fc.bias", {2 * C});
    a.off = m->gb_floats_per_batch;
    m->gb_floats_per_batch += 2 * C;
    if (!dry) {
      a.idx = (int)m->fcs.size();
      StyleFcDesc d;
      d.W = W;
      d.b = b;
      d.off = a.off;
      d.n = 2 * C;
      d.pad = 0;
      m->fcs.push_back(d);
    }
    return a;
  }

  ConvNeXt convnext(const std::string& p, int C, bool snake = true) {
    ConvNeXt c;
    c.C = C;
    c.dw_w = ptr(p + ".dwconv.weight", {C, 1, 7});
    c.dw_b = ptr(p + ".dwconv.bias", {C});
    c.norm = fc(p + ".norm", C);
    // GeneratorConvNeXtBlock has a snake parameter; AdaptiveConvNeXtBlock (duration predictor) uses GELU instead
    c.alpha = snake ? ptr(p + ".snake", {1, 1, 4 * C}) : nullptr;
    c.grn_gamma = ptr(p + ".grn.gamma", {1, 1, 4 * C});
    const float* grn_beta = ptr(p + ".grn.beta", {1, 1, 4 * C});
    c.b1 = ptr(p + ".pwconv1.bias", {4 * C});
    const float* w2 = ptr(p + ".pwconv2.weight", {C, 4 * C});
    const float* b2 = ptr(p + ".pwconv2.bias", {C});
    c.pw1 = conv(p + ".pwconv1");
    c.w1p = c.pw1.wp;
    c.w1_raw = ptr(p + ".pwconv1.weight", {4 * C, C});
    c.w2_raw = w2;
    // pw2: packed conv with bias := b2eff (written by the W2A job)
    PackedConv pc;
    pc.Cout = C;
    pc.Cin = 4 * C;
    pc.K = 1;
    pc.CinP = 4 * C;
    pc.CoutP = (int)align_up(C, 32);
    float* wp = m->ab.take<float>((size_t)pc.CinP * pc.CoutP);
    float* bp = m->ab.take<float>(pc.CoutP);
    float* w2a = m->ab.take<float>((size_t)4 * C * C);
    pc.wp = wp;
    pc.bias = bp;
    c.pw2 = pc;
    c.w2a = w2a;
    if (!dry && w2) {
      m->jobs.push_back(PackJob::conv(PK_CONV, pc, w2, nullptr, nullptr, nullptr, wp, nullptr));
      m->jobs.push_back(PackJob::w2a(w2, b2, grn_beta, C, w2a, bp));
    }
    if (m->train_enabled) add_dgrad(pc);
    return c;
  }

  ResBlock32 resblock(const std::string& p) {
    ResBlock32 r;
    for (int i = 0; i < 3; ++i) {
      const std::string si = std::to_string(i);
      r.c1[i] = conv(p + ".convs1." + si, true);
      r.c2[i] = conv(p + ".convs2." + si, true);
      r.n1[i] = fc(p + ".adain1." + si, 32);
      r.n2[i] = fc(p + ".adain2." + si, 32);
      r.a1[i] = ptr(p + ".alpha1." + si, {1, 32, 1});
      r.a2[i] = ptr(p + ".alpha2." + si, {1, 32, 1});
    }
    return r;
  }

  void vocoder(const std::string& g) {
    VocoderPlan& v = m->voc;
    v.amp_input_conv = conv(g + "amp_input_conv");
    const int hd = v.amp_input_conv.Cout ? v.amp_input_conv.Cout : 256;
    v.hidden = hd;
    v.amp_norm_w = ptr(g + "amp_norm.weight", {hd});
    v.amp_norm_b = ptr(g + "amp_norm.bias", {hd});
    const std::string c = g + "amp_conformer.layers.0.";
    Conformer& cf = v.conf;
    cf.ff1n = fc(c + "ff1.fn.norm", hd);
    cf.ff1a = conv(c + "ff1.fn.fn.net.0");
    cf.ff1b = conv(c + "ff1.fn.fn.net.3");
    cf.attn_n = fc(c + "attn.norm", hd);
    cf.to_q = conv(c + "attn.fn.to_q", false, false);
    cf.to_kv = conv(c + "attn.fn.to_kv", false, false);
    cf.to_out = conv(c + "attn.fn.to_out");
    cf.conv_n = fc(c + "conv.norm", hd);
    cf.pw1 = conv(c + "conv.net.1", false, true, true);
    cf.dw_w = ptr(c + "conv.net.3.conv.weight", {2 * hd, 1, 31});
    cf.dw_b = ptr(c + "conv.net.3.conv.bias", {2 * hd});
    cf.bn_w = ptr(c + "conv.net.4.weight", {2 * hd});
    cf.bn_b = ptr(c + "conv.net.4.bias", {2 * hd});
    cf.bn_rm = ptr(c + "conv.net.4.running_mean", {2 * hd});
    cf.bn_rv = ptr(c + "conv.net.4.running_var", {2 * hd});
    cf.pw2 = conv(c + "conv.net.6");
    cf.ff2n = fc(c + "ff2.fn.norm", hd);
    cf.ff2a = conv(c + "ff2.fn.fn.net.0");
    cf.ff2b = conv(c + "ff2.fn.fn.net.3");
    cf.post_n = fc(c + "post_norm", hd);
    const std::string b = g + "basegen.";
    v.amp_convnext.clear();
    for (int i = 0; has(b + "amp_convnext." + std::to_string(i) + ".dwconv.weight"); ++i)
      v.amp_convnext.push_back(convnext(b + "amp_convnext." + std::to_string(i), hd));
    int after = hd;
    for (int i = 0; i < 3; ++i) {
      after /= 2;
      v.upconv[i] = conv(b + "upconvs." + std::to_string(i));
      v.upblock[i] = convnext(b + "upblocks." + std::to_string(i), after);
    }
    v.lin_w = ptr(b + "m_source.l_linear.weight", {1, 9});
    v.lin_b = ptr(b + "m_source.l_linear.bias", {1});
    // STFT bases are deterministic buffers; use the bound ones when present, else the built-in table
    v.stft_fr = has(b + "stft.weight_forward_real") ? ptr(b + "stft.weight_forward_real", {33, 1, 64}) : m->stft_default;
    v.stft_fi = has(b + "stft.weight_forward_imag") ? ptr(b + "stft.weight_forward_imag", {33, 1, 64})
                                                     : m->stft_default + 33 * 64;
    v.stft_br = has(b + "stft.weight_backward_real") ? ptr(b + "stft.weight_backward_real", {33, 1, 64})
                                                      : m->stft_default + 2 * 33 * 64;
    v.stft_bi = has(b + "stft.weight_backward_imag") ? ptr(b + "stft.weight_backward_imag", {33, 1, 64})
                                                      : m->stft_default + 3 * 33 * 64;
    v.amp_prior_conv = conv(b + "amp_prior_conv");
    v.phase_prior_conv = conv(b + "phase_prior_conv");
    v.amp_prior_block = resblock(b + "amp_prior_block");
    v.phase_prior_block = resblock(b + "phase_prior_block");
    v.phase_input_conv = conv(b + "phase_input_conv");
    v.amp_output_conv = conv(b + "amp_output_conv");
    v.real_conv = conv(b + "phase_output_real_conv");
    v.imag_conv = conv(b + "phase_output_imag_conv");
    v.phase_norm_w = ptr(b + "phase_norm.weight", {32});
    v.phase_norm_b = ptr(b + "phase_norm.bias", {32});
    v.amp_fln_w = ptr(b + "amp_final_layer_norm.weight", {32});
    v.amp_fln_b = ptr(b + "amp_final_layer_norm.bias", {32});
    v.phase_fln_w = ptr(b + "phase_final_layer_norm.weight", {32});
    v.phase_fln_b = ptr(b + "phase_final_layer_norm.bias", {32});
    v.phase_convnext.clear();
    for (int i = 0; has(b + "phase_convnext." + std::to_string(i) + ".dwconv.weight"); ++i)
      v.phase_convnext.push_back(convnext(b + "phase_convnext." + std::to_string(i), 32));
    if (ok && (v.amp_convnext.empty() || v.phase_convnext.empty())) {
      m->missing = b + "amp_convnext.0 / phase_convnext.0";
      ok = false;
    }
  }

  void text_encoder(const std::string& p) {
    TextEncPlan& t = m->te;
    const Param* e = get(p + "emb.weight");
    if (!e) return;
    t.emb = e->p;
    t.tokens = (int)e->shape[0];
    t.H = (int)e->shape[1];
    for (int i = 0; i < 3; ++i) {
      const std::string si = std::to_string(i);
      t.pre[i] = conv(p + "prenet.conv_layers." + si);
      t.pre_g[i] = ptr(p + "prenet.norm_layers." + si + ".gamma", {t.H});
      t.pre_b[i] = ptr(p + "prenet.norm_layers." + si + ".beta", {t.H});
    }
    t.proj = conv(p + "prenet.proj");
    t.layers.clear();
    for (int i = 0; has(p + "encoder.attn_layers." + std::to_string(i) + ".conv_q.weight"); ++i) {
      const std::string si = std::to_string(i);
      TextEncLayer l;
      l.q = conv(p + "encoder.attn_layers." + si + ".conv_q");
      l.k = conv(p + "encoder.attn_layers." + si + ".conv_k");
      l.v = conv(p + "encoder.attn_layers." + si + ".conv_v");
      l.o = conv(p + "encoder.attn_layers." + si + ".conv_o");
      l.n1g = ptr(p + "encoder.norm_layers_1." + si + ".gamma", {t.H});
      l.n1b = ptr(p + "encoder.norm_layers_1." + si + ".beta", {t.H});
      l.f1 = conv(p + "encoder.ffn_layers." + si + ".conv_1");
      l.f2 = conv(p + "encoder.ffn_layers." + si + ".conv_2");
      l.n2g = ptr(p + "encoder.norm_layers_2." + si + ".gamma", {t.H});
      l.n2b = ptr(p + "encoder.norm_layers_2." + si + ".beta", {t.H});
      t.layers.push_back(l);
    }
    t.proj_m = conv(p + "proj_m");
    for (int i = 0; i < 4; ++i) t.theta[i] = 1.0f / powf(10000.0f, (float)(2 * i) / 8.0f);
  }

  DecBlock dec_block(const std::string& p) {
    DecBlock d;
    d.c1 = conv(p + ".conv1", true);
    d.c2 = conv(p + ".conv2", true);
    d.Cin = d.c1.Cin;
    d.Cout = d.c1.Cout;
    d.n1 = fc(p + ".norm1", d.Cin);
    d.n2 = fc(p + ".norm2", d.Cout);
    d.has_sc = has(p + ".conv1x1.parametrizations.weight.original0");
    if (d.has_sc) d.sc = conv(p + ".conv1x1", true, false);
    return d;
  }

  void decoder(const std::string& p) {
    DecoderPlan& d = m->dec;
    d.encode = dec_block(p + "encode");
    for (int i = 0; i < 4; ++i) d.decode[i] = dec_block(p + "decode." + std::to_string(i));
    d.asr_res = conv(p + "asr_res.0", true);
    d.f0_g = ptr(p + "F0_conv.parametrizations.weight.original0", {1, 1, 1});
    d.f0_v = ptr(p + "F0_conv.parametrizations.weight.original1", {1, 1, 3});
    d.f0_b = ptr(p + "F0_conv.bias", {1});
    d.n_g = ptr(p + "N_conv.parametrizations.weight.original0", {1, 1, 1});
    d.n_v = ptr(p + "N_conv.parametrizations.weight.original1", {1, 1, 3});
    d.n_b = ptr(p + "N_conv.bias", {1});
    d.v_g = ptr(p + "voiced_conv.parametrizations.weight.original0", {1, 1, 1});
    d.v_v = ptr(p + "voiced_conv.parametrizations.weight.original1", {1, 1, 3});
    d.v_b = ptr(p + "voiced_conv.bias", {1});
    d.fnv_w = m->ab.take<float>(12);
  }

  // spectral-normed Conv2d [Cout][Cin][KH][KW] -> PackedConv in 2-D mode (reduction index (kh, ci), K = KW)
  PackedConv conv2d_sn(const std::string& name, bool bias = true) {
    PackedConv pc;
    const Param* w = get(name + ".weight_orig");
    const float* u = ptr(name + ".weight_u");
    const float* v = ptr(name + ".weight_v");
    const float* b = bias ? ptr(name + ".bias") : nullptr;
    if (!w || w->shape.size() != 4) return pc;
    const int Cout = (int)w->shape[0], Cin = (int)w->shape[1], KH = (int)w->shape[2], KW = (int)w->shape[3];
    pc.Cout = Cout;
    pc.Cin = KH * Cin;
    pc.K = KW;
    pc.CinP = (int)align_up(pc.Cin, CI_CHUNK);
    pc.CoutP = (int)align_up(Cout, 32);
    float* wp = m->ab.take<float>((size_t)KW * pc.CinP * pc.CoutP);
    float* bp = m->ab.take<float>(pc.CoutP);
    float* ts = m->ab.take<float>(Cout);
    float* ts2 = m->train_enabled ? m->ab.take<float>(sn_power_iter_scratch_floats(Cout, Cin * KH * KW)) : nullptr;
    pc.wp = wp;
    pc.bias = bias ? bp : nullptr;
    if (!dry) m->jobs.push_back(PackJob::conv2d_sn(pc, Cin, KH, w->p, u, v, b, wp, bp, ts, ts2));
    if (m->train_enabled) {  // input-gradient weights: rows (kh', co), columns ci, taps flipped in both directions
      PackedConv d;
      d.Cin = KH * Cout;
      d.CinP = (int)align_up(d.Cin, CI_CHUNK);
      d.Cout = Cin;
      d.CoutP = (int)align_up(Cin, 32);
      d.K = KW;
      float* wd = m->ab.take<float>((size_t)KW * d.CinP * d.CoutP);
      d.wp = wd;
      d.bias = nullptr;
      if (!dry) {
        m->jobs.push_back(PackJob::dgrad2d(pc, Cin, KH, wd));
        m->dgrad[wp] = d;
      }
    }
    return pc;
  }

  void style_encoder() {
    StylePlan& sp = m->sty_enc;
    sp.stem = conv2d_sn("shared.0");
    sp.n_mels = sp.stem.Cout ? sp.stem.Cout : 80;
    for (int i = 0; i < 4; ++i) {
      const std::string p = "shared." + std::to_string(i + 1);
      StyleResBlk& r = sp.blk[i];
      r.c1 = conv2d_sn(p + ".conv1");
      r.c2 = conv2d_sn(p + ".conv2");
      r.Cin = r.c1.Cout;
      r.Cout = r.c2.Cout;
      r.has_sc = has(p + ".conv1x1.weight_orig");
      if (r.has_sc) r.sc = conv2d_sn(p + ".conv1x1", false);
      r.down = has(p + ".downsample_res.conv.weight_orig");
      if (r.down) {
        const std::string d = p + ".downsample_res.conv";
        const float* w = ptr(d + ".weight_orig", {r.Cin, 1, 3, 3});
        const float* u = ptr(d + ".weight_u", {r.Cin});
        const float* v = ptr(d + ".weight_v", {9});
        r.dw_b = ptr(d + ".bias", {r.Cin});
        float* w9 = m->ab.take<float>((size_t)r.Cin * 9);
        float* ts = m->ab.take<float>(r.Cin);
        float* ts2 = m->train_enabled ? m->ab.take<float>(sn_power_iter_scratch_floats(r.Cin, 9)) : nullptr;
        r.dw_w9 = w9;
        if (!dry) m->jobs.push_back(PackJob::dw2d_sn(r.Cin, w, u, v, w9, ts, ts2));
      }
    }
    sp.head = conv2d_sn("shared.6");
    const Param* fw = get("unshared.weight");
    sp.fc_w = fw ? fw->p : nullptr;
    sp.style_dim = fw ? (int)fw->shape[0] : 64;
    sp.fc_b = ptr("unshared.bias");
  }

  // DurationPredictor (duration_predictor.py:16-58)
  void duration_predictor() {
    text_encoder("text_encoder.");
    DurationPlan& d = m->dur;
    const int C = m->te.proj_m.Cout;
    d.cnx.clear();
    for (int i = 0; has("conv_next." + std::to_string(i) + ".dwconv.weight"); ++i)
      d.cnx.push_back(convnext("conv_next." + std::to_string(i), C, false));
    d.proj = conv("duration_proj.linear_layer");
    d.classes = d.proj.Cout;
    d.qn = fc("query_norm", C);
    d.kn = fc("key_norm", C);
    d.cq = conv("cross_attention.conv_q");
    d.ck = conv("cross_attention.conv_k");
    d.cv = conv("cross_attention.conv_v");
    d.co = conv("cross_attention.conv_o");
    d.dw_g = ptr("cross_post.0.parametrizations.weight.original0", {C, 1, 1});
    d.dw_v = ptr("cross_post.0.parametrizations.weight.original1", {C, 1, 5});
    d.dw_b = ptr("cross_post.0.bias", {C});
    d.post = conv("cross_post.2", true);
  }
  // PitchEnergyPredictor (pitch_energy_predictor.py:8-60)
  void pitch_energy_predictor() {
    text_encoder("text_encoder.");
    PitchEnergyPlan& p = m->pe;
    const int hc = m->te.proj_m.Cout + m->style_dim;
    p.layers.clear();
    const std::string pre = "prosody_encoder.";
    for (int i = 0; has(pre + "attn_layers." + std::to_string(i) + ".conv_q.weight"); ++i) {
      const std::string si = std::to_string(i);
      ProsodyLayer l;
      l.q = conv(pre + "attn_layers." + si + ".conv_q");
      l.k = conv(pre + "attn_layers." + si + ".conv_k");
      l.v = conv(pre + "attn_layers." + si + ".conv_v");
      l.o = conv(pre + "attn_layers." + si + ".conv_o");
      l.n1 = fc(pre + "norm_layers_1." + si, hc);
      l.f1 = conv(pre + "ffn_layers." + si + ".conv_1");
      l.f2 = conv(pre + "ffn_layers." + si + ".conv_2");
      l.n2 = fc(pre + "norm_layers_2." + si, hc);
      l.proj = conv(pre + "proj_layers." + si);
      p.layers.push_back(l);
    }
    for (int i = 0; i < 4; ++i) {
      p.f0[i] = dec_block("F0." + std::to_string(i));
      p.nn[i] = dec_block("N." + std::to_string(i));
    }
    p.f0p = conv("F0_proj");
    p.np = conv("N_proj");
  }

  // TextAligner (text_aligner.py:33-45, 130-274): dimensions from the bound shapes
  void text_aligner() {
    AlignerPlan& a = m->ali;
    static const int kernel[3] = {5, 3, 3};
    for (int i = 0; i < 3; ++i) {
      const std::string p = "encoder.layers." + std::to_string(i);
      a.tdnn[i] = conv(p + ".0");
      const int C = a.tdnn[i].Cout;
      if (ok && (a.tdnn[i].K != kernel[i] || (i > 0 && (a.tdnn[i].Cin != a.hidden || C != a.hidden)))) {
        m->missing = p + ".0.weight (shape mismatch)";
        ok = false;
      }
      if (i == 0) {
        a.hidden = C;
        a.n_mels = a.tdnn[0].Cin;
      }
      a.rm[i] = ptr(p + ".2.running_mean", {C});
      a.rv[i] = ptr(p + ".2.running_var", {C});
      a.bn_scale[i] = m->ab.take<float>(C);
      a.bn_shift[i] = m->ab.take<float>(C);
    }
    if (m->kind == "text_aligner_train") {  // BatchNorm1d(affine=False) for kernels that take a weight and a bias
      a.bn_one = m->ab.take<float>(a.hidden);
      a.bn_zero = m->ab.take<float>(a.hidden);
    }
    for (int i = 0; i < 5; ++i) {
      const std::string p = "encoder.layers.3.ffn." + std::to_string(3 * i);
      a.ffn[i] = conv(p);
      if (ok && (a.ffn[i].K != 1 || a.ffn[i].Cin != a.hidden || a.ffn[i].Cout != a.hidden)) {
        m->missing = p + ".weight (shape mismatch)";
        ok = false;
      }
    }
    a.out = conv("encoder_output_layer");
    if (ok && (a.out.K != 1 || a.out.Cin != a.hidden || a.out.Cout < 2)) {
      m->missing = "encoder_output_layer.weight (shape mismatch)";
      ok = false;
    }
    a.classes = a.out.Cout;
  }

  // ---- RMVPE (train/dataprep/rmvpe/model.py:49-86): n_blocks, inter_layers and en_out_channels from the bound keys / shapes ----
  void rm_fail(const std::string& key) {
    if (ok) m->missing = key + " (shape mismatch)";
    ok = false;
  }
  // Conv2d [Cout][Cin][KH][KW] (+ the BatchNorm `bn` behind it, + bias) -> PackedConv in 2-D mode, packed by rmvpe_pack_conv_kernel
  PackedConv rm_conv2d(const std::string& name, const std::string& bn, bool bias, int Cin, int Cout, int KH) {
    PackedConv pc;
    RmvpePackJob j;
    j.w = ptr(name + ".weight", {Cout, Cin, KH, KH});
    if (bias) j.bias = ptr(name + ".bias", {Cout});
    if (!bn.empty()) {
      j.bn_w = ptr(bn + ".weight", {Cout});
      j.bn_b = ptr(bn + ".bias", {Cout});
      j.bn_rm = ptr(bn + ".running_mean", {Cout});
      j.bn_rv = ptr(bn + ".running_var", {Cout});
    }
    pc.Cout = Cout, pc.Cin = KH * Cin, pc.K = KH;
    pc.CinP = (int)align_up(pc.Cin, CI_CHUNK), pc.CoutP = (int)align_up(Cout, 32);
    j.wp = m->ab.take<float>((size_t)pc.K * pc.CinP * pc.CoutP);
    j.bp = m->ab.take<float>(pc.CoutP);
    j.Cout = Cout, j.Cin = Cin, j.KH = KH, j.KW = KH, j.CinP = pc.CinP, j.CoutP = pc.CoutP;
    pc.wp = j.wp, pc.bias = j.bp;
    if (!dry && ok) m->rmv.packs.push_back(j);
    return pc;
  }
  RmvpeBlock rm_block(const std::string& p, int Cin, int Cout) {
    RmvpeBlock b;
    b.Cin = Cin, b.Cout = Cout;
    b.c1 = rm_conv2d(p + ".conv.0", p + ".conv.1", false, Cin, Cout, 3);
    b.c2 = rm_conv2d(p + ".conv.3", p + ".conv.4", false, Cout, Cout, 3);
    b.has_sc = Cin != Cout;
    if (b.has_sc) b.sc = rm_conv2d(p + ".shortcut", "", true, Cin, Cout, 1);
    return b;
  }
  void rmvpe() {
    RmvpePlan& p = m->rmv;
    if (!dry) p.packs.clear();
    const std::string e = "unet.encoder.", im = "unet.intermediate.", d = "unet.decoder.";
    const Param* w0 = get(e + "layers.0.conv.0.conv.0.weight");
    if (!w0) return;
    if (w0->shape.size() != 4 || w0->shape[1] != 1 || w0->shape[0] < 1) return rm_fail(e + "layers.0.conv.0.conv.0.weight");
    p.C0 = (int)w0->shape[0];
    p.n_blocks = 0;
    while (has(e + "layers.0.conv." + std::to_string(p.n_blocks) + ".conv.0.weight")) ++p.n_blocks;
    p.inter_layers = 0;
    while (has(im + "layers." + std::to_string(p.inter_layers) + ".conv.0.conv.0.weight")) ++p.inter_layers;
    if (p.inter_layers < 1) return rm_fail(im + "layers.0.conv.0.conv.0.weight");
    static const char* bn_part[4] = {"weight", "bias", "running_mean", "running_var"};
    for (int i = 0; i < 4; ++i) p.in_bn[i] = ptr(e + "bn." + bn_part[i], {1});
    p.in_ss = m->ab.take<float>(2);
    int cin = 1, c = p.C0;
    for (int l = 0; l < RMVPE_LEVELS; ++l) {
      p.enc[l].clear();
      for (int j = 0; j < p.n_blocks; ++j)
        p.enc[l].push_back(rm_block(e + "layers." + std::to_string(l) + ".conv." + std::to_string(j), j ? c : cin, c));
      cin = c;
      c *= 2;
    }
    // (c = 2 * the deepest encoder width = the intermediate's width)
    p.inter.clear();
    for (int i = 0; i < p.inter_layers; ++i)
      for (int j = 0; j < p.n_blocks; ++j)
        p.inter.push_back(rm_block(im + "layers." + std::to_string(i) + ".conv." + std::to_string(j), (i || j) ? c : cin, c));
    for (int i = 0; i < RMVPE_LEVELS; ++i) {
      const std::string dl = d + "layers." + std::to_string(i);
      const int co = c / 2;
      RmvpeUp& u = p.up[i];
      u.Cin = c, u.Cout = co;
      RmvpePackJob j;
      j.w = ptr(dl + ".conv1.0.weight", {c, co, 3, 3});
      j.bn_w = ptr(dl + ".conv1.1.weight", {co});
      j.bn_b = ptr(dl + ".conv1.1.bias", {co});
      j.bn_rm = ptr(dl + ".conv1.1.running_mean", {co});
      j.bn_rv = ptr(dl + ".conv1.1.running_var", {co});
      j.wp = m->ab.take<float>((size_t)c * co * 9);
      j.bp = m->ab.take<float>(co);
      j.Cout = co, j.Cin = c, j.KH = 3, j.KW = 3, j.deconv = 1;
      u.wd = j.wp, u.bias = j.bp;
      if (!dry && ok) p.packs.push_back(j);
      p.dec[i].clear();
      for (int k = 0; k < p.n_blocks; ++k) p.dec[i].push_back(rm_block(dl + ".conv2." + std::to_string(k), k ? co : 2 * co, co));
      c = co;
    }
    p.cnn = rm_conv2d("cnn", "", true, p.C0, 3, 3);
    {  // nn.GRU(384, 256, bidirectional): both directions' W_ih x + b_ih as one K = 1 conv of 1536 rows
      const int nin = 3 * RMVPE_MELS, H3 = 768;
      PackedConv pc;
      pc.Cin = nin, pc.Cout = 2 * H3, pc.K = 1, pc.CinP = (int)align_up(nin, CI_CHUNK), pc.CoutP = (int)align_up(2 * H3, 32);
      float* wp = m->ab.take<float>((size_t)pc.CinP * pc.CoutP);
      float* bp = m->ab.take<float>(pc.CoutP);
      pc.wp = wp, pc.bias = bp;
      for (int r = 0; r < 2; ++r) {
        const std::string sfx = r ? "_l0_reverse" : "_l0";
        RmvpePackJob j;
        j.w = ptr("fc.0.gru.weight_ih" + sfx, {H3, nin});
        j.bias = ptr("fc.0.gru.bias_ih" + sfx, {H3});
        j.wp = wp, j.bp = bp;
        j.Cout = H3, j.Cin = nin, j.CinP = pc.CinP, j.CoutP = pc.CoutP, j.co_off = r * H3;
        if (!dry && ok) p.packs.push_back(j);
        p.whh[r] = ptr("fc.0.gru.weight_hh" + sfx, {H3, 256});
        p.bhh[r] = ptr("fc.0.gru.bias_hh" + sfx, {H3});
      }
      p.gru_ih = pc;
      p.whhT = m->ab.take<float>((size_t)2 * H3 * 256);
    }
    p.head = conv("fc.1");
    if (ok && (p.head.Cin != 512 || p.head.Cout != RMVPE_CLASSES || p.head.K != 1)) rm_fail("fc.1.weight");
  }

  // ---- WavLM (transformers' WavLMModel): widths, depths, heads, kernels, groups and num_buckets from the bound shapes; the
  //      strides, max_bucket_distance and layer_norm_eps from sty_wavlm_set_config ----
  void wavlm() {
    WavlmPlan& p = m->wav;
    if (!dry) p.packs.clear();
    p.layers.clear();
    p.pos.clear();
    p.pos_d.clear();
    m->wav_keep = WavlmKeep();
    if (p.n_conv < 2) {
      if (ok) m->missing = "the conv strides (sty_wavlm_set_config was not called)";
      ok = false;
      return;
    }
    const std::string fe = "feature_extractor.conv_layers.";
    int cin = 1;
    for (int i = 0; i < p.n_conv; ++i) {
      const std::string key = fe + std::to_string(i) + ".conv.weight";
      const Param* w = get(key);
      if (!w) return;
      if (w->shape.size() != 3 || w->shape[1] != cin || w->shape[2] < 1) return rm_fail(key);
      const int C = (int)w->shape[0], k = (int)w->shape[2], s = p.stride[i];
      p.dim[i] = C, p.kern[i] = k;
      if (i == 0) {
        p.conv0_w = w->p;
        p.gn_w = ptr(fe + "0.layer_norm.weight", {C});
        p.gn_b = ptr(fe + "0.layer_norm.bias", {C});
      } else {
        PackedConv pc;
        pc.Cin = s * cin, pc.Cout = C, pc.K = cdiv(k, s);
        pc.CinP = (int)align_up(pc.Cin, CI_CHUNK), pc.CoutP = (int)align_up(C, 32);
        WavlmPackJob j;
        j.w = w->p;
        j.wp = m->ab.take<float>((size_t)pc.K * pc.CinP * pc.CoutP);
        j.Cout = C, j.Cin = cin, j.K = k, j.s = s, j.CinP = pc.CinP, j.CoutP = pc.CoutP;
        pc.wp = j.wp;
        p.conv[i] = pc;
        p.conv_d[i] = dgrad_shape(pc);
        if (!dry && ok) p.packs.push_back(j);
      }
      cin = C;
    }
    p.fp_ln_w = ptr("feature_projection.layer_norm.weight", {cin});
    p.fp_ln_b = ptr("feature_projection.layer_norm.bias", {cin});
    p.proj = conv("feature_projection.projection");
    if (!ok) return;
    if (p.proj.Cin != cin || p.proj.K != 1) return rm_fail("feature_projection.projection.weight");
    const int H = p.hidden = p.proj.Cout;
    {
      const std::string pc_ = "encoder.pos_conv_embed.conv.";
      const Param* v = get(pc_ + "parametrizations.weight.original1");
      if (!v) return;
      if (v->shape.size() != 3 || v->shape[0] != H || v->shape[1] < 1 || H % v->shape[1]) return rm_fail(pc_ + "parametrizations.weight.original1");
      const int Cg = (int)v->shape[1], K = (int)v->shape[2];
      p.pos_k = K, p.pos_groups = H / Cg, p.pos_v = v->p;
      if (K - 1 > 128) return rm_fail(pc_ + "parametrizations.weight.original1 (more than 129 taps)");
      const float* g = ptr(pc_ + "parametrizations.weight.original0", {1, 1, K});
      const float* bias = ptr(pc_ + "bias", {H});
      p.pos_nrm = m->ab.take<float>(K);
      for (int gi = 0; gi < p.pos_groups; ++gi) {
        PackedConv pc;
        pc.Cin = pc.Cout = Cg, pc.K = K;
        pc.CinP = (int)align_up(Cg, CI_CHUNK), pc.CoutP = (int)align_up(Cg, 32);
        WavlmPackJob j;
        j.w = v->p, j.g = g, j.nrm = p.pos_nrm, j.bias = bias;
        j.wp = m->ab.take<float>((size_t)K * pc.CinP * pc.CoutP);
        j.bp = m->ab.take<float>(pc.CoutP);
        j.Cout = Cg, j.Cin = Cg, j.K = K, j.s = 1, j.CinP = pc.CinP, j.CoutP = pc.CoutP, j.co0 = gi * Cg;
        pc.wp = j.wp, pc.bias = j.bp;
        p.pos.push_back(pc);
        p.pos_d.push_back(dgrad_shape(pc));
        if (!dry && ok) p.packs.push_back(j);
      }
    }
    p.enc_ln_w = ptr("encoder.layer_norm.weight", {H});
    p.enc_ln_b = ptr("encoder.layer_norm.bias", {H});
    const Param* emb = get("encoder.layers.0.attention.rel_attn_embed.weight");
    if (!emb) return;
    if (emb->shape.size() != 2 || emb->shape[0] < 4 || emb->shape[1] < 1 || H % emb->shape[1]) return rm_fail("encoder.layers.0.attention.rel_attn_embed.weight");
    p.num_buckets = (int)emb->shape[0], p.heads = (int)emb->shape[1], p.rel_embed = emb->p;
    if (p.max_distance <= p.num_buckets / 4) {  // (the bucket function divides by log(max_distance / (num_buckets / 4)))
      if (ok) m->missing = "max_bucket_distance " + std::to_string(p.max_distance) + " must exceed num_buckets / 4 = " + std::to_string(p.num_buckets / 4) + " (shape mismatch)";
      ok = false;
      return;
    }
    const int DH = H / p.heads;
    for (int l = 0; has("encoder.layers." + std::to_string(l) + ".attention.q_proj.weight"); ++l) {
      const std::string pl = "encoder.layers." + std::to_string(l) + ".";
      WavlmLayer y;
      y.q = conv(pl + "attention.q_proj");
      y.k = conv(pl + "attention.k_proj");
      y.v = conv(pl + "attention.v_proj");
      y.o = conv(pl + "attention.out_proj");
      y.gate_w = ptr(pl + "attention.gru_rel_pos_linear.weight", {8, DH});
      y.gate_b = ptr(pl + "attention.gru_rel_pos_linear.bias", {8});
      y.gate_c = ptr(pl + "attention.gru_rel_pos_const", {1, p.heads, 1, 1});
      y.ln1_w = ptr(pl + "layer_norm.weight", {H});
      y.ln1_b = ptr(pl + "layer_norm.bias", {H});
      y.f1 = conv(pl + "feed_forward.intermediate_dense");
      y.f2 = conv(pl + "feed_forward.output_dense");
      y.ln2_w = ptr(pl + "final_layer_norm.weight", {H});
      y.ln2_b = ptr(pl + "final_layer_norm.bias", {H});
      if (ok && (y.q.Cin != H || y.q.Cout != H || y.k.Cout != H || y.v.Cout != H || y.o.Cout != H || y.f1.Cin != H || y.f2.Cout != H ||
                 y.f2.Cin != y.f1.Cout))
        return rm_fail(pl + "attention.q_proj.weight");
      p.layers.push_back(y);
    }
    if (ok && p.layers.empty()) {
      m->missing = "encoder.layers.0.attention.q_proj.weight";
      ok = false;
    }
  }

  void build() {
    m->gb_floats_per_batch = 0;
    if (m->kind == "speech_predictor") {
      text_encoder("text_encoder.");
      m->seg_job_split = m->jobs.size();  // pack jobs of the module whose backward runs last (gradient segment 1)
      decoder("decoder.");
      vocoder("generator.");
    } else if (m->kind == "vocoder") {
      vocoder("");
    } else if (m->kind == "mel_style_encoder") {
      style_encoder();
    } else if (m->kind == "pitch_style_encoder") {
      m->pse_pre = conv("preconv", true);
      style_encoder();
    } else if (m->kind == "duration_predictor") {
      duration_predictor();
    } else if (m->kind == "pitch_energy_predictor") {
      pitch_energy_predictor();
    } else if (m->kind == "text_aligner" || m->kind == "text_aligner_train") {
      text_aligner();
    } else if (m->kind == "rmvpe") {
      rmvpe();
    } else if (m->kind == "wavlm") {
      wavlm();
    }
  }
};

int model_ready(const sty_model* m, const char* kind_a, const char* kind_b) {
  if (!m) {
    set_error("null model");
    return STY_EINVAL;
  }
  if (m->kind != kind_a && (!kind_b || m->kind != kind_b)) {
    set_error("model kind '%s' does not provide this entry point", m->kind.c_str());
    return STY_EINVAL;
  }
  if (!m->finalized) {
    set_error("model not finalized");
    return STY_ESTATE;
  }
  return STY_OK;
}
int entry_ready(const sty_model* m, const char* kind_a, const char* kind_b, bool bad_args, const char* msg) {
  const int rc = model_ready(m, kind_a, kind_b);
  if (rc) return rc;
  if (bad_args) {
    set_error("%s", msg);
    return STY_EINVAL;
  }
  return STY_OK;
}

}  // namespace sty

using namespace sty;

extern "C" {

int sty_model_create(const char* kind, sty_model** out) {
  if (!kind || !out) {
    set_error("sty_model_create: null argument");
    return STY_EINVAL;
  }
  std::string k(kind);
  if (k != "speech_predictor" && k != "vocoder" && k != "mel_style_encoder" && k != "duration_predictor" &&
      k != "pitch_energy_predictor" && k != "pitch_style_encoder" && k != "text_aligner" && k != "text_aligner_train" && k != "rmvpe" && k != "wavlm") {
    set_error("unknown model kind '%s'", kind);
    return STY_EINVAL;
  }
  *out = new sty_model();
  (*out)->kind = k;
  return STY_OK;
}

void sty_model_destroy(sty_model* m) {
  if (!m) return;
  if (m->arena) {
    convp16_forget_range(m->arena, m->arena + m->arena_bytes);
    (void)hipFree(m->arena);
  }
  if (m->prepared_ev) (void)hipEventDestroy(m->prepared_ev);
  if (m->fcs_dev) (void)hipFree(m->fcs_dev);
  if (m->stft_default) (void)hipFree(m->stft_default);
  if (m->garena) (void)hipFree(m->garena);
  if (m->fcs_bwd_dev) (void)hipFree(m->fcs_bwd_dev);
  if (m->wav_bucket_dev) (void)hipFree(m->wav_bucket_dev);
  m->wt.free();
  if (m->trainer) trainer_destroy(m->trainer);
  delete m;
}

int sty_model_bind(sty_model* m, const char* key, const float* ptr, int ndim, const int64_t* shape) {
  if (!m || !key || !ptr || ndim < 0 || (ndim > 0 && !shape)) {
    set_error("sty_model_bind: bad argument");
    return STY_EINVAL;
  }
  Param p;
  p.p = ptr;
  p.shape.assign(shape, shape + ndim);
  m->params[key] = p;
  m->finalized = false;
  return STY_OK;
}

int sty_model_finalize(sty_model* m) {
  if (!m) {
    set_error("null model");
    return STY_EINVAL;
  }
  m->train_prepared = false;
  if (m->arena) {
    convp16_forget_range(m->arena, m->arena + m->arena_bytes);
    (void)hipFree(m->arena);
    m->arena = nullptr;
  }
  if (!m->stft_default) {
    float host[4 * 33 * 64];
    build_stft64_bases(host);
    STY_HIP(hipMalloc((void**)&m->stft_default, sizeof(host)));
    STY_HIP(hipMemcpy(m->stft_default, host, sizeof(host), hipMemcpyHostToDevice));
  }
  m->requested.clear();
  m->jobs.clear();
  if (m->wav_bucket_dev) (void)hipFree(m->wav_bucket_dev);  // (it depends on num_buckets and max_bucket_distance)
  m->wav_bucket_dev = nullptr;
  m->wav_bucket_T = 0;
  m->wt.free();
  m->fcs.clear();
  m->missing.clear();
  m->ab = Bump();
  Builder dry{m, true};
  dry.build();
  if (!dry.ok) {
    set_error("state_dict key missing or wrong shape: %s", m->missing.c_str());
    return m->missing.find("shape") != std::string::npos ? STY_ESHAPE : STY_EINVAL;
  }
  m->arena_bytes = align_up(m->ab.off, 256) + 256;
  STY_HIP(hipMalloc((void**)&m->arena, m->arena_bytes));
  STY_HIP(hipMemset(m->arena, 0, m->arena_bytes));
  m->ab = Bump();
  m->ab.base = m->arena;
  m->ab.cap = m->arena_bytes;
  Builder real{m, false};
  real.build();
  if (!real.ok || m->ab.overflow) {
    set_error("internal: arena plan mismatch");
    return STY_EINVAL;
  }
  if (m->fcs_dev) {
    (void)hipFree(m->fcs_dev);
    m->fcs_dev = nullptr;
  }
  if (!m->fcs.empty()) {
    STY_HIP(hipMalloc((void**)&m->fcs_dev, m->fcs.size() * sizeof(StyleFcDesc)));
    STY_HIP(hipMemcpy(m->fcs_dev, m->fcs.data(), m->fcs.size() * sizeof(StyleFcDesc), hipMemcpyHostToDevice));
  }
  if (m->garena) {
    (void)hipFree(m->garena);
    m->garena = nullptr;
  }
  if (m->train_enabled) {
    STY_HIP(hipMalloc((void**)&m->garena, m->arena_bytes));
    STY_HIP(hipMemset(m->garena, 0, m->arena_bytes));
    m->pgrad.clear();
    for (auto& kv : m->pgrad_by_key) {
      auto it = m->params.find(kv.first);
      if (it == m->params.end()) {
        set_error("sty_model_bind_grad: '%s' is not a bound parameter", kv.first.c_str());
        return STY_EINVAL;
      }
      m->pgrad[it->second.p] = kv.second;
    }
  }
  m->finalized = true;
  m->prepared = false;
  m->split_packed = m->fp32_split != 0;
  return STY_OK;
}

// the text aligner is an inference-only kind (alignment decisions are arg-max decisions: fp32 operands, no training graph)
static int refuse_aligner(const sty_model* m, const char* what) {
  // (rmvpe: pitch values hang on an arg-max too; wavlm: a frozen network whose forward alone is built)
  if (m->kind != "text_aligner" && m->kind != "rmvpe" && m->kind != "wavlm") return STY_OK;
  set_error("%s: model kind '%s' is inference-only and runs fp32 operands%s", what, m->kind.c_str(),
            m->kind == "wavlm" ? " (its bf16 operand mode has a door of its own: sty_wavlm_set_compute)" : "");
  return STY_EINVAL;
}

int sty_model_enable_training(sty_model* m) {
  if (!m) {
    set_error("null model");
    return STY_EINVAL;
  }
  if (refuse_aligner(m, "sty_model_enable_training")) return STY_EINVAL;
  m->train_enabled = true;
  m->finalized = false;
  return STY_OK;
}

int sty_model_set_train_opts(sty_model* m, const sty_train_opts* o) {
  if (!m || !o || (o->f0_smooth && !(o->f0_smooth & 1)) || (o->energy_smooth && !(o->energy_smooth & 1)) ||
      o->f0_smooth < 0 || o->energy_smooth < 0 || o->f0_smooth > 63 || o->energy_smooth > 63) {
    set_error("sty_model_set_train_opts: null argument or smoothing width not an odd number in [0, 63]");
    return STY_EINVAL;
  }
  if (o->compute_bf16 && refuse_aligner(m, "sty_model_set_train_opts(compute_bf16)")) return STY_EINVAL;
  if (o->compute_bf16 && m->kind == "text_aligner_train") {  // its sibling's reason: alignment decisions are arg-max decisions
    set_error("sty_model_set_train_opts(compute_bf16): model kind 'text_aligner_train' runs fp32 operands");
    return STY_EINVAL;
  }
  if (o->compute_bf16 && m->fp32_split) {
    set_error("sty_model_set_train_opts(compute_bf16): the model runs the fp32 split mode (sty_model_set_fp32_split); switch it off first");
    return STY_EINVAL;
  }
  m->topts = *o;
  return STY_OK;
}

int sty_model_set_fp32_split(sty_model* m, int on) {
  if (!m) {
    set_error("sty_model_set_fp32_split: null model");
    return STY_EINVAL;
  }
  if (m->kind != "speech_predictor") {
    set_error("sty_model_set_fp32_split: model kind '%s' has no split mode (speech_predictor alone)", m->kind.c_str());
    return STY_EINVAL;
  }
  if (on && m->topts.compute_bf16) {
    set_error("sty_model_set_fp32_split: the model runs the bf16 compute mode (sty_model_set_train_opts); switch it off first");
    return STY_EINVAL;
  }
  m->fp32_split = on ? 1 : 0;
  if (on && !m->split_packed) m->finalized = false;  // the fragment triples are laid out and packed by the next finalize
  return STY_OK;
}

int sty_model_bind_grad(sty_model* m, const char* key, float* grad) {
  if (!m || !key || !grad) {
    set_error("sty_model_bind_grad: bad argument");
    return STY_EINVAL;
  }
  if (refuse_aligner(m, "sty_model_bind_grad")) return STY_EINVAL;
  m->pgrad_by_key[key] = grad;
  m->train_enabled = true;
  m->finalized = false;
  return STY_OK;
}

int sty_model_num_keys(const sty_model* m) { return m ? (int)m->requested.size() : 0; }
const char* sty_model_key(const sty_model* m, int i) {
  if (!m || i < 0 || i >= (int)m->requested.size()) return nullptr;
  return m->requested[i].c_str();
}

int sty_model_set_grad_hook(sty_model* m, sty_grad_hook hook, void* user) {
  if (!m) {
    set_error("sty_model_set_grad_hook: null model");
    return STY_EINVAL;
  }
  m->grad_hook = hook;
  m->grad_hook_user = user;
  return STY_OK;
}

int sty_model_invalidate(sty_model* m) {
  if (!m) {
    set_error("sty_model_invalidate: null model");
    return STY_EINVAL;
  }
  m->prepared = false;
  m->train_prepared = false;
  return STY_OK;
}

int sty_model_prepare(sty_model* m, void* stream) {
  if (!m || !m->finalized) {
    set_error("sty_model_prepare: model not finalized");
    return STY_ESTATE;
  }
  int rc = weights_prepare(m, S(stream));
  if (rc) return rc;
  m->prepared = true;
  return STY_OK;
}

}  // extern "C"
