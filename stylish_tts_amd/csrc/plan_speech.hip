// The speech side's inference plans: Run's blocks (ConvNeXt, resblock, conformer), the vocoder, the text encoder and
// the decoder, with the vocoder's and the speech predictor's inference entries and the two single-block entries.
#include "run.h"

namespace sty {

// ---------------------------------------------------------------------------------------------------
// forward plans: the blocks and plans of Run (run.h)
// ---------------------------------------------------------------------------------------------------
// GeneratorConvNeXtBlock: x [B][C][T] -> y.  The fused C == 32 kernel reads a 3-sample halo of x, so it must
// run out of place (y != x); the generic path is in place when y == x (its last conv is 1x1).
void Run::convnext(const ConvNeXt& c, const float* x, float* y, int T) {
  const int C = c.C;
  Scope sc(*this);
  if (C == 32) {
    if (live() && x == y) {
      set_error("internal: fused ConvNeXt32 needs distinct input and output buffers");
      rc = STY_EINVAL;
      return;
    }
    const int nt = convnext32_ntiles(T);
    double* part = ws.take<double>((size_t)B * 128 * nt * 2);
    float* scale = ws.take<float>((size_t)B * 128);
    if (live()) {
      Cnx32Args a;
      a.x = x;
      a.dw_w = c.dw_w;
      a.dw_b = c.dw_b;
      a.gb = gbp(c.norm);
      a.w1p = c.w1p;
      a.b1 = c.b1;
      a.alpha = c.alpha;
      a.w2a = c.w2a;
      a.b2eff = c.pw2.bias;
      a.scale = scale;
      a.part = part;
      a.y = y;
      a.T = T;
      a.ntiles = nt;
      a.bf16 = m->topts.compute_bf16;
      chk(launch_convnext32(a, B, 1, st));
      chk(launch_grn_finalize(part, nt, c.grn_gamma, B, 128, scale, st));
      chk(launch_convnext32(a, B, 2, st));
    }
    return;
  }
  float* u = ws.take<float>((size_t)B * C * T);
  float* h = ws.take<float>((size_t)B * 4 * C * T);
  const int nseg = row_stats_nseg(T);
  double* part = ws.take<double>((size_t)B * 4 * C * nseg * 2);
  float* scale = ws.take<float>((size_t)B * 4 * C);
  if (live()) {
    chk(launch_dwconv_adaln(x, c.dw_w, c.dw_b, B, C, T, 7, 1e-6f, gbp(c.norm), u, st));
    ConvArgs a = base(c.pw1, u, T, h);
    a.act = c.alpha ? ACT_SNAKE : ACT_GELU;  // Generator block: snake; AdaptiveConvNeXtBlock: exact GELU
    a.act_alpha = c.alpha;
    conv(a);
    chk(launch_row_stats(h, B * 4 * C, T, part, st));
    chk(launch_grn_finalize(part, nseg, c.grn_gamma, B, 4 * C, scale, st));
    ConvArgs b2 = base(c.pw2, h, T, y);
    b2.pro = PRO_SCALE;
    b2.pa = scale;
    b2.residual = x;
    conv(b2);
  }
}

// AdaptiveGeneratorBlock in place on x [B][32][T].  When the convs run on the persistent 32-channel kernel, each one
// leaves the (sum, sum of squares) partials of its OUTPUT behind (ConvArgs::stat_part), so only the first AdaIN of
// the block needs a statistics pass of its own.
void Run::resblock(const ResBlock32& r, float* x, int T) {
  Scope sc_(*this);
  float* xt = ws.take<float>((size_t)B * 32 * T);
  const int nseg_row = row_stats_nseg(T), nseg_p = conv32p_stat_nseg(T);
  const int nseg_max = nseg_row > nseg_p ? nseg_row : nseg_p;
  double* part_x = ws.take<double>((size_t)B * 32 * nseg_max * 2);
  double* part_t = ws.take<double>((size_t)B * 32 * nseg_max * 2);
  float* a = ws.take<float>(B * 32);
  float* s = ws.take<float>(B * 32);
  const int dil[3] = {1, 3, 5};
  bool have_x = false;  // part_x holds the statistics of x (left by the previous iteration's second conv)
  for (int i = 0; i < 3 && live(); ++i) {
    if (have_x)
      chk(launch_adain_finalize(part_x, nseg_p, gbp(r.n1[i]), B, 32, T, 1e-5f, a, s, st));
    else
      adain(x, 32, T, r.n1[i], a, s, part_x);
    ConvArgs c1 = base(r.c1[i], x, T, xt);
    c1.dil = dil[i];
    c1.pad = 5 * dil[i];
    c1.pro = PRO_AFFINE_SNAKE;
    c1.pa = a;
    c1.ps = s;
    c1.palpha = r.a1[i];
    const bool f1 = plan_route(m, c1).stats();
    if (f1) c1.stat_part = part_t;
    conv(c1);
    if (f1)
      chk(launch_adain_finalize(part_t, nseg_p, gbp(r.n2[i]), B, 32, T, 1e-5f, a, s, st));
    else
      adain(xt, 32, T, r.n2[i], a, s, part_t);
    ConvArgs c2 = base(r.c2[i], xt, T, x);
    c2.pro = PRO_AFFINE_SNAKE;
    c2.pa = a;
    c2.ps = s;
    c2.palpha = r.a2[i];
    c2.residual = x;
    have_x = plan_route(m, c2).stats() && i + 1 < 3;
    if (have_x) c2.stat_part = part_x;
    conv(c2);
  }
}

// ConformerBlock on x [B][C][T] -> out (conformer.py:242-250)
void Run::conformer(const Conformer& c, const float* x, float* out, int C, int T) {
  Scope sc_(*this);
  const size_t n = (size_t)B * C * T;
  float* z = ws.take<float>(n);
  float* big = ws.take<float>(4 * n);
  float* xff1 = ws.take<float>(n);
  float* q = ws.take<float>(2 * n);
  float* kv = ws.take<float>(4 * n);
  float* o = ws.take<float>(2 * n);
  float* x2 = ws.take<float>(n);
  float* g = ws.take<float>(2 * n);
  float* d = ws.take<float>(2 * n);
  float* x3 = ws.take<float>(n);
  float* x4 = ws.take<float>(n);
  if (live()) {
    auto ff = [&](const AdaFc& nrm, const PackedConv& w0, const PackedConv& w3, const float* in, float* res) {
      layernorm_ada(in, z, C, T, nrm);
      ConvArgs a = base(w0, z, T, big);
      a.act = ACT_SWISH;
      conv(a);
      ConvArgs b2 = base(w3, big, T, res);
      b2.out_scale = 0.5f;
      b2.residual = in;
      conv(b2);
    };
    ff(c.ff1n, c.ff1a, c.ff1b, x, xff1);
    layernorm_ada(x, z, C, T, c.attn_n);
    conv(base(c.to_q, z, T, q));
    conv(base(c.to_kv, z, T, kv));
    AttnArgs at;
    const int inner = c.to_q.Cout;  // 512 = 8 x 64
    at.q = q;
    at.k = kv;
    at.v = kv + (size_t)inner * T;
    at.o = o;
    at.qbs = (size_t)inner * T;
    at.kbs = at.vbs = (size_t)2 * inner * T;
    at.obs = (size_t)inner * T;
    at.T = T;
    at.H = 8;
    at.scale = 1.0f / sqrtf((float)(inner / 8));
    at.lengths = nullptr;
    at.bf16 = m->topts.compute_bf16;  // (round 6) bf16 mode: the conformer's attention on the bf16 matrix cores in the inference
                                      // plan as well (attn16.hip, as the training graph since round 4; c5-bf16: 242 us per forward
                                      // on the fp32 kernel)
    chk(launch_attention(at, B, inner / 8, st));
    ConvArgs ao = base(c.to_out, o, T, x2);
    ao.residual = xff1;
    conv(ao);
    layernorm_ada(x2, z, C, T, c.conv_n);
    ConvArgs p1 = base(c.pw1, z, T, g);
    p1.act = ACT_GLU;
    conv(p1);
    chk(launch_dwconv_bn_swish(g, c.dw_w, c.dw_b, c.bn_w, c.bn_b, c.bn_rm, c.bn_rv, 1e-5f, B, 2 * C, T, 31, d, st));
    ConvArgs p2 = base(c.pw2, d, T, x3);
    p2.residual = x2;
    conv(p2);
    ff(c.ff2n, c.ff2a, c.ff2b, x3, x4);
    layernorm_ada(x4, out, C, T, c.post_n);
  }
}

// MultiGenerator.forward
void Run::vocoder(const sty_vocoder_io& io) {
  const VocoderPlan& v = m->voc;
  const int T = io.T, Tu = 75 * T, N = 300 * T, C = v.hidden;
  // ---- harmonic source branch (no grad in the reference) ----
  float* prior = ws.take<float>((size_t)B * N);
  float* srcws = ws.take<float>(source_workspace_floats(B, T));
  float* lap = ws.take<float>((size_t)B * 32 * Tu);
  float* pp = ws.take<float>((size_t)B * 32 * Tu);
  float* hs = ws.take<float>((size_t)B * 32 * Tu);
  float* hp = ws.take<float>((size_t)B * 32 * Tu);
  const float* prior_used = prior;
  if (live()) {
    if (io.prior_override)
      prior_used = io.prior_override;
    else
      chk(launch_source(B, T, io.pitch, io.voiced, io.noise, io.seed, v.lin_w, v.lin_b, prior, srcws, st));
    chk(launch_stft64(B, N, prior_used, v.stft_fr, v.stft_fi, hs, hp, st));
    conv(base(v.amp_prior_conv, hs, Tu, lap));
    conv(base(v.phase_prior_conv, hp, Tu, pp));
  }
  resblock(v.amp_prior_block, lap, Tu);
  resblock(v.phase_prior_block, pp, Tu);
  if (live()) {
    tap(io.tap_prior, prior_used, (size_t)B * N);
    tap(io.tap_har_spec, hs, (size_t)B * 32 * Tu);
    tap(io.tap_har_phase, hp, (size_t)B * 32 * Tu);
    tap(io.tap_logamp_prior, lap, (size_t)B * 32 * Tu);
    tap(io.tap_phase_prior, pp, (size_t)B * 32 * Tu);
  }
  // hs / hp are dead from here on: reuse them
  // ---- stage A @T ----
  const size_t mark = ws.off;
  float* x0 = ws.take<float>((size_t)B * C * T);
  float* x1 = ws.take<float>((size_t)B * C * T);
  float* xc = ws.take<float>((size_t)B * C * T);
  if (live()) {
    conv(base(v.amp_input_conv, io.mel, T, x0));
    chk(launch_chan_layernorm(x0, x1, B, C, T, 1e-6f, 0, v.amp_norm_w, v.amp_norm_b, nullptr, 0, nullptr, st));
  }
  conformer(v.conf, x1, xc, C, T);
  if (live()) tap(io.tap_conformer_out, xc, (size_t)B * C * T);
  // ---- stage B: ConvNeXt trunk with pixel-shuffle upsampling ----
  for (const ConvNeXt& c : v.amp_convnext) convnext(c, xc, xc, T);
  float* cur = xc;
  int Tc = T, Cc = C;
  const int rates[3] = {3, 5, 5};
  float* trunk = nullptr;
  for (int i = 0; i < 3; ++i) {
    const int s = rates[i];
    float* nx = (i == 2) ? hs : ws.take<float>((size_t)B * (Cc / 2) * Tc * s);
    if (live()) {
      ConvArgs a = base(v.upconv[i], cur, Tc, nx);
      a.shuffle = s;
      conv(a);
    }
    Tc *= s;
    Cc /= 2;
    if (i == 2) {  // C == 32: fused block, out of place hs -> hp (har_phase is dead by now)
      convnext(v.upblock[i], nx, hp, Tc);
      nx = hp;
    } else {
      convnext(v.upblock[i], nx, nx, Tc);
    }
    cur = nx;
  }
  trunk = cur;  // [B][32][Tu] (lives in hp)
  if (live()) tap(io.tap_trunk, trunk, (size_t)B * 32 * Tu);
  note_peak();
  ws.off = mark;
  // ---- heads @75T ----
  float* logamp = ws.take<float>((size_t)B * 32 * Tu);
  float* ph = hs;
  float* ph_alt = ws.take<float>((size_t)B * 32 * Tu);
  float* real = ws.take<float>((size_t)B * 32 * Tu);
  float* imag = ws.take<float>((size_t)B * 32 * Tu);
  // The final LayerNorms in front of the k = 21 head convs: fused into the tiled kernel's prologue (rounds 1-4) where the
  // persistent 32-channel kernel does not take the conv; where it does (round 5), a LayerNorm pass + the persistent kernel are
  // faster than the fused tiled launch (c5-bf16: 121 us against ~35 + 40; the real / imag pair shares one pass)
  ConvArgs head_probe = base(v.amp_output_conv, trunk, Tu, logamp);
  const bool head32p = plan_route(m, head_probe).kernel == CONV_32P;
  float* lnbuf = head32p ? ws.take<float>((size_t)B * 32 * Tu) : nullptr;
  if (live()) {
    ConvArgs a = base(v.amp_output_conv, trunk, Tu, logamp);
    if (head32p) {
      chk(launch_chan_layernorm(trunk, lnbuf, B, 32, Tu, 1e-6f, 0, v.amp_fln_w, v.amp_fln_b, nullptr, 0, nullptr, st));
      a.x[0] = lnbuf;
    } else {
      a.pro = PRO_LN_AFFINE;
      a.palpha = v.amp_fln_w;
      a.pbeta = v.amp_fln_b;
      a.ln_eps = 1e-6f;
    }
    conv(a);
    tap(io.tap_logamp, logamp, (size_t)B * 32 * Tu);
    ConvArgs p = base(v.phase_input_conv, trunk, Tu, ph);
    p.nsrc = 3;
    p.x[1] = lap;
    p.x[2] = pp;
    p.xc[0] = p.xc[1] = p.xc[2] = 32;
    p.ln_out = 1;
    p.ln_w = v.phase_norm_w;
    p.ln_b = v.phase_norm_b;
    p.ln_eps = 1e-6f;
    conv(p);
  }
  for (const ConvNeXt& c : v.phase_convnext) {  // ping-pong: the fused block is out of place
    convnext(c, ph, ph_alt, Tu);
    float* t = ph;
    ph = ph_alt;
    ph_alt = t;
  }
  if (live()) {
    ConvArgs r = base(v.real_conv, ph, Tu, real);
    if (head32p) {
      chk(launch_chan_layernorm(ph, lnbuf, B, 32, Tu, 1e-6f, 0, v.phase_fln_w, v.phase_fln_b, nullptr, 0, nullptr, st));
      r.x[0] = lnbuf;
    } else {
      r.pro = PRO_LN_AFFINE;
      r.palpha = v.phase_fln_w;
      r.pbeta = v.phase_fln_b;
      r.ln_eps = 1e-6f;
    }
    conv(r);
    r.w = v.imag_conv;
    r.y = imag;
    conv(r);
    chk(launch_istft64(B, Tu, logamp, real, imag, v.stft_br, v.stft_bi, io.audio, st));
  }
  note_peak();
}

// TextEncoder.forward -> mu [B][inter][L]
void Run::text_encoder(const int64_t* tokens, const int64_t* lengths, int L, float* mu) {
  const TextEncPlan& t = m->te;
  const int H = t.H;
  Scope sc_(*this);
  const size_t n = (size_t)B * H * L;
  float* mask = ws.take<float>((size_t)B * L);
  float* x = ws.take<float>(n);
  float* h1 = ws.take<float>(n);
  float* h2 = ws.take<float>(n);
  float* q = ws.take<float>(n);
  float* k = ws.take<float>(n);
  float* vv = ws.take<float>(n);
  float* o = ws.take<float>(n);
  float* f = ws.take<float>((size_t)B * (t.layers.empty() ? H : t.layers[0].f1.Cout) * L);
  if (live()) {
    chk(launch_length_mask(lengths, B, L, mask, st));
    chk(launch_embedding(tokens, t.emb, B, L, H, t.tokens, sqrtf((float)H), x, st));
    const float* hin = x;
    for (int i = 0; i < 3; ++i) {
      ConvArgs a = base(t.pre[i], hin, L, h1);
      a.pro = PRO_MASK;
      a.mask = mask;
      conv(a);
      chk(launch_chan_layernorm(h1, h2, B, H, L, 1e-4f, 0, t.pre_g[i], t.pre_b[i], nullptr, 1, nullptr, st));
      hin = h2;
    }
    // hin holds relu(LN(...)) of layer 3; x = (x + proj(hin)) * mask
    ConvArgs pj = base(t.proj, hin, L, x);
    pj.residual = x;
    pj.out_mask = mask;
    pj.out_mask_post = 1;
    conv(pj);
    for (const TextEncLayer& l : t.layers) {
      ConvArgs aq = base(l.q, x, L, q);
      aq.pro = PRO_MASK;
      aq.mask = mask;
      conv(aq);
      aq.w = l.k;
      aq.y = k;
      conv(aq);
      aq.w = l.v;
      aq.y = vv;
      conv(aq);
      chk(launch_rope(q, k, B, 8, H / 8, L, 8, t.theta, st));
      AttnArgs at;
      at.q = q;
      at.k = k;
      at.v = vv;
      at.o = o;
      at.qbs = at.kbs = at.vbs = at.obs = (size_t)H * L;
      at.T = L;
      at.H = 8;
      at.scale = 1.0f / sqrtf((float)(H / 8));
      at.lengths = lengths;
      chk(launch_attention(at, B, H / 8, st));
      // x is masked already (prenet output / previous LN2 output are written masked)
      ConvArgs ao = base(l.o, o, L, h1);
      ao.residual = x;
      conv(ao);
      chk(launch_chan_layernorm(h1, x, B, H, L, 1e-4f, 0, l.n1g, l.n1b, nullptr, 0, nullptr, st));
      ConvArgs f1 = base(l.f1, x, L, f);
      f1.pro = PRO_MASK;
      f1.mask = mask;
      f1.act = ACT_RELU;
      conv(f1);
      ConvArgs f2 = base(l.f2, f, L, h1);
      f2.pro = PRO_MASK;
      f2.mask = mask;
      f2.out_mask = mask;
      f2.residual = x;
      conv(f2);
      chk(launch_chan_layernorm(h1, x, B, H, L, 1e-4f, 0, l.n2g, l.n2b, nullptr, 0, mask, st));
    }
    ConvArgs pm = base(t.proj_m, x, L, mu);
    pm.out_mask = mask;
    pm.out_mask_post = 1;
    conv(pm);
  }
}

// AdaptiveDecoderBlock (ada_norm.py:180-192): xcat [B][Cin][T] -> out [B][Cout][T]
void Run::dec_block(const DecBlock& d, const float* xcat, float* out, int T) {
  Scope sc_(*this);
  float* h = ws.take<float>((size_t)B * d.Cout * T);
  float* sc = ws.take<float>((size_t)B * d.Cout * T);
  const int cmax = d.Cin > d.Cout ? d.Cin : d.Cout;
  double* part = ws.take<double>((size_t)B * cmax * row_stats_nseg(T) * 2);
  float* a = ws.take<float>((size_t)B * cmax);
  float* s = ws.take<float>((size_t)B * cmax);
  if (live()) {
    const float r2 = 0.70710678118654752f;
    const float* res = xcat;
    if (d.has_sc) {
      ConvArgs c = base(d.sc, xcat, T, sc);
      c.out_scale = r2;
      conv(c);
      res = sc;
    } else {  // identity shortcut (Cin == Cout): (h + x) / sqrt(2)
      chk(launch_scale_copy(xcat, r2, (size_t)B * d.Cout * T, sc, st));
      res = sc;
    }
    adain(xcat, d.Cin, T, d.n1, a, s, part);
    ConvArgs c1 = base(d.c1, xcat, T, h);
    c1.pro = PRO_AFFINE_LRELU;
    c1.pa = a;
    c1.ps = s;
    conv(c1);
    adain(h, d.Cout, T, d.n2, a, s, part);
    ConvArgs c2 = base(d.c2, h, T, out);
    c2.pro = PRO_AFFINE_LRELU;
    c2.pa = a;
    c2.ps = s;
    c2.out_scale = r2;
    c2.residual = res;
    conv(c2);
    if (!d.has_sc && d.Cin != d.Cout) {
      set_error("decoder block: identity shortcut needs Cin == Cout");
      rc = STY_EINVAL;
    }
  }
}

// Decoder.forward eval mode (decoder.py:77-90): asr [B][128][T] -> mel [B][128][T]
void Run::decoder(const float* asr, const float* pitch, const float* energy, const float* voiced, int T, float* out) {
  const DecoderPlan& d = m->dec;
  Scope sc_(*this);
  const int din = d.asr_res.Cin, dr = d.asr_res.Cout, dh = d.encode.Cout;
  float* fnv = ws.take<float>((size_t)B * 3 * T);
  float* cat = ws.take<float>((size_t)B * (dh + dr + 3) * T);
  float* x = ws.take<float>((size_t)B * dh * T);
  float* res = ws.take<float>((size_t)B * dr * T);
  if (live()) {
    chk(launch_fnv(pitch, energy, voiced, d.fnv_w, B, T, fnv, st));
    const float* s1[2] = {asr, fnv};
    const int c1[2] = {din, 3};
    chk(launch_concat(s1, c1, 2, B, T, cat, st));
  }
  dec_block(d.encode, cat, x, T);
  if (live()) conv(base(d.asr_res, asr, T, res));
  for (int i = 0; i < 4; ++i) {
    if (live()) {
      const float* s2[3] = {x, res, fnv};
      const int c2[3] = {dh, dr, 3};
      chk(launch_concat(s2, c2, 3, B, T, cat, st));
    }
    dec_block(d.decode[i], cat, i == 3 ? out : x, T);
  }
}

int run_style_fc(Run& r, const float* style) {
  sty_model* m = r.m;
  r.gb = r.ws.take<float>(m->gb_floats_per_batch * r.B);
  if (r.live() && !m->fcs.empty())
    r.chk(launch_style_fc(m->fcs_dev, (int)m->fcs.size(), r.B, m->style_dim, style, r.gb, r.st));
  return r.rc;
}

int find_block(sty_model* m, const char* kind, const char* prefix, int C, int* k, const void** blk, const char* no_resblock) {
  const std::string p(prefix);
  if (std::string(kind) == "convnext") {
    auto it = m->params.find(p + ".dwconv.weight");
    if (it == m->params.end()) {
      set_error("no such block: %s", prefix);
      return STY_EINVAL;
    }
    auto match = [&](const ConvNeXt& c) { return c.dw_w == it->second.p; };
    const ConvNeXt* b = nullptr;
    for (const ConvNeXt& c : m->voc.amp_convnext)
      if (match(c)) b = &c;
    for (const ConvNeXt& c : m->voc.phase_convnext)
      if (match(c)) b = &c;
    for (int i = 0; i < 3; ++i)
      if (match(m->voc.upblock[i])) b = &m->voc.upblock[i];
    if (!b || b->C != C) {
      set_error("block %s not found or channel mismatch", prefix);
      return STY_EINVAL;
    }
    *k = 0;
    *blk = b;
    return STY_OK;
  }
  if (std::string(kind) == "resblock") {
    const ResBlock32* b = nullptr;
    if (p.size() >= 15 && p.compare(p.size() - 15, 15, "amp_prior_block") == 0) b = &m->voc.amp_prior_block;
    if (p.size() >= 17 && p.compare(p.size() - 17, 17, "phase_prior_block") == 0) b = &m->voc.phase_prior_block;
    if (!b || C != 32) {
      set_error(no_resblock, prefix);
      return STY_EINVAL;
    }
    *k = 1;
    *blk = b;
    return STY_OK;
  }
  set_error("sty_block: kind must be \"convnext\" or \"resblock\", not %s", kind);
  return STY_EINVAL;
}

}  // namespace sty

using namespace sty;

extern "C" {

static int vocoder_run(sty_model* m, const sty_vocoder_io* io, void* ws, size_t ws_bytes, void* stream, size_t* need) {
  Run r(m, io->B, ws, ws_bytes, stream);
  run_style_fc(r, io->style);
  r.vocoder(*io);
  return r.finish(need, ws, ws_bytes);
}

int sty_vocoder_workspace_bytes(const sty_model* m, int B, int T, size_t* bytes) {
  const int rc = entry_ready(m, "speech_predictor", "vocoder", !bytes || B <= 0 || T <= 1, "sty_vocoder_workspace_bytes: bad argument");
  if (rc) return rc;
  const sty_vocoder_io io = vocoder_io_dims(B, T);
  return vocoder_run(const_cast<sty_model*>(m), &io, nullptr, 0, nullptr, bytes);
}

int sty_vocoder_fwd(sty_model* m, const sty_vocoder_io* io, void* workspace, size_t ws_bytes, void* stream) {
  const bool bad = !io || !workspace || !io->mel || !io->style || !io->audio || io->B <= 0 || io->T <= 1 ||
                   (!io->prior_override && (!io->pitch || !io->voiced));
  int rc = entry_ready(m, "speech_predictor", "vocoder", bad, "sty_vocoder_fwd: bad argument");
  if (rc || (rc = ensure_prepared(m, stream))) return rc;
  return vocoder_run(m, io, workspace, ws_bytes, stream, nullptr);
}

static int speech_run(sty_model* m, const sty_speech_io* io, void* ws, size_t ws_bytes, void* stream, size_t* need) {
  Run r(m, io->B, ws, ws_bytes, stream);
  run_style_fc(r, io->style);
  const int B = io->B, L = io->L, T = io->T;
  const int inter = m->te.proj_m.Cout ? m->te.proj_m.Cout : 128;
  float* enc = r.ws.take<float>((size_t)B * inter * L);
  float* asr = r.ws.take<float>((size_t)B * inter * T);
  float* mel = r.ws.take<float>((size_t)B * m->dec.encode.Cout * T);
  r.text_encoder(io->texts, io->text_lengths, L, enc);
  if (r.live()) {
    r.tap(io->tap_text_encoding, enc, (size_t)B * inter * L);
    r.chk(launch_bmm_ct(enc, io->alignment, B, inter, L, T, asr, r.st));
  }
  r.decoder(asr, io->pitch, io->energy, io->voiced, T, mel);
  if (r.live()) r.tap(io->tap_decoder_out, mel, (size_t)B * m->dec.encode.Cout * T);
  sty_vocoder_io v = vocoder_io_of(*io);
  v.mel = mel;
  r.vocoder(v);
  return r.finish(need, ws, ws_bytes);
}

int sty_speech_workspace_bytes(const sty_model* m, int B, int L, int T, size_t* bytes) {
  const int rc = entry_ready(m, "speech_predictor", nullptr, !bytes || B <= 0 || L <= 0 || T <= 1, "sty_speech_workspace_bytes: bad argument");
  if (rc) return rc;
  const sty_speech_io io = speech_io_dims(B, L, T);
  return speech_run(const_cast<sty_model*>(m), &io, nullptr, 0, nullptr, bytes);
}

int sty_speech_fwd(sty_model* m, const sty_speech_io* io, void* workspace, size_t ws_bytes, void* stream) {
  const bool bad = !io || !workspace || !io->texts || !io->text_lengths || !io->alignment || !io->pitch || !io->energy ||
                   !io->voiced || !io->style || !io->denormal_pitch || !io->audio || io->B <= 0 || io->L <= 0 || io->T <= 1;
  int rc = entry_ready(m, "speech_predictor", nullptr, bad, "sty_speech_fwd: bad argument");
  if (rc || (rc = ensure_prepared(m, stream))) return rc;
  return speech_run(m, io, workspace, ws_bytes, stream, nullptr);
}

// ---- fine-grained entry points ----
int sty_convnext_fwd(sty_model* m, const char* prefix, int B, int C, int T, const float* x, const float* style,
                     float* y, void* workspace, size_t ws_bytes, void* stream) {
  int rc = entry_ready(m, "speech_predictor", "vocoder", !prefix || !x || !style || !y || !workspace, "sty_convnext_fwd: bad argument");
  if (rc) return rc;
  if ((rc = ensure_prepared(m, stream))) return rc;
  int k = 0;
  const void* blk = nullptr;
  if ((rc = find_block(m, "convnext", prefix, C, &k, &blk))) return rc;
  Run r(m, B, workspace, ws_bytes, stream);
  run_style_fc(r, style);
  if (x == y && C == 32) {
    set_error("sty_convnext_fwd: C == 32 runs out of place, y must differ from x");
    return STY_EINVAL;
  }
  r.convnext(*static_cast<const ConvNeXt*>(blk), x, y, T);
  return r.finish(nullptr, workspace, ws_bytes);
}

int sty_resblock_fwd(sty_model* m, const char* prefix, int B, int T, const float* x, const float* style, float* y,
                     void* workspace, size_t ws_bytes, void* stream) {
  int rc = entry_ready(m, "speech_predictor", "vocoder", !prefix || !x || !style || !y || !workspace, "sty_resblock_fwd: bad argument");
  if (rc) return rc;
  if ((rc = ensure_prepared(m, stream))) return rc;
  int k = 0;
  const void* blk = nullptr;
  if ((rc = find_block(m, "resblock", prefix, 32, &k, &blk, "no such resblock: %s"))) return rc;
  Run r(m, B, workspace, ws_bytes, stream);
  run_style_fc(r, style);
  if (y != x) STY_HIP(hipMemcpyAsync(y, x, (size_t)B * 32 * T * sizeof(float), hipMemcpyDeviceToDevice, r.st));
  r.resblock(*static_cast<const ResBlock32*>(blk), y, T);
  return r.finish(nullptr, workspace, ws_bytes);
}

}  // extern "C"
