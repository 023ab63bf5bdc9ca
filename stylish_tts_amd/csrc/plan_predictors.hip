// The inference plans beside the speech predictor: the style encoders, the duration and pitch-energy predictors, the text
// aligner and RMVPE, with their inference entries.
#include "run.h"

namespace sty {

// MelStyleEncoder.forward (mel_style_encoder.py:147-152): mel [B][1][n_mels][T] -> style [B][style_dim]
void style_run(Run& r, const float* mel, int T, float* style) {
  // padded-flat image layout (conv2d.hip): every activation is [B][C][H][W+1] with a zero last column
  const StylePlan& sp = r.m->sty_enc;
  const int B = r.B;
  auto conv2d = [&](const PackedConv& w, const float* x, int Cin2d, int n, int Wp, float* y, int hpad, int pad, int pro,
                    float out_scale, const float* residual, const float* mask) {
    if (!r.live()) return;
    ConvArgs a;
    a.x[0] = x;
    a.xc[0] = w.Cin;
    a.nsrc = 1;
    a.B = B;
    a.T = n;
    a.pad = pad;
    a.w = w;
    a.flatW = Wp;
    a.hpad = hpad;
    a.Cin2d = Cin2d;
    a.pro = pro;
    a.out_scale = out_scale;
    a.residual = residual;
    a.out_mask = mask;
    a.out_mask_post = 1;
    a.y = y;
    a.bf16 = r.m->topts.compute_bf16;  // the compute mode also applies to the inference plan (a frozen encoder of a stage)
    r.chk(launch_conv1d(a, r.st));
  };
  auto mask_for = [&](int Hh, int Ww, int Hv, int Wv) {
    float* mk = r.ws.take<float>((size_t)B * Hh * (Ww + 1));
    if (r.live()) r.chk(launch_flat_mask(B, Hh, Ww + 1, Hv, Wv, mk, r.st));
    return mk;
  };
  const float r2 = 0.70710678118654752f;
  int H = sp.n_mels, W = T, C = sp.n_mels;
  float* melp = r.ws.take<float>((size_t)B * H * (W + 1));
  if (r.live()) r.chk(launch_pad_cols(mel, (size_t)B * H, W, melp, r.st));
  const float* mk = mask_for(H, W, H, W);
  float* x = r.ws.take<float>((size_t)B * C * H * (W + 1));
  conv2d(sp.stem, melp, 1, H * (W + 1), W + 1, x, 1, 1, PRO_NONE, 1.f, nullptr, mk);
  for (int i = 0; i < 4; ++i) {
    const StyleResBlk& k = sp.blk[i];
    const int Ho = k.down ? H / 2 : H, Wo = k.down ? (W + 1) / 2 : W;
    const int n = H * (W + 1), no = Ho * (Wo + 1);
    const float* mko = k.down ? mask_for(Ho, Wo, Ho, Wo) : mk;
    float* sc_full = r.ws.take<float>((size_t)B * k.Cout * n);
    float* sc = r.ws.take<float>((size_t)B * k.Cout * no);
    float* h1 = r.ws.take<float>((size_t)B * k.Cin * n);
    float* h2 = r.ws.take<float>((size_t)B * k.Cin * no);
    float* y = r.ws.take<float>((size_t)B * k.Cout * no);
    // shortcut (scaled by 1/sqrt2 up front: pooling is linear).  Learned shortcut + down-sampling: the reference runs
    // conv1x1 then avg_pool2d (mel_style_encoder.py:93-99); both are linear and the 1x1 conv has no bias, so they commute --
    // pooling FIRST puts the conv (and in training its input gradient and weight gradient) on a quarter of the positions
    // and halves the pooled channels
    const float* res = nullptr;
    if (k.down && k.has_sc) {
      float* pooled = sc_full;  // [B][Cin][Ho][Wo + 1] fits in the full-resolution Cout buffer
      if (r.live()) r.chk(launch_avgpool2(x, B * k.Cin, H, W, 1.f, pooled, r.st));
      conv2d(k.sc, pooled, k.Cin, no, Wo + 1, sc, 0, 0, PRO_NONE, r2, nullptr, mko);
      res = sc;
    } else if (k.down) {
      if (r.live()) r.chk(launch_avgpool2(x, B * k.Cout, H, W, r2, sc, r.st));
      res = sc;
    } else if (k.has_sc) {
      conv2d(k.sc, x, k.Cin, n, W + 1, sc_full, 0, 0, PRO_NONE, r2, nullptr, mk);
      res = sc_full;
    }
    // residual branch
    conv2d(k.c1, x, k.Cin, n, W + 1, h1, 1, 1, PRO_LRELU, 1.f, nullptr, mk);
    const float* h = h1;
    if (k.down) {
      if (r.live()) r.chk(launch_dwconv2d_s2(h1, k.dw_w9, k.dw_b, B, k.Cin, H, W, h2, r.st));
      h = h2;
    }
    conv2d(k.c2, h, k.Cin, no, Wo + 1, y, 1, 1, PRO_LRELU, r2, res, mko);
    // identity shortcut (last block: 384 -> 384, no downsample): out = (x + conv2(h)) / sqrt2
    if (!res && r.live()) r.chk(launch_axpy(x, r2, y, (size_t)B * k.Cout * no, r.st));
    x = y;
    H = Ho;
    W = Wo;
    C = k.Cout;
    mk = mko;
  }
  // LeakyReLU -> 5x5 valid conv -> global mean -> LeakyReLU -> Linear
  const int KH = 5;
  const int Hh = H - KH + 1, Wh = W - sp.head.K + 1;
  const int n = H * (W + 1);
  if (r.live() && (Hh < 1 || Wh < 1)) {
    set_error("style encoder: input too short (need T >= 40 frames)");
    r.rc = STY_ESHAPE;
    return;
  }
  const float* mkh = mask_for(H, W, Hh > 0 ? Hh : 0, Wh > 0 ? Wh : 0);
  float* hd = r.ws.take<float>((size_t)B * C * n);
  conv2d(sp.head, x, C, n, W + 1, hd, 0, 0, PRO_LRELU, 1.f, nullptr, mkh);
  if (r.live()) r.chk(launch_pool_fc(hd, B, C, n, Hh * Wh, sp.fc_w, sp.fc_b, sp.style_dim, style, r.st));
  r.note_peak();
}

// DurationPredictor.forward (duration_predictor.py:58-87): -> out [B][L][classes]
void duration_forward(Run& r, const int64_t* texts, const int64_t* lengths, int L, float* out) {
  sty_model* m = r.m;
  const DurationPlan& d = m->dur;
  const int B = r.B, C = m->te.proj_m.Cout;
  const size_t n = (size_t)B * C * L;
  float* enc = r.ws.take<float>(n);
  float* mask = r.ws.take<float>((size_t)B * L);
  float* qn = r.ws.take<float>(n);
  float* kn = r.ws.take<float>(n);
  float* q = r.ws.take<float>(n);
  float* k = r.ws.take<float>(n);
  float* v = r.ws.take<float>(n);
  float* o = r.ws.take<float>(n);
  float* a1 = r.ws.take<float>(n);
  float* a2 = r.ws.take<float>(n);
  float* x = r.ws.take<float>(n);
  float* wdw = r.ws.take<float>((size_t)C * 5);
  float* dl = r.ws.take<float>((size_t)B * d.classes * L);
  r.text_encoder(texts, lengths, L, enc);
  if (r.live()) {
    r.chk(launch_length_mask(lengths, B, L, mask, r.st));
    // compute_cross: queries / keys are two AdaLN views of the text encoding (duration_predictor.py:61-72)
    r.layernorm_ada(enc, qn, C, L, d.qn);
    r.layernorm_ada(enc, kn, C, L, d.kn);
    r.conv(r.base(d.cq, qn, L, q));
    r.conv(r.base(d.ck, kn, L, k));
    r.conv(r.base(d.cv, kn, L, v));
    const int H = 8, DH = C / H;
    r.chk(launch_rope(q, k, B, H, DH, L, 8, m->te.theta, r.st));
    AttnArgs at;
    at.q = q;
    at.k = k;
    at.v = v;
    at.o = o;
    at.qbs = at.kbs = at.vbs = at.obs = (size_t)C * L;
    at.T = L;
    at.H = H;
    at.scale = 1.0f / sqrtf((float)DH);
    at.lengths = lengths;
    r.chk(launch_attention(at, B, DH, r.st));
    r.conv(r.base(d.co, o, L, a1));
    // cross_post: weight-normed depthwise k5 -> SiLU -> weight-normed 1x1; (. + encoding) / sqrt(2)
    r.chk(launch_wn_dw(d.dw_g, d.dw_v, C, 5, wdw, r.st));
    r.chk(launch_dwconv_fwd(a1, wdw, d.dw_b, B, C, L, 5, 2, a2, r.st));
    r.chk(launch_act_fwd(ACT_SWISH, a2, nullptr, B, C, L, a1, r.st));
    const float r2 = 0.70710678118654752f;
    r.chk(launch_scale_copy(enc, r2, n, a2, r.st));
    ConvArgs pc = r.base(d.post, a1, L, x);
    pc.out_scale = r2;
    pc.residual = a2;
    r.conv(pc);
  }
  for (const ConvNeXt& c : d.cnx) {
    r.convnext(c, x, x, L);
    if (r.live()) r.chk(launch_mask_mul(x, mask, B, C, L, r.st));
  }
  if (r.live()) {
    r.conv(r.base(d.proj, x, L, dl));
    r.chk(launch_dur_post(dl, mask, B, d.classes, L, out, r.st));
  }
}

// PitchEnergyPredictor.forward (pitch_energy_predictor.py:62-82): -> f0 [B][T], energy [B][T]
void pitch_energy_forward(Run& r, const int64_t* texts, const int64_t* lengths, const float* alignment,
                                 const float* style, int L, int T, float* f0, float* energy) {
  sty_model* m = r.m;
  const PitchEnergyPlan& p = m->pe;
  const int B = r.B, D = m->te.proj_m.Cout, S = m->style_dim, HC = D + S;
  const size_t nh = (size_t)B * HC * L;
  float* enc = r.ws.take<float>((size_t)B * D * L);
  float* mask = r.ws.take<float>((size_t)B * L);
  float* sx = r.ws.take<float>((size_t)B * S * L);
  float* x = r.ws.take<float>(nh);
  float* q = r.ws.take<float>(nh);
  float* k = r.ws.take<float>(nh);
  float* v = r.ws.take<float>(nh);
  float* o = r.ws.take<float>(nh);
  float* h1 = r.ws.take<float>(nh);
  float* x2 = r.ws.take<float>(nh);
  float* f = r.ws.take<float>(2 * nh);
  float* pj = r.ws.take<float>((size_t)B * D * L);
  float* xt = r.ws.take<float>((size_t)B * HC * T);
  r.text_encoder(texts, lengths, L, enc);
  if (r.live()) {
    r.chk(launch_length_mask(lengths, B, L, mask, r.st));
    r.chk(launch_style_expand(style, B, S, L, sx, r.st));
    const float* src[2] = {enc, sx};
    const int cs[2] = {D, S};
    r.chk(launch_concat(src, cs, 2, B, L, x, r.st));
    const int H = p.heads, DH = HC / H;
    for (const ProsodyLayer& l : p.layers) {  // prosody_encoder.py:69-79, dropout off
      r.chk(launch_mask_mul(x, mask, B, HC, L, r.st));
      r.conv(r.base(l.q, x, L, q));
      r.conv(r.base(l.k, x, L, k));
      r.conv(r.base(l.v, x, L, v));
      r.chk(launch_rope_n(q, k, B, H, DH, L, DH / 2, r.st));
      AttnArgs at;
      at.q = q;
      at.k = k;
      at.v = v;
      at.o = o;
      at.qbs = at.kbs = at.vbs = at.obs = (size_t)HC * L;
      at.T = L;
      at.H = H;
      at.scale = 1.0f / sqrtf((float)DH);
      at.lengths = lengths;
      r.chk(launch_attention(at, B, DH, r.st));
      ConvArgs ao = r.base(l.o, o, L, h1);
      ao.residual = x;
      r.conv(ao);
      r.layernorm_ada(h1, x2, HC, L, l.n1);
      ConvArgs f1 = r.base(l.f1, x2, L, f);
      f1.pro = PRO_MASK;
      f1.mask = mask;
      f1.act = ACT_RELU;
      r.conv(f1);
      ConvArgs f2 = r.base(l.f2, f, L, h1);
      f2.pro = PRO_MASK;
      f2.mask = mask;
      f2.out_mask = mask;
      f2.residual = x2;
      r.conv(f2);
      r.layernorm_ada(h1, x2, HC, L, l.n2);
      r.conv(r.base(l.proj, x2, L, pj));
      const float* s2[2] = {pj, sx};
      r.chk(launch_concat(s2, cs, 2, B, L, x, r.st));
    }
    r.chk(launch_mask_mul(x, mask, B, HC, L, r.st));
    r.chk(launch_bmm_ct(x, alignment, B, HC, L, T, xt, r.st));
  }
  // two stacks of AdaptiveDecoderBlocks on the expanded prosody, 1x1 heads
  for (int which = 0; which < 2; ++which) {
    const DecBlock* blk = which ? p.nn : p.f0;
    Run::Scope sc(r);
    const float* in = xt;
    float* bufs[2] = {r.ws.take<float>((size_t)B * D * T), r.ws.take<float>((size_t)B * D * T)};
    for (int i = 0; i < 4; ++i) {
      r.dec_block(blk[i], in, bufs[i & 1], T);
      in = bufs[i & 1];
    }
    if (r.live()) r.conv(r.base(which ? p.np : p.f0p, in, T, which ? energy : f0));
  }
}

// CTCModel.forward in eval mode (text_aligner.py:73-127, 209-274): mel [B][n_mels][T], lengths [B] -> log_probs [B][T][classes].
// Frames at or beyond a row's length are zeroed in front of each TDNN conv (the conv's mask prologue); what the convs
// compute on those frames is kept, as the reference keeps it.  fp32 operands throughout (compute_bf16 is refused for the kind).
void aligner_forward(Run& r, const float* mel, const int64_t* lengths, int T, float* out) {
  const AlignerPlan& p = r.m->ali;
  const int B = r.B, H = p.hidden, V = p.classes;
  const size_t n = (size_t)B * H * T;
  float* mask = r.ws.take<float>((size_t)B * T);
  float* a = r.ws.take<float>(n);
  float* b = r.ws.take<float>(n);
  float* c = r.ws.take<float>(n);
  float* logits = r.ws.take<float>((size_t)B * V * T);
  if (!r.live()) return;
  r.chk(launch_length_mask(lengths, B, T, mask, r.st));
  const float* x = mel;
  for (int i = 0; i < 3 && r.live(); ++i) {
    float* y = (i & 1) ? b : a;
    ConvArgs ca = r.base(p.tdnn[i], x, T, y);
    ca.pro = PRO_MASK;
    ca.mask = mask;
    ca.act = ACT_RELU;
    r.conv(ca);
    r.chk(launch_aligner_bn(y, B, H, T, p.bn_scale[i], p.bn_shift[i], r.st));
    x = y;
  }
  // Ffn: five Linear + ReLU, the skip around all five in the last one's output stage (x = a here)
  const float* src = a;
  for (int i = 0; i < 5 && r.live(); ++i) {
    float* y = (i & 1) ? c : b;
    ConvArgs ca = r.base(p.ffn[i], src, T, y);
    ca.act = ACT_RELU;
    if (i == 4) ca.residual = a;
    r.conv(ca);
    src = y;
  }
  if (r.live()) {
    r.conv(r.base(p.out, src, T, logits));
    r.chk(launch_log_softmax_rows(logits, B, V, T, out, r.st));
  }
}

// RMVPE.mel2hidden (train/dataprep/rmvpe/inference.py:29-36) over E2E0.forward (model.py:82-86): logmel [B][128][n] ->
// salience [B][n][360].  H is time (reflected to Tp, the next multiple of 32), W the 128 mel bins; every activation is
// padded-flat [B][C][H][W + 1] (conv2d.hip).  Level l has H = Tp >> l, W = 128 >> l, C0 << l channels.  cat[l] is the decoder's
// concat input [B][2 C_l][n_l]: the encoder writes its skip into the second half when it produces it (one launch per
// utterance: the conv's output has no batch stride), the transposed conv writes the first half.
void rmvpe_forward(Run& r, int n, const float* logmel, float* sal) {
  const RmvpePlan& p = r.m->rmv;
  const int B = r.B, L = RMVPE_LEVELS, Tp = 32 * ((n - 1) / 32 + 1);
  auto Hl = [&](int l) { return Tp >> l; };
  auto Wl = [&](int l) { return RMVPE_MELS >> l; };
  auto Nl = [&](int l) { return (size_t)Hl(l) * (Wl(l) + 1); };
  auto Cl = [&](int l) { return p.C0 << l; };
  const float* mk[L + 1];
  for (int l = 0; l <= L; ++l) {
    float* m = r.ws.take<float>((size_t)B * Nl(l));
    if (r.live()) r.chk(launch_flat_mask(B, Hl(l), Wl(l) + 1, Hl(l), Wl(l), m, r.st));
    mk[l] = m;
  }
  float* cat[L];
  for (int l = 0; l < L; ++l) cat[l] = r.ws.take<float>((size_t)B * 2 * Cl(l) * Nl(l));
  const size_t big = (size_t)B * (p.C0 > 3 ? p.C0 : 3) * Nl(0);  // (3: cnn's output) the largest activation: C_l n_l shrinks with l, the intermediate is 2 C_4 n_5
  float* x0 = r.ws.take<float>((size_t)B * Nl(0));
  float* pp[2] = {r.ws.take<float>(big), r.ws.take<float>(big)};
  float* hb = r.ws.take<float>(big);
  float* sb = r.ws.take<float>(big);
  const int nf = 3 * RMVPE_MELS;
  float* gin = r.ws.take<float>((size_t)B * nf * Tp);
  float* xg = r.ws.take<float>((size_t)B * 1536 * Tp);
  float* hcat = r.ws.take<float>((size_t)B * 512 * Tp);
  float* logits = r.ws.take<float>((size_t)B * RMVPE_CLASSES * Tp);
  r.note_peak();
  if (!r.live()) return;
  // one conv on level l; Bc = 1 with pre-offset pointers: the launch of one utterance
  auto conv2d = [&](const PackedConv& w, const float* x, int Cin2d, int l, int Bc, int act, const float* residual, float* y) {
    if (!r.live()) return;
    ConvArgs a;
    a.x[0] = x;
    a.xc[0] = w.Cin;
    a.B = Bc;
    a.T = (int)Nl(l);
    a.w = w;
    a.flatW = Wl(l) + 1;
    a.hpad = a.pad = (w.K - 1) / 2;
    a.Cin2d = Cin2d;
    a.act = act;
    a.residual = residual;
    a.out_mask = mk[l];
    a.out_mask_post = 1;
    a.y = y;
    r.chk(launch_conv1d(a, r.st));  // fp32 operands: compute_bf16 is refused for the kind
  };
  // ConvBlockRes: relu(bn(conv(relu(bn(conv x))))) + (x | conv1x1(x) + b).  skip != nullptr: the output goes to channels
  // [skip_c0, skip_c0 + Cout) of a buffer with skip_C channels
  auto block = [&](const RmvpeBlock& k, const float* x, int l, float* y, float* skip, int skip_C, int skip_c0) {
    const float* res = x;
    if (k.has_sc) {
      conv2d(k.sc, x, k.Cin, l, B, ACT_NONE, nullptr, sb);
      res = sb;
    }
    conv2d(k.c1, x, k.Cin, l, B, ACT_RELU, nullptr, hb);
    if (!skip) return conv2d(k.c2, hb, k.Cout, l, B, ACT_RELU, res, y);
    const size_t per = (size_t)k.Cout * Nl(l);
    for (int b = 0; b < B; ++b)
      conv2d(k.c2, hb + b * per, k.Cout, l, 1, ACT_RELU, res + b * per, skip + ((size_t)b * skip_C + skip_c0) * Nl(l));
  };
  r.chk(launch_rmvpe_input(logmel, p.in_ss, B, n, Tp, x0, r.st));
  const float* cur = x0;
  int flip = 0;
  for (int l = 0; l < L && r.live(); ++l) {  // Encoder (deepunet.py:127-133)
    const int C = Cl(l);
    for (int j = 0; j < p.n_blocks; ++j) {
      const bool last = j == p.n_blocks - 1;
      block(p.enc[l][j], cur, l, pp[flip], last ? cat[l] : nullptr, 2 * C, C);
      if (!last) cur = pp[flip], flip ^= 1;
    }
    for (int b = 0; b < B && r.live(); ++b)  // AvgPool2d(2) of the skip, read where it lies
      r.chk(launch_avgpool2(cat[l] + ((size_t)b * 2 * C + C) * Nl(l), C, Hl(l), Wl(l), 1.f, pp[flip] + (size_t)b * C * Nl(l + 1), r.st));
    cur = pp[flip], flip ^= 1;
  }
  for (size_t i = 0; i < p.inter.size() && r.live(); ++i) {  // Intermediate (deepunet.py:149-152)
    block(p.inter[i], cur, L, pp[flip], nullptr, 0, 0);
    cur = pp[flip], flip ^= 1;
  }
  for (int i = 0; i < L && r.live(); ++i) {  // Decoder (deepunet.py:90-95, 167-170)
    const int l = L - 1 - i, C = Cl(l);
    r.chk(launch_rmvpe_deconv(cur, p.up[i].wd, p.up[i].bias, B, p.up[i].Cin, C, Hl(l + 1), Wl(l + 1), (size_t)2 * C * Nl(l), cat[l], r.st));
    cur = cat[l];
    for (int j = 0; j < p.n_blocks; ++j) {
      block(p.dec[i][j], cur, l, pp[flip], nullptr, 0, 0);
      cur = pp[flip], flip ^= 1;
    }
  }
  conv2d(p.cnn, cur, p.C0, 0, B, ACT_NONE, nullptr, hb);  // [B][3][Tp][129]
  if (!r.live()) return;
  r.chk(launch_rmvpe_gru_in(hb, B, Tp, gin, r.st));
  r.conv(r.base(p.gru_ih, gin, Tp, xg));
  if (r.live()) r.chk(launch_rmvpe_gru(xg, p.whhT, p.bhh[0], p.bhh[1], B, Tp, hcat, r.st));
  r.conv(r.base(p.head, hcat, Tp, logits));
  if (r.live()) r.chk(launch_rmvpe_salience(logits, B, Tp, n, sal, r.st));
}

}  // namespace sty

using namespace sty;

extern "C" {

// ---- second-stage predictors (inference) ----
static int duration_run(sty_model* m, int B, int L, const int64_t* texts, const int64_t* lengths, const float* style,
                        float* out, void* ws, size_t ws_bytes, void* stream, size_t* need) {
  Run r(m, B, ws, ws_bytes, stream);
  run_style_fc(r, style);
  duration_forward(r, texts, lengths, L, out);
  return r.finish(need, ws, ws_bytes);
}
int sty_duration_workspace_bytes(const sty_model* m, int B, int L, size_t* bytes) {
  const int rc = entry_ready(m, "duration_predictor", nullptr, !bytes || B <= 0 || L <= 0, "sty_duration_workspace_bytes: bad argument");
  if (rc) return rc;
  return duration_run(const_cast<sty_model*>(m), B, L, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, bytes);
}
int sty_duration_fwd(sty_model* m, int B, int L, const int64_t* texts, const int64_t* text_lengths, const float* style,
                     float* dur_pred, void* workspace, size_t ws_bytes, void* stream) {
  int rc = entry_ready(m, "duration_predictor", nullptr, !texts || !text_lengths || !style || !dur_pred || !workspace || B <= 0 || L <= 0,
                       "sty_duration_fwd: bad argument");
  if (rc || (rc = ensure_prepared(m, stream))) return rc;
  return duration_run(m, B, L, texts, text_lengths, style, dur_pred, workspace, ws_bytes, stream, nullptr);
}
// ---- text aligner (inference) ----
static int aligner_run(sty_model* m, int B, int T, const float* mel, const int64_t* lengths, float* out, void* ws,
                       size_t ws_bytes, void* stream, size_t* need) {
  Run r(m, B, ws, ws_bytes, stream);
  aligner_forward(r, mel, lengths, T, out);
  return r.finish(need, ws, ws_bytes);
}
int sty_aligner_workspace_bytes(const sty_model* m, int B, int T, size_t* bytes) {
  const int rc = entry_ready(m, "text_aligner", "text_aligner_train", !bytes || B <= 0 || T <= 0, "sty_aligner_workspace_bytes: bad argument");
  if (rc) return rc;
  return aligner_run(const_cast<sty_model*>(m), B, T, nullptr, nullptr, nullptr, nullptr, 0, nullptr, bytes);
}
int sty_aligner_fwd(sty_model* m, int B, int T, const float* mel, const int64_t* mel_lengths, float* log_probs,
                    void* workspace, size_t ws_bytes, void* stream) {
  int rc = entry_ready(m, "text_aligner", "text_aligner_train", !mel || !mel_lengths || !log_probs || !workspace || B <= 0 || T <= 0,
                       "sty_aligner_fwd: bad argument");
  if (rc) return rc;
  if (m->topts.compute_bf16) {
    set_error("sty_aligner_fwd: compute_bf16 is refused for the text aligner");
    return STY_EINVAL;
  }
  if ((rc = ensure_prepared(m, stream))) return rc;
  return aligner_run(m, B, T, mel, mel_lengths, log_probs, workspace, ws_bytes, stream, nullptr);
}
// ---- RMVPE pitch extraction (train/dataprep/rmvpe/inference.py) ----
void sty_rmvpe_resample_kernel_host(float* out) { build_rmvpe_resample_kernel(out); }
void sty_rmvpe_mel_basis_host(float* out) { build_rmvpe_mel_basis(out); }
int sty_rmvpe_mel_workspace_bytes(int B, int N, size_t* bytes) {
  if (!bytes || B <= 0 || N <= 0 || rmvpe_resampled_len(N) <= 512) {
    set_error("sty_rmvpe_mel_workspace_bytes: bad argument (the reflect padding needs more than 512 samples at 16 kHz)");
    return STY_EINVAL;
  }
  *bytes = rmvpe_mel_workspace_floats(B, N) * sizeof(float);
  return STY_OK;
}
int sty_rmvpe_mel_fwd(int B, int N, const float* audio, float* logmel, void* workspace, size_t ws_bytes, void* stream) {
  if (!audio || !logmel || !workspace || B <= 0 || N <= 0 || rmvpe_resampled_len(N) <= 512) {
    set_error("sty_rmvpe_mel_fwd: bad argument (the reflect padding needs more than 512 samples at 16 kHz)");
    return STY_EINVAL;
  }
  if (ws_bytes < rmvpe_mel_workspace_floats(B, N) * sizeof(float)) {
    set_error("sty_rmvpe_mel_fwd: workspace too small");
    return STY_ENOMEM;
  }
  return launch_rmvpe_mel(B, N, audio, logmel, (float*)workspace, S(stream));
}
// the frame axis is reflected to the next multiple of 32: at most 15 frames when n >= 17 (and at most n - 1 above that)
static int rmvpe_shape_ok(const char* what, const sty_model* m, int B, int n) {
  if (!m || B <= 0) {
    set_error("%s: bad argument", what);
    return STY_EINVAL;
  }
  if (n < 17) {
    set_error("%s: %d frames cannot be reflected to a multiple of 32 (at least 17 are needed)", what, n);
    return STY_ESHAPE;
  }
  return STY_OK;
}
static int rmvpe_run(sty_model* m, int B, int n, const float* logmel, float* sal, void* ws, size_t ws_bytes, void* stream,
                     size_t* need) {
  Run r(m, B, ws, ws_bytes, stream);
  rmvpe_forward(r, n, logmel, sal);
  return r.finish(need, ws, ws_bytes);
}
int sty_rmvpe_workspace_bytes(const sty_model* m, int B, int n, size_t* bytes) {
  int rc = rmvpe_shape_ok("sty_rmvpe_workspace_bytes", m, B, n);
  if (rc || (rc = model_ready(m, "rmvpe"))) return rc;
  if (!bytes) {
    set_error("sty_rmvpe_workspace_bytes: bad argument");
    return STY_EINVAL;
  }
  return rmvpe_run(const_cast<sty_model*>(m), B, n, nullptr, nullptr, nullptr, 0, nullptr, bytes);
}
int sty_rmvpe_fwd(sty_model* m, int B, int n, const float* logmel, float* salience, void* workspace, size_t ws_bytes,
                  void* stream) {
  int rc = rmvpe_shape_ok("sty_rmvpe_fwd", m, B, n);
  if (rc || (rc = model_ready(m, "rmvpe"))) return rc;
  if (!logmel || !salience || !workspace) {
    set_error("sty_rmvpe_fwd: bad argument");
    return STY_EINVAL;
  }
  if ((rc = ensure_prepared(m, stream))) return rc;
  return rmvpe_run(m, B, n, logmel, salience, workspace, ws_bytes, stream, nullptr);
}
int sty_rmvpe_decode(int B, int n, const float* salience, float thred, float* f0, void* stream) {
  if (!salience || !f0 || B <= 0 || n <= 0) {
    set_error("sty_rmvpe_decode: bad argument");
    return STY_EINVAL;
  }
  return launch_rmvpe_decode(salience, B * n, thred, f0, S(stream));
}
static int pitch_energy_run(sty_model* m, int B, int L, int T, const int64_t* texts, const int64_t* lengths,
                            const float* alignment, const float* style, float* f0, float* energy, void* ws,
                            size_t ws_bytes, void* stream, size_t* need) {
  Run r(m, B, ws, ws_bytes, stream);
  run_style_fc(r, style);
  pitch_energy_forward(r, texts, lengths, alignment, style, L, T, f0, energy);
  return r.finish(need, ws, ws_bytes);
}
int sty_pitch_energy_workspace_bytes(const sty_model* m, int B, int L, int T, size_t* bytes) {
  const int rc = entry_ready(m, "pitch_energy_predictor", nullptr, !bytes || B <= 0 || L <= 0 || T <= 0,
                             "sty_pitch_energy_workspace_bytes: bad argument");
  if (rc) return rc;
  return pitch_energy_run(const_cast<sty_model*>(m), B, L, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, 0, nullptr, bytes);
}
int sty_pitch_energy_fwd(sty_model* m, int B, int L, int T, const int64_t* texts, const int64_t* text_lengths,
                         const float* alignment, const float* style, float* pitch, float* energy, void* workspace,
                         size_t ws_bytes, void* stream) {
  const bool bad = !texts || !text_lengths || !alignment || !style || !pitch || !energy || !workspace || B <= 0 || L <= 0 || T <= 0;
  int rc = entry_ready(m, "pitch_energy_predictor", nullptr, bad, "sty_pitch_energy_fwd: bad argument");
  if (rc || (rc = ensure_prepared(m, stream))) return rc;
  return pitch_energy_run(m, B, L, T, texts, text_lengths, alignment, style, pitch, energy, workspace, ws_bytes,
                          stream, nullptr);
}

static int style_entry(sty_model* m, int B, int T, const float* mel, float* style, void* ws, size_t ws_bytes,
                       void* stream, size_t* need) {
  Run r(m, B, ws, ws_bytes, stream);
  style_run(r, mel, T, style);
  return r.finish(need, ws, ws_bytes);
}
// PitchStyleEncoder.forward at coarse_multiplier 1 (mel_style_encoder.py:188-205)
static int pitch_style_entry(sty_model* m, int B, int T, const float* mel, const float* pitch, const float* energy,
                             float* style, void* ws, size_t ws_bytes, void* stream, size_t* need) {
  Run r(m, B, ws, ws_bytes, stream);
  const int C = m->pse_pre.Cin, D = m->pse_pre.Cout, Tp = T + 2;
  float* cat = r.ws.take<float>((size_t)B * C * T);
  float* padded = r.ws.take<float>((size_t)B * C * Tp);
  float* pre = r.ws.take<float>((size_t)B * D * Tp);
  if (r.live()) {
    const float* src[3] = {mel, pitch, energy};
    const int cs[3] = {C - 2, 1, 1};
    r.chk(launch_concat(src, cs, 3, B, T, cat, r.st));
    r.chk(launch_pad_time(cat, B * C, T, 1, padded, r.st));  // Conv1d(k = 1, padding = 1): two bias-only frames
    r.conv(r.base(m->pse_pre, padded, Tp, pre));
  }
  style_run(r, pre, Tp, style);
  return r.finish(need, ws, ws_bytes);
}
int sty_pitch_style_workspace_bytes(const sty_model* m, int B, int T, size_t* bytes) {
  const int rc = entry_ready(m, "pitch_style_encoder", nullptr, !bytes || B <= 0 || T < 40,
                             "sty_pitch_style_workspace_bytes: bad argument (T >= 40 frames)");
  if (rc) return rc;
  return pitch_style_entry(const_cast<sty_model*>(m), B, T, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                           bytes);
}
int sty_pitch_style_fwd(sty_model* m, int B, int T, const float* mel, const float* pitch, const float* energy,
                        float* style, void* workspace, size_t ws_bytes, void* stream) {
  int rc = entry_ready(m, "pitch_style_encoder", nullptr, !mel || !pitch || !energy || !style || !workspace || B <= 0 || T < 40,
                       "sty_pitch_style_fwd: bad argument (T >= 40 frames)");
  if (rc || (rc = ensure_prepared(m, stream))) return rc;
  return pitch_style_entry(m, B, T, mel, pitch, energy, style, workspace, ws_bytes, stream, nullptr);
}
int sty_style_workspace_bytes(const sty_model* m, int B, int T, size_t* bytes) {
  const int rc = entry_ready(m, "mel_style_encoder", nullptr, !bytes || B <= 0 || T < 40,
                             "sty_style_workspace_bytes: bad argument (T >= 40 frames)");
  if (rc) return rc;
  return style_entry(const_cast<sty_model*>(m), B, T, nullptr, nullptr, nullptr, 0, nullptr, bytes);
}
int sty_style_fwd(sty_model* m, int B, int T, const float* mel, float* style, void* workspace, size_t ws_bytes,
                  void* stream) {
  int rc = entry_ready(m, "mel_style_encoder", nullptr, !mel || !style || !workspace || B <= 0 || T < 40,
                       "sty_style_fwd: bad argument (T >= 40 frames)");
  if (rc || (rc = ensure_prepared(m, stream))) return rc;
  return style_entry(m, B, T, mel, style, workspace, ws_bytes, stream, nullptr);
}

}  // extern "C"
