"""state_dict manifests (key -> shape) of the hot-path modules, built from config dims only.

The drop-in contract of this package is the reference's state_dict key layout (what `build_model`
registers, train/models/models.py:29-85): the nn.Module shells in modules.py create
exactly these parameters/buffers, and libstylish_hip.so binds them by these names.  tests/ checks the
manifests key-for-key against fixtures dumped from the reference's own state_dict.
"""
from collections import OrderedDict

DEFAULT_CFG = dict(
    sample_rate=24000, n_mels=80, n_fft=512, win_length=512, hop_length=300,
    style_dim=64, inter_dim=128,
    dec_hidden=128, dec_residual=64,
    gen_input_dim=128, io_kernel=21, conformer_layers=1, conv_layers=8,
    tokens=178, te_hidden=128, te_filter=512, te_heads=8, te_layers=8, te_kernel=3,
    se_n_mels=80, se_max_channels=384, se_skip_downsample=True,
)


def _wn(m, name, shape):
    """weight_norm (new parametrization API): original0 = g, original1 = v."""
    m[name + ".parametrizations.weight.original0"] = [shape[0]] + [1] * (len(shape) - 1)
    m[name + ".parametrizations.weight.original1"] = list(shape)


def _adain(m, name, style_dim, ch):
    m[name + ".fc.weight"] = [2 * ch, style_dim]
    m[name + ".fc.bias"] = [2 * ch]


def _decoder_block(m, p, cin, cout, sd):  # ada_norm.py:143-178
    m[p + ".conv1.bias"] = [cout]
    _wn(m, p + ".conv1", [cout, cin, 3])
    m[p + ".conv2.bias"] = [cout]
    _wn(m, p + ".conv2", [cout, cout, 3])
    _adain(m, p + ".norm1", sd, cin)
    _adain(m, p + ".norm2", sd, cout)
    if cin != cout:
        _wn(m, p + ".conv1x1", [cout, cin, 1])


def _convnext(m, p, c, sd):  # conv_next.py:57-76
    m[p + ".snake"] = [1, 1, 4 * c]
    m[p + ".dwconv.weight"] = [c, 1, 7]
    m[p + ".dwconv.bias"] = [c]
    _adain(m, p + ".norm", sd, c)
    m[p + ".pwconv1.weight"] = [4 * c, c]
    m[p + ".pwconv1.bias"] = [4 * c]
    m[p + ".grn.gamma"] = [1, 1, 4 * c]
    m[p + ".grn.beta"] = [1, 1, 4 * c]
    m[p + ".pwconv2.weight"] = [c, 4 * c]
    m[p + ".pwconv2.bias"] = [c]


def _gen_block(m, p, c, sd):  # ada_norm.py:11-107
    for grp in ("convs1", "convs2"):
        for i in range(3):
            m[f"{p}.{grp}.{i}.bias"] = [c]
            _wn(m, f"{p}.{grp}.{i}", [c, c, 11])
    for grp in ("adain1", "adain2"):
        for i in range(3):
            _adain(m, f"{p}.{grp}.{i}", sd, c)
    for grp in ("alpha1", "alpha2"):
        for i in range(3):
            m[f"{p}.{grp}.{i}"] = [1, c, 1]


def _conv(m, p, cout, cin, k, bias=True):
    m[p + ".weight"] = [cout, cin, k]
    if bias:
        m[p + ".bias"] = [cout]


def multi_generator_manifest(cfg=None):
    """MultiGenerator on its own (generator.py:802-855): the `generator.*` keys of the SpeechPredictor without the
    prefix -- what `MultiGenerator(...).state_dict()` holds in the reference."""
    full = speech_predictor_manifest(cfg)
    return OrderedDict((k[len("generator."):], v) for k, v in full.items() if k.startswith("generator."))


def speech_predictor_manifest(cfg=None):
    c = dict(DEFAULT_CFG, **(cfg or {}))
    sd = c["style_dim"]
    m = OrderedDict()
    H, F, L = c["te_hidden"], c["te_filter"], c["te_layers"]
    # text_encoder (text_encoder.py:397-432)
    m["text_encoder.emb.weight"] = [c["tokens"], H]
    for i in range(3):
        _conv(m, f"text_encoder.prenet.conv_layers.{i}", H, H, 5)
    for i in range(3):
        m[f"text_encoder.prenet.norm_layers.{i}.gamma"] = [H]
        m[f"text_encoder.prenet.norm_layers.{i}.beta"] = [H]
    _conv(m, "text_encoder.prenet.proj", H, H, 1)
    for i in range(L):
        for n in ("conv_q", "conv_k", "conv_v", "conv_o"):
            _conv(m, f"text_encoder.encoder.attn_layers.{i}.{n}", H, H, 1)
    for i in range(L):
        m[f"text_encoder.encoder.norm_layers_1.{i}.gamma"] = [H]
        m[f"text_encoder.encoder.norm_layers_1.{i}.beta"] = [H]
    for i in range(L):
        _conv(m, f"text_encoder.encoder.ffn_layers.{i}.conv_1", F, H, c["te_kernel"])
        _conv(m, f"text_encoder.encoder.ffn_layers.{i}.conv_2", H, F, c["te_kernel"])
    for i in range(L):
        m[f"text_encoder.encoder.norm_layers_2.{i}.gamma"] = [H]
        m[f"text_encoder.encoder.norm_layers_2.{i}.beta"] = [H]
    _conv(m, "text_encoder.proj_m", c["inter_dim"], H, 1)
    # decoder (decoder.py:7-50)
    din, dh, dr = c["inter_dim"], c["dec_hidden"], c["dec_residual"]
    _decoder_block(m, "decoder.encode", din + 3, dh, sd)
    for i in range(4):
        _decoder_block(m, f"decoder.decode.{i}", dh + 3 + dr, dh, sd)
    for n in ("F0_conv", "N_conv", "voiced_conv"):
        m[f"decoder.{n}.bias"] = [1]
        _wn(m, f"decoder.{n}", [1, 1, 3])
    m["decoder.asr_res.0.bias"] = [dr]
    _wn(m, "decoder.asr_res.0", [dr, din, 1])
    # generator = MultiGenerator (generator.py:802-855)
    hd = c["n_fft"] // 2  # 256
    g = "generator."
    _conv(m, g + "amp_input_conv", hd, c["gen_input_dim"], c["io_kernel"])
    m[g + "amp_norm.weight"] = [hd]
    m[g + "amp_norm.bias"] = [hd]
    for li in range(c["conformer_layers"]):
        p = f"{g}amp_conformer.layers.{li}."
        # registration order in ConformerBlock.__init__ (conformer.py:199-240)
        for ff in ("ff1",):
            pass
        def _ff(name):
            _adain(m, p + name + ".fn.norm", sd, hd)
            m[p + name + ".fn.fn.net.0.weight"] = [4 * hd, hd]
            m[p + name + ".fn.fn.net.0.bias"] = [4 * hd]
            m[p + name + ".fn.fn.net.3.weight"] = [hd, 4 * hd]
            m[p + name + ".fn.fn.net.3.bias"] = [hd]
        _ff("ff1")
        _adain(m, p + "attn.norm", sd, hd)
        m[p + "attn.fn.to_q.weight"] = [512, hd]
        m[p + "attn.fn.to_kv.weight"] = [1024, hd]
        m[p + "attn.fn.to_out.weight"] = [hd, 512]
        m[p + "attn.fn.to_out.bias"] = [hd]
        _adain(m, p + "conv.norm", sd, hd)
        _conv(m, p + "conv.net.1", 4 * hd, hd, 1)
        m[p + "conv.net.3.conv.weight"] = [2 * hd, 1, 31]
        m[p + "conv.net.3.conv.bias"] = [2 * hd]
        for n, shp in (("weight", [2 * hd]), ("bias", [2 * hd]), ("running_mean", [2 * hd]),
                       ("running_var", [2 * hd]), ("num_batches_tracked", [])):
            m[p + "conv.net.4." + n] = shp
        _conv(m, p + "conv.net.6", hd, 2 * hd, 1)
        _ff("ff2")
        _adain(m, p + "post_norm", sd, hd)
    b = g + "basegen."
    hid = c["n_fft"] // 2 // 8  # 32
    for i in range(c["conv_layers"] - 3):
        _convnext(m, f"{b}amp_convnext.{i}", hd, sd)
    after = hd
    rates = [3, 5, 5]
    for i, s in enumerate(rates):
        before, after = after, after // 2
        _conv(m, f"{b}upconvs.{i}", after * s, before, 11)
    after = hd
    for i, s in enumerate(rates):
        after = after // 2
        _convnext(m, f"{b}upblocks.{i}", after, sd)
    m[b + "m_source.l_linear.weight"] = [1, 9]
    m[b + "m_source.l_linear.bias"] = [1]
    _conv(m, b + "amp_prior_conv", hid, hid, c["io_kernel"])
    _conv(m, b + "phase_prior_conv", hid, hid, c["io_kernel"])
    _gen_block(m, b + "amp_prior_block", hid, sd)
    _gen_block(m, b + "phase_prior_block", hid, sd)
    _conv(m, b + "phase_input_conv", hid, 3 * hid, c["io_kernel"])
    _conv(m, b + "amp_output_conv", hid, hid, c["io_kernel"])
    _conv(m, b + "phase_output_real_conv", hid, hid, c["io_kernel"])
    _conv(m, b + "phase_output_imag_conv", hid, hid, c["io_kernel"])
    m[b + "phase_norm.weight"] = [hid]
    m[b + "phase_norm.bias"] = [hid]
    for i in range(c["conv_layers"]):
        _convnext(m, f"{b}phase_convnext.{i}", hid, sd)
    for n in ("amp_final_layer_norm", "phase_final_layer_norm"):
        m[b + n + ".weight"] = [hid]
        m[b + n + ".bias"] = [hid]
    nf = c["n_fft"] // 8  # 64
    m[b + "stft.window"] = [nf]
    for n in ("weight_forward_real", "weight_forward_imag", "weight_backward_real", "weight_backward_imag"):
        m[b + "stft." + n] = [nf // 2 + 1, 1, nf]
    return m


def _sn(m, p, shape, bias=True):
    """old-style spectral_norm hook: bias, weight_orig, weight_u, weight_v."""
    if bias:
        m[p + ".bias"] = [shape[0]]
    m[p + ".weight_orig"] = list(shape)
    m[p + ".weight_u"] = [shape[0]]
    n = 1
    for s in shape[1:]:
        n *= s
    m[p + ".weight_v"] = [n]


def style_encoder_manifest(cfg=None):
    """MelStyleEncoder (mel_style_encoder.py:121-145), default dims 80 -> 384, style 64."""
    c = dict(DEFAULT_CFG, **(cfg or {}))
    m = OrderedDict()
    dim_in = c["se_n_mels"]
    _sn(m, "shared.0", [dim_in, 1, 3, 3])
    for i in range(4):
        dim_out = min(dim_in * 2, c["se_max_channels"])
        p = f"shared.{i + 1}"
        down = not (i == 3 and c["se_skip_downsample"])
        if down:
            _sn(m, p + ".downsample_res.conv", [dim_in, 1, 3, 3])
        _sn(m, p + ".conv1", [dim_in, dim_in, 3, 3])
        _sn(m, p + ".conv2", [dim_out, dim_in, 3, 3])
        if dim_in != dim_out:
            _sn(m, p + ".conv1x1", [dim_out, dim_in, 1, 1], bias=False)
        dim_in = dim_out
    _sn(m, "shared.6", [dim_in, dim_in, 5, 5])
    m["unshared.weight"] = [c["style_dim"], dim_in]
    m["unshared.bias"] = [c["style_dim"]]
    return m


def _text_encoder(m, pre, c, inter):
    """TextEncoder keys under `pre` (text_encoder.py:397-432) with projection width `inter`."""
    H, Fd, L = c["te_hidden"], c["te_filter"], c["te_layers"]
    m[pre + "emb.weight"] = [c["tokens"], H]
    for i in range(3):
        _conv(m, f"{pre}prenet.conv_layers.{i}", H, H, 5)
    for i in range(3):
        m[f"{pre}prenet.norm_layers.{i}.gamma"] = [H]
        m[f"{pre}prenet.norm_layers.{i}.beta"] = [H]
    _conv(m, pre + "prenet.proj", H, H, 1)
    for i in range(L):
        for n in ("conv_q", "conv_k", "conv_v", "conv_o"):
            _conv(m, f"{pre}encoder.attn_layers.{i}.{n}", H, H, 1)
    for i in range(L):
        m[f"{pre}encoder.norm_layers_1.{i}.gamma"] = [H]
        m[f"{pre}encoder.norm_layers_1.{i}.beta"] = [H]
    for i in range(L):
        _conv(m, f"{pre}encoder.ffn_layers.{i}.conv_1", Fd, H, c["te_kernel"])
        _conv(m, f"{pre}encoder.ffn_layers.{i}.conv_2", H, Fd, c["te_kernel"])
    for i in range(L):
        m[f"{pre}encoder.norm_layers_2.{i}.gamma"] = [H]
        m[f"{pre}encoder.norm_layers_2.{i}.beta"] = [H]
    _conv(m, pre + "proj_m", inter, H, 1)


N3_CFG = dict(dp_layers=3, dp_classes=16, pe_inter=256, pe_layers=3, pe_heads=2)


def duration_predictor_manifest(cfg=None):
    """DurationPredictor (duration_predictor.py:16-58), registration order of the reference."""
    c = {**DEFAULT_CFG, **N3_CFG, **(cfg or {})}
    sd, d = c["style_dim"], c["inter_dim"]
    m = OrderedDict()
    _text_encoder(m, "text_encoder.", c, d)
    for i in range(c["dp_layers"]):
        p = f"conv_next.{i}"
        m[p + ".dwconv.weight"] = [d, 1, 7]
        m[p + ".dwconv.bias"] = [d]
        _adain(m, p + ".norm", sd, d)
        m[p + ".pwconv1.weight"] = [4 * d, d]
        m[p + ".pwconv1.bias"] = [4 * d]
        m[p + ".grn.gamma"] = [1, 1, 4 * d]
        m[p + ".grn.beta"] = [1, 1, 4 * d]
        m[p + ".pwconv2.weight"] = [d, 4 * d]
        m[p + ".pwconv2.bias"] = [d]
    m["duration_proj.linear_layer.weight"] = [c["dp_classes"], d]
    m["duration_proj.linear_layer.bias"] = [c["dp_classes"]]
    _adain(m, "query_norm", sd, d)
    _adain(m, "key_norm", sd, d)
    for n in ("conv_q", "conv_k", "conv_v", "conv_o"):
        _conv(m, f"cross_attention.{n}", d, d, 1)
    m["cross_post.0.bias"] = [d]
    _wn(m, "cross_post.0", [d, 1, 5])
    m["cross_post.2.bias"] = [d]
    _wn(m, "cross_post.2", [d, d, 1])
    return m


def pitch_energy_predictor_manifest(cfg=None):
    """PitchEnergyPredictor (pitch_energy_predictor.py:8-60)."""
    c = {**DEFAULT_CFG, **N3_CFG, **(cfg or {})}
    sd, d = c["style_dim"], c["pe_inter"]
    hc = d + sd
    m = OrderedDict()
    _text_encoder(m, "text_encoder.", c, d)
    p = "prosody_encoder."
    for i in range(c["pe_layers"]):
        for n in ("conv_q", "conv_k", "conv_v", "conv_o"):
            _conv(m, f"{p}attn_layers.{i}.{n}", hc, hc, 1)
    for i in range(c["pe_layers"]):
        _adain(m, f"{p}norm_layers_1.{i}", sd, hc)
    for i in range(c["pe_layers"]):
        _conv(m, f"{p}ffn_layers.{i}.conv_1", 2 * hc, hc, 1)
        _conv(m, f"{p}ffn_layers.{i}.conv_2", hc, 2 * hc, 1)
    for i in range(c["pe_layers"]):
        _adain(m, f"{p}norm_layers_2.{i}", sd, hc)
    for i in range(c["pe_layers"]):
        _conv(m, f"{p}proj_layers.{i}", d, hc, 1)
    dims = [(hc, d), (d, d // 2), (d // 2, d // 2), (d // 2, d // 2)]
    for name in ("F0", "N"):
        for i, (ci, co) in enumerate(dims):
            _decoder_block(m, f"{name}.{i}", ci, co, sd)
    _conv(m, "F0_proj", 1, d // 2, 1)
    _conv(m, "N_proj", 1, d // 2, 1)
    return m


def pitch_style_encoder_manifest(cfg=None):
    """PitchStyleEncoder (mel_style_encoder.py:155-186): weight-normed 1x1 preconv over (mel, pitch, energy), then the
    MelStyleEncoder stack."""
    c = {**DEFAULT_CFG, **(cfg or {})}
    m = OrderedDict()
    d = c["se_n_mels"]
    m["preconv.bias"] = [d]
    _wn(m, "preconv", [d, d + 2, 1])
    m.update(style_encoder_manifest(c))
    return m


def text_aligner_manifest(n_mels=80, tokens=178, hidden_dim=640):
    """tdnn_blstm_ctc_model_base (text_aligner.py:33-45): three TDNN layers Conv1d(k = 5, 3, 3) -> ReLU ->
    BatchNorm1d(affine=False) (buffers only), an Ffn of five Linear + ReLU (Sequential indices 0, 3, 6, 9, 12: ReLU and
    Dropout sit in between), the output Linear over tokens + 1 classes (the blank is the last one)."""
    m = OrderedDict()
    cin = n_mels
    for i, k in enumerate((5, 3, 3)):
        _conv(m, f"encoder.layers.{i}.0", hidden_dim, cin, k)
        m[f"encoder.layers.{i}.2.running_mean"] = [hidden_dim]
        m[f"encoder.layers.{i}.2.running_var"] = [hidden_dim]
        m[f"encoder.layers.{i}.2.num_batches_tracked"] = []
        cin = hidden_dim
    for j in range(5):
        m[f"encoder.layers.3.ffn.{3 * j}.weight"] = [hidden_dim, hidden_dim]
        m[f"encoder.layers.3.ffn.{3 * j}.bias"] = [hidden_dim]
    m["encoder_output_layer.weight"] = [tokens + 1, hidden_dim]
    m["encoder_output_layer.bias"] = [tokens + 1]
    return m


def _bn2d(m, name, c):
    m[name + ".weight"] = [c]
    m[name + ".bias"] = [c]
    m[name + ".running_mean"] = [c]
    m[name + ".running_var"] = [c]
    m[name + ".num_batches_tracked"] = []


def _rmvpe_block(m, p, cin, cout):  # ConvBlockRes, train/dataprep/rmvpe/deepunet.py:6-41
    m[p + ".conv.0.weight"] = [cout, cin, 3, 3]
    _bn2d(m, p + ".conv.1", cout)
    m[p + ".conv.3.weight"] = [cout, cout, 3, 3]
    _bn2d(m, p + ".conv.4", cout)
    if cin != cout:
        m[p + ".shortcut.weight"] = [cout, cin, 1, 1]
        m[p + ".shortcut.bias"] = [cout]


def rmvpe_manifest(n_blocks=4, inter_layers=4, en_out_channels=16):
    """E2E0(n_blocks, 1, (2, 2), 5, inter_layers, 1, en_out_channels) (train/dataprep/rmvpe/model.py:49-86): DeepUnet0 of five
    encoder / decoder levels over 128 mel bins (deepunet.py:220-248), Conv2d(en_out_channels, 3, 3 x 3), one bidirectional GRU
    layer of 256 over 3 * 128 features (seq.py:4-16), Linear(512, 360).  The defaults are RMVPE's own `E2E0(4, 1, (2, 2))`
    (inference.py:16): 741 keys, 90,423,165 parameters (tests/golden/manifest_rmvpe.json is the reference's own list)."""
    m = OrderedDict()
    _bn2d(m, "unet.encoder.bn", 1)
    cin, c = 1, en_out_channels
    for l in range(5):
        for j in range(n_blocks):
            _rmvpe_block(m, f"unet.encoder.layers.{l}.conv.{j}", cin if j == 0 else c, c)
        cin, c = c, 2 * c
    for i in range(inter_layers):
        for j in range(n_blocks):
            _rmvpe_block(m, f"unet.intermediate.layers.{i}.conv.{j}", cin if i == 0 and j == 0 else c, c)
    for i in range(5):
        co = c // 2
        m[f"unet.decoder.layers.{i}.conv1.0.weight"] = [c, co, 3, 3]
        _bn2d(m, f"unet.decoder.layers.{i}.conv1.1", co)
        for j in range(n_blocks):
            _rmvpe_block(m, f"unet.decoder.layers.{i}.conv2.{j}", 2 * co if j == 0 else co, co)
        c = co
    m["cnn.weight"] = [3, en_out_channels, 3, 3]
    m["cnn.bias"] = [3]
    for sfx in ("_l0", "_l0_reverse"):
        m["fc.0.gru.weight_ih" + sfx] = [768, 384]
        m["fc.0.gru.weight_hh" + sfx] = [768, 256]
        m["fc.0.gru.bias_ih" + sfx] = [768]
        m["fc.0.gru.bias_hh" + sfx] = [768]
    m["fc.1.weight"] = [360, 512]
    m["fc.1.bias"] = [360]
    return m


WAVLM_DEFAULT_CFG = dict(
    hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
    conv_dim=(512, 512, 512, 512, 512, 512, 512), conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2),
    num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, num_buckets=320, max_bucket_distance=800,
    layer_norm_eps=1e-5, feat_extract_norm="group", feat_extract_activation="gelu", hidden_act="gelu",
    do_stable_layer_norm=False, conv_bias=False,
)


def wavlm_manifest(**cfg):
    """transformers' WavLMModel(WavLMConfig(**cfg)).state_dict() without masked_spec_embed (eval mode never reads it), for the
    configurations slm.check_wavlm_config accepts: group norm on the first feature conv, bias-free feature convs, post-LN layers.
    The defaults are the class's own (what microsoft/wavlm-base-plus is): 247 keys, 94,381,168 parameters with
    masked_spec_embed's 768 left out (tests/golden/manifest_wavlm.json is the class's own list)."""
    c = dict(WAVLM_DEFAULT_CFG)
    unknown = sorted(set(cfg) - set(c))
    if unknown:
        raise TypeError(f"wavlm_manifest: unknown config field(s) {unknown}")
    c.update(cfg)
    H, heads = c["hidden_size"], c["num_attention_heads"]
    m = OrderedDict()
    cin = 1
    for i, (dim, k) in enumerate(zip(c["conv_dim"], c["conv_kernel"])):
        m[f"feature_extractor.conv_layers.{i}.conv.weight"] = [dim, cin, k]
        if i == 0:
            m["feature_extractor.conv_layers.0.layer_norm.weight"] = [dim]
            m["feature_extractor.conv_layers.0.layer_norm.bias"] = [dim]
        cin = dim
    m["feature_projection.layer_norm.weight"] = [cin]
    m["feature_projection.layer_norm.bias"] = [cin]
    m["feature_projection.projection.weight"] = [H, cin]
    m["feature_projection.projection.bias"] = [H]
    K, G = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
    m["encoder.pos_conv_embed.conv.bias"] = [H]
    m["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = [1, 1, K]  # weight_norm(dim=2)
    m["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = [H, H // G, K]
    m["encoder.layer_norm.weight"] = [H]
    m["encoder.layer_norm.bias"] = [H]
    for l in range(c["num_hidden_layers"]):
        p = f"encoder.layers.{l}."
        for name in ("k_proj", "v_proj", "q_proj", "out_proj"):
            m[p + f"attention.{name}.weight"] = [H, H]
            m[p + f"attention.{name}.bias"] = [H]
        m[p + "attention.gru_rel_pos_const"] = [1, heads, 1, 1]
        m[p + "attention.gru_rel_pos_linear.weight"] = [8, H // heads]
        m[p + "attention.gru_rel_pos_linear.bias"] = [8]
        if l == 0:
            m[p + "attention.rel_attn_embed.weight"] = [c["num_buckets"], heads]
        m[p + "layer_norm.weight"] = [H]
        m[p + "layer_norm.bias"] = [H]
        m[p + "feed_forward.intermediate_dense.weight"] = [c["intermediate_size"], H]
        m[p + "feed_forward.intermediate_dense.bias"] = [c["intermediate_size"]]
        m[p + "feed_forward.output_dense.weight"] = [H, c["intermediate_size"]]
        m[p + "feed_forward.output_dense.bias"] = [H]
        m[p + "final_layer_norm.weight"] = [H]
        m[p + "final_layer_norm.bias"] = [H]
    return m
