"""The length-masked paths on ragged text batches, against the float64 oracle.

Every model that reads text takes `text_lengths`, and the mask reaches a large part of the kernel surface: the length mask
itself, the conv prologue and output masks, the masked channel LayerNorm, the -1e4 attention mask (forward and all backward
kernels), the masked weight- and bias-gradient kernels, the masked backward passes of the training tape, the duration
kernels and the zero-duration tail of the alignment kernel.  The batches here (tests/cases.py RAGGED_CASES) put a length on,
below and above every tile edge of those kernels at L <= 130 and hold rows of length 1; tests/test_ragged_oracle.py pins what
is assumed about the reference arithmetic on the same inputs (the fp32 oracle inside half of each gate; an off-by-one in one
row's length moving every gradient by 20 x the gate or more).

Runs on the GPU box only (`-m gpu`); self-contained: models from oracle.manifest + oracle.weights.fill_state_dict.
"""
import functools
import os

import pytest
import torch

from tests.cases import RAGGED_CASES, RAGGED_PAD_IDS, make_ragged
from tests.test_ragged_oracle import GATE_GRAD, GATE_OUT, N_GRADS, duration_cotangent, duration_params, oracle_duration, rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMB = "text_encoder.emb.weight"
# frames per case where a test needs durations (every row sums to T): c3's 208 at c3's L, about two frames a token elsewhere
FRAMES = {100: 208, 37: 80, 130: 272, 64: 136}
CASE_IDS = [f"L{L}-" + "_".join(map(str, ln)) for L, ln in RAGGED_CASES]


class Report:
    """the per-tensor table of tests/test_hip_parity.py"""

    def __init__(self):
        self.rows, self.bad = [], []

    def add(self, name, got, ref, tol):
        e = rel(got, ref)
        ok = e <= tol and bool(torch.isfinite(got).all())
        self.rows.append(f"  {name:48s} rel_err {e:9.3e}  tol {tol:.1e}  {'ok' if ok else 'FAIL'}")
        if not ok:
            self.bad.append(name)

    def done(self):
        print("\n" + "\n".join(self.rows))
        assert not self.bad, f"parity failures: {self.bad}"


def dev(t):
    return t.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(i):
    L, lengths = RAGGED_CASES[i]
    return make_ragged(L, lengths)


@functools.lru_cache(maxsize=None)
def _oracle64(i):
    cs = _case(i)
    return oracle_duration(duration_params(), cs["texts_a"], cs["text_lengths"], cs["style"], torch.float64)


def _hip_duration(texts, text_lengths, style, *, bf16=False):
    """a fresh DurationPredictor: forward (inference entry point), forward_train and backward under the shared cotangent
    -> (out_inference, out_train, d_style, {key: gradient}), all on the CPU"""
    import stylish_tts_amd as S
    dp = S.DurationPredictor()
    dp.load_state_dict(duration_params())
    dp = dp.to(DEV)
    with torch.no_grad():
        out_inf = dp(dev(texts), dev(text_lengths), dev(style)).cpu()
    dp.enable_training()
    if bf16:
        dp.set_train_opts(compute_bf16=True)
    out = dp.forward_train(dev(texts), dev(text_lengths), dev(style))
    d_style = dp.backward(dev(duration_cotangent(*out.shape)))
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in dp.named_parameters() if p.grad is not None}
    return out_inf, out.cpu(), d_style.cpu(), grads


@pytest.mark.parametrize("i", range(len(RAGGED_CASES)), ids=CASE_IDS)
def test_duration_predictor_training_graph_on_ragged_batches_vs_float64_oracle(i):
    """DurationPredictor forward_train + backward, dropout off, fp32, against autograd on the float64 oracle with EVERY
    parameter that has a gradient listed (195: the text encoder's prenet, eight attention / FFN layers with their masked
    LayerNorms, emb, proj_m; the cross attention, the ConvNeXt blocks, the head).  Gates: those the graph has on its one
    ragged input in test_hip_parity.py (out 5e-5; d_style and gradients 5e-4 of the tensor's maximum); the fp32 oracle sits
    inside half of them on these inputs (test_ragged_oracle.py; worst 2.5e-6 / 1.1e-4).  The inference entry point (the
    second implementation of the text encoder) is held to the same 5e-5 on `out`."""
    cs = _case(i)
    out64, ds64, g64 = _oracle64(i)
    out_inf, out, d_style, grads = _hip_duration(cs["texts_a"], cs["text_lengths"], cs["style"])
    assert len(g64) == N_GRADS
    assert set(g64) <= set(grads), sorted(set(g64) - set(grads))
    rep = Report()
    rep.add("out (inference)", out_inf, out64, GATE_OUT)
    rep.add("out (training graph)", out, out64, GATE_OUT)
    rep.add("d_style", d_style, ds64, GATE_GRAD)
    for k in g64:
        rep.add("d " + k[-46:], grads[k], g64[k], GATE_GRAD)
    print(f"\n  L={RAGGED_CASES[i][0]} lengths={RAGGED_CASES[i][1]}: {len(g64)} parameter gradients")
    rep.done()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(RAGGED_CASES)), ids=CASE_IDS)
def test_duration_predictor_padding_is_exact(i, compute):
    """No tolerance: the output at padded positions is exactly 0; ids on the padded positions (variant B: 170..177, which
    no valid position uses) change no bit of the output, through the inference entry point and through the training graph;
    after backward the embedding-gradient rows of ids that occur on padding only are exactly 0 (float atomics in the
    parameter sums do not disturb an exact zero).  Again in the bf16 compute mode: with lengths present the attention stays
    on the fp32 kernels there, so what it adds are the masked convs on bf16 operands, their twins and weight gradients."""
    cs = _case(i)
    tl, pad = cs["text_lengths"], ~cs["valid"]
    inf_a, out_a, _, g_a = _hip_duration(cs["texts_a"], tl, cs["style"], bf16=compute == "bf16")
    inf_b, out_b, _, g_b = _hip_duration(cs["texts_b"], tl, cs["style"], bf16=compute == "bf16")
    for name, t in (("inference A", inf_a), ("inference B", inf_b), ("training A", out_a), ("training B", out_b)):
        assert torch.isfinite(t).all(), name
        assert (t[pad] == 0).all(), f"{name}: padded output not exactly 0: max {t[pad].abs().max().item():.3e}"
    assert torch.equal(inf_a, inf_b), f"inference: padded ids leak, max {(inf_a - inf_b).abs().max().item():.3e}"
    assert torch.equal(out_a, out_b), f"training graph: padded ids leak, max {(out_a - out_b).abs().max().item():.3e}"
    lo, hi = RAGGED_PAD_IDS
    assert g_a[EMB].abs().max().item() > 0 and g_b[EMB].abs().max().item() > 0
    assert (g_b[EMB][lo:hi] == 0).all(), f"d emb rows {lo}..{hi - 1} (padding only): {g_b[EMB][lo:hi].abs().max().item():.3e}"
    assert (g_a[EMB][0] == 0).all(), f"d emb row 0 (padding only): {g_a[EMB][0].abs().max().item():.3e}"
    assert (g_a[EMB][lo:hi] == 0).all() and (g_b[EMB][0] == 0).all()  # ids that occur nowhere


def test_negative_control_one_length_off_by_one_is_red_on_every_gated_tensor():
    """NEGATIVE CONTROL, L = 100: the library gets row 1 with length 66 where the oracle keeps 65.  The gates of the test
    above must report this RED on `out` (valid positions), on d_style and on EVERY one of the 195 gradients (the float64
    oracle moves each by 1.2e-2 or more under this change, test_ragged_oracle.py; the gate is 5e-4)."""
    cs = _case(0)
    out64, ds64, g64 = _oracle64(0)
    tl = cs["text_lengths"].clone()
    assert tl[1].item() == 65
    tl[1] = 66
    _, out, d_style, grads = _hip_duration(cs["texts_a"], tl, cs["style"])
    valid = cs["valid"][:, :, None].float()
    rows, green = [], []
    for name, got, ref, tol in [("out (valid positions)", out * valid, out64, GATE_OUT), ("d_style", d_style, ds64, GATE_GRAD)] + \
            [("d " + k[-46:], grads[k], g64[k], GATE_GRAD) for k in g64]:
        e = rel(got, ref)
        rows.append(f"  {name:48s} rel_err {e:9.3e}  tol {tol:.1e}  {'red' if e > tol else 'GREEN'}")
        if not e > tol:
            green.append(name)
    print("\n  NEGATIVE CONTROL (row 1: length 66 against the oracle's 65)\n" + "\n".join(rows))
    assert not green, f"the gates do not see an off-by-one length on: {green}"


# ---- SpeechPredictor and PitchEnergyPredictor at c3's text length ----------------------------------------------------------
def _mel_l1(a, b):
    from oracle.frontend import calculate_mel
    return (calculate_mel(a.squeeze(1), 512, 512, 300) - calculate_mel(b.squeeze(1), 512, 512, 300)).abs().mean().item()


@functools.lru_cache(maxsize=None)
def _frames_case():
    L, lengths = RAGGED_CASES[0]
    cs = make_ragged(L, lengths, T=FRAMES[L])
    from oracle import frontend
    cs["alignment"] = frontend.duration_to_alignment(cs["durations"])
    cs["voiced"] = (cs["pitch"] > 20).float()
    assert cs["alignment"].shape == (len(lengths), L, FRAMES[L])
    return cs


SP_EXTRA = ["text_encoder.prenet.conv_layers.1.weight", "text_encoder.prenet.norm_layers.2.gamma",
            "text_encoder.encoder.ffn_layers.3.conv_2.weight", "text_encoder.encoder.norm_layers_2.7.beta",
            "text_encoder.encoder.attn_layers.0.conv_k.bias", "text_encoder.proj_m.weight",
            "decoder.encode.conv1x1.parametrizations.weight.original1", "decoder.decode.0.norm1.fc.weight",
            "decoder.N_conv.parametrizations.weight.original1", "decoder.N_conv.parametrizations.weight.original0",
            "decoder.F0_conv.bias", "decoder.asr_res.0.parametrizations.weight.original1"]


def _sp_keys():
    """the keys of test_speech_predictor_backward_vs_oracle_and_reference_golden: those of its fixture plus its extras"""
    from safetensors import safe_open
    with safe_open(os.path.join(os.path.dirname(__file__), "golden", "sp_small_grads.safetensors"), "pt") as f:
        gold = [k[len("grad."):] for k in f.keys() if k not in ("grad.style", "grad.energy")]
    assert EMB in gold
    return gold + SP_EXTRA


def test_speech_predictor_on_a_ragged_batch_at_c3_text_length():
    """SpeechPredictor at B = 8, L = 100, T = 208 with lengths 100, 65, 64, 63, 33, 17, 16, 1: the acoustic tape's masked
    text encoder, the soft alignment with zero-duration tails (padded tokens still carry softmax weight there) and the
    `enc @ alignment` contraction on a ragged batch.  forward and forward_train against the oracle (prior shared): taps
    1e-5, audio MSE <= 1e-8, mel-L1 <= 1e-3 (the gates of test_speech_predictor_end_to_end_vs_oracle_and_golden); the
    text_encoding tap exactly 0 on padded columns; audio bit-identical between token variants A and B; backward under the
    cotangent sign(oracle audio) / N against the oracle's autograd at the keys and 3e-2 gates of
    test_speech_predictor_backward_vs_oracle_and_reference_golden; embedding-gradient rows of padding-only ids exactly 0."""
    import stylish_tts_amd as S
    from oracle import speech_predictor as osp
    from oracle.manifest import speech_predictor_manifest
    from oracle.weights import fill_state_dict
    cs = _frames_case()
    B, L = cs["texts_a"].shape
    T = cs["pitch"].shape[1]
    tl, ali = cs["text_lengths"], cs["alignment"]
    P = fill_state_dict(speech_predictor_manifest(), 0)
    keys = _sp_keys()
    Q = {k: v.detach().clone() for k, v in P.items()}
    for k in keys:
        Q[k].requires_grad_(True)
    style_r, energy_r = cs["style"].clone().requires_grad_(True), cs["energy"].clone().requires_grad_(True)
    want = {}
    ref = osp.speech_predictor(Q, cs["texts_a"], tl, ali, cs["pitch"], energy_r, cs["voiced"], style_r, cs["pitch"],
                               cs["noise"], want)
    ref.abs().mean().backward()
    ref = ref.detach()
    prior = want["prior"].detach()
    pad = ~cs["valid"]

    def args(texts):
        return (dev(texts), dev(tl), dev(ali), dev(cs["pitch"]), dev(cs["energy"]), dev(cs["voiced"]), dev(cs["style"]),
                dev(cs["pitch"]))

    # ---- inference ----
    m = S.SpeechPredictor()
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected and all(".stft." in k for k in missing)
    m = m.to(DEV)
    audio, taps = {}, {}
    for v in ("a", "b"):
        taps[v] = dict(tap_text_encoding=torch.zeros(B, 128, L, device=DEV), tap_decoder_out=torch.zeros(B, 128, T, device=DEV))
        with torch.no_grad():
            audio[v] = m(*args(cs["texts_" + v]), noise=dev(cs["noise"]), prior_override=dev(prior), taps=taps[v]).audio.cpu()
    torch.cuda.synchronize()
    rep = Report()
    rep.add("text_encoding", taps["a"]["tap_text_encoding"], want["text_encoding"], 1e-5)
    rep.add("decoder_out", taps["a"]["tap_decoder_out"], want["decoder_out"], 1e-5)
    enc = taps["a"]["tap_text_encoding"].cpu()
    assert (enc.transpose(1, 2)[pad] == 0).all(), "text_encoding tap: padded columns not exactly 0"
    assert torch.equal(enc, taps["b"]["tap_text_encoding"].cpu()), "text_encoding: padded ids leak"
    assert torch.equal(audio["a"], audio["b"]), f"inference audio: padded ids leak, max {(audio['a'] - audio['b']).abs().max().item():.3e}"
    mse, ml1 = ((audio["a"] - ref) ** 2).mean().item(), _mel_l1(audio["a"], ref)
    print(f"\n  inference audio vs oracle: max|err| {(audio['a'] - ref).abs().max().item():.3e} mse {mse:.3e} mel-L1 {ml1:.3e}")
    assert mse <= 1e-8 and ml1 <= 1e-3
    # ---- training graph, both token variants ----
    cot = dev(torch.sign(ref) / ref.numel())
    res = {}
    for v in ("a", "b"):
        mt = S.SpeechPredictor()
        mt.load_state_dict(P, strict=False)
        mt = mt.to(DEV).enable_training()
        au = mt.forward_train(*args(cs["texts_" + v]), noise=dev(cs["noise"]), prior_override=dev(prior))
        d_style, d_energy = mt.backward(cot)
        torch.cuda.synchronize()
        named = dict(mt.named_parameters())
        res[v] = dict(audio=au.cpu(), d_style=d_style.cpu(), d_energy=d_energy.cpu(),
                      grads={k: named[k].grad.detach().cpu().clone() for k in keys})
    assert torch.equal(res["a"]["audio"], res["b"]["audio"]), "training-graph audio: padded ids leak"
    mse, ml1 = ((res["a"]["audio"] - ref) ** 2).mean().item(), _mel_l1(res["a"]["audio"], ref)
    print(f"  training-graph audio vs oracle: mse {mse:.3e} mel-L1 {ml1:.3e}")
    assert mse <= 1e-8 and ml1 <= 1e-3
    rep.add("d_style vs oracle", res["a"]["d_style"], style_r.grad, 3e-2)
    rep.add("d_energy vs oracle", res["a"]["d_energy"], energy_r.grad, 3e-2)
    for k in keys:
        rep.add("d " + k[-46:], res["a"]["grads"][k], Q[k].grad, 3e-2)
    lo, hi = RAGGED_PAD_IDS
    ga, gb = res["a"]["grads"][EMB], res["b"]["grads"][EMB]
    assert (Q[EMB].grad[lo:hi] == 0).all() and (Q[EMB].grad[0] == 0).all()  # (the reference arithmetic does the same)
    assert (gb[lo:hi] == 0).all(), f"d emb rows {lo}..{hi - 1} (padding only): {gb[lo:hi].abs().max().item():.3e}"
    assert (ga[0] == 0).all(), f"d emb row 0 (padding only): {ga[0].abs().max().item():.3e}"
    rep.done()


def test_pitch_energy_predictor_on_a_ragged_batch_at_c3_text_length():
    """PitchEnergyPredictor on the same batch, forward through the inference entry point and through forward_train, against
    the float64 oracle with the alignment of oracle.frontend.duration_to_alignment.  The graph's gate is 1e-3
    (test_second_stage_predictors_vs_reference_golden) and the fp32 oracle alone sits near 5e-4 from float64 on this batch
    (four AdaIN blocks behind three AdaLN layers amplify fp32 rounding), so the gate is computed here from the oracle:
    max(1e-3, 2 x the fp32 oracle's own distance from float64) per output; both distances are printed.  Token variants A
    and B bit-identical."""
    import stylish_tts_amd as S
    from oracle import predictors as OP
    from oracle.manifest import pitch_energy_predictor_manifest
    from oracle.weights import fill_state_dict
    cs = _frames_case()
    tl, ali = cs["text_lengths"], cs["alignment"]
    Pp = fill_state_dict(pitch_energy_predictor_manifest(), 4)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in Pp.items()}
    with torch.no_grad():
        f64, e64 = OP.pitch_energy_predictor(P64, cs["texts_a"], tl, ali.double(), cs["style"].double())
        f32, e32 = OP.pitch_energy_predictor(Pp, cs["texts_a"], tl, ali, cs["style"])
    own = dict(pitch=rel(f32, f64), energy=rel(e32, e64))
    gate = {k: max(1e-3, 2 * v) for k, v in own.items()}
    out = {}
    for v in ("a", "b"):
        pe = S.PitchEnergyPredictor()
        pe.load_state_dict(Pp)
        pe = pe.to(DEV)
        with torch.no_grad():
            f0, en = pe(dev(cs["texts_" + v]), dev(tl), dev(ali), dev(cs["style"]))
        pe.enable_training()
        f0t, ent = pe.forward_train(dev(cs["texts_" + v]), dev(tl), dev(ali), dev(cs["style"]))
        torch.cuda.synchronize()
        out[v] = dict(pitch=f0.cpu(), energy=en.cpu(), pitch_t=f0t.cpu(), energy_t=ent.cpu())
    print(f"\n  fp32 oracle vs float64 oracle: pitch {own['pitch']:.3e} energy {own['energy']:.3e}; gates "
          f"{gate['pitch']:.3e} / {gate['energy']:.3e}")
    for k in out["a"]:
        assert torch.equal(out["a"][k], out["b"][k]), f"{k}: padded ids leak, max {(out['a'][k] - out['b'][k]).abs().max().item():.3e}"
    rep = Report()
    rep.add("pitch (inference) vs float64", out["a"]["pitch"], f64, gate["pitch"])
    rep.add("energy (inference) vs float64", out["a"]["energy"], e64, gate["energy"])
    rep.add("pitch (training graph) vs float64", out["a"]["pitch_t"], f64, gate["pitch"])
    rep.add("energy (training graph) vs float64", out["a"]["energy_t"], e64, gate["energy"])
    rep.done()


# ---- kernel level ---------------------------------------------------------------------------------------------------------
def _alignment_inputs():
    """name -> (durations [B, L], multiplier)"""
    cases = {}
    for (L, lengths), cid in zip(RAGGED_CASES, CASE_IDS):
        cases[cid] = (make_ragged(L, lengths, T=FRAMES[L])["durations"], 1)
    # a zero duration in the MIDDLE of the valid tokens (rows sum to 208); one token that takes all 208 frames
    mid = torch.zeros(3, 100)
    mid[0, :52] = 4
    mid[0, 17] = 0
    mid[0, 18] = 8
    mid[1, :100] = 2
    mid[1, [0, 1, 50, 98]] = 0
    mid[1, [2, 51, 97, 99]] = 6
    mid[2, 0] = 208
    assert (mid.sum(1) == 208).all()
    cases["zero duration in the middle / one token of 208 frames"] = (mid, 1)
    one = torch.zeros(2, 100)
    one[0, 63] = 208
    one[1, 99] = 208
    cases["one token of 208 frames behind zero durations"] = (one, 1)
    # fractional durations: the expectation over the class table of the duration predictor's output on the first case
    from oracle import predictors as OP
    cs = _case(0)
    frac = OP.prediction_to_duration(_oracle64(0)[0], cs["text_lengths"]).float()
    cases["fractional (predicted) durations"] = (frac, 1)
    cases["fractional (predicted) durations x 3"] = (frac, 3)
    return cases


def test_alignment_kernel_on_ragged_durations():
    """sty_alignment_fwd (through DurationProcessor.duration_to_alignment, which takes the frame count as the reference does)
    on the five cases' durations with their zero tails, a zero duration in the middle of the valid tokens, one token that
    takes all frames, and fractional durations at multiplier 1 and 3, against oracle.frontend.duration_to_alignment.

    Gate: the kernel's existing 1e-6 (test_alignment: 40 tokens) is tighter than the reference arithmetic itself at these
    lengths -- the fp32 oracle's softmax sums 100 ... 130 terms one after the other and sits 1.4e-6 ... 1.7e-6 of the tensor's
    maximum from the float64 oracle on the integer durations (5.6e-7 at L = 37), 2.7e-6 / 5.8e-6 on the fractional ones at
    multiplier 1 / 3 -- so per input the gate is max(1e-6, 2 x the fp32 oracle's own distance from float64), both printed.
    First run on an MI355X, against the fp32 oracle: integer durations 5.3e-7 ... 1.8e-6 (inside that gate: rounding, not a
    defect), fractional durations 5.9e-6 and 2.5e-5 (OUTSIDE it, gates 5.4e-6 and 1.2e-5): the kernel kept the running sum
    of the durations in fp32, where torch.cumsum accumulates in double on the host; fixed in alignment_kernel."""
    import stylish_tts_amd as S
    from oracle import frontend, predictors as OP
    proc = S.DurationProcessor(16, 50)
    rep = Report()
    for name, (dur, mult) in _alignment_inputs().items():
        ref = frontend.duration_to_alignment(dur, mult)
        own = rel(ref, OP.duration_to_alignment(dur.double(), mult))
        got = proc.duration_to_alignment(dev(dur), mult)
        torch.cuda.synchronize()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        print(f"  {name[-48:]:48s} fp32 oracle vs float64 oracle {own:9.3e}")
        rep.add(name[-48:], got, ref, max(1e-6, 2 * own))
    rep.done()


@pytest.mark.parametrize("i", range(len(RAGGED_CASES)), ids=CASE_IDS)
def test_duration_loss_kernels_on_ragged_batches_vs_float64_autograd(i):
    """sty_prediction_to_duration and sty_duration_loss_fwd_bwd against float64 autograd of the closed forms of
    oracle/stages.py (per-row smooth-L1 mean, weighted cross entropy, LossLog normalisation) with a non-trivial
    d_duration_extra: losses 1e-5 relative, durations and d_pred 1e-5 of the tensor's maximum (the fp32 kernel-level gate;
    the fp32 closed form itself sits 1e-8 ... 1e-7 from float64 on these inputs), d_pred exactly 0 on padded positions."""
    import torch.nn.functional as F
    from oracle import predictors as OP
    from stylish_tts_amd import duration as D
    L, lengths = RAGGED_CASES[i]
    B, NC = len(lengths), 16
    tl = torch.tensor(lengths)
    valid = torch.arange(L)[None, :] < tl[:, None]
    g = torch.Generator().manual_seed(40 + i)
    pred = 2 * torch.randn(B, L, NC, generator=g)
    tgt = torch.randint(1, 51, (B, L), generator=g) * valid
    cw = 0.2 + torch.rand(NC, generator=g)
    extra = 1e-2 * torch.randn(B, L, generator=g)
    w_dur, w_ce = 8.0, 8.0
    cls = OP.dur_to_class(tgt)
    p64 = pred.double().requires_grad_(True)
    dur64 = OP.prediction_to_duration(p64, tl)
    ce = torch.nn.CrossEntropyLoss(weight=cw.double())
    l_dur = sum(F.smooth_l1_loss(dur64[b, :tl[b]], tgt[b, :tl[b]].double()) for b in range(B)) / B
    l_ce = sum(ce(p64[b, :tl[b]], cls[b, :tl[b]]) for b in range(B)) / B
    (w_dur * l_dur / (l_dur.detach() + 1e-9) + w_ce * l_ce / (l_ce.detach() + 1e-9) + (dur64 * extra.double()).sum()).backward()
    dur = D.prediction_to_duration(dev(pred), dev(tl))
    losses, d_pred = D.duration_losses(dev(pred), dev(tl), dev(tgt.float()), dev(cls), dev(cw), w_dur, w_ce, dev(extra))
    torch.cuda.synchronize()
    losses, d_pred, dur = losses.cpu(), d_pred.cpu(), dur.cpu()
    assert (dur[~valid] == 0).all() and (d_pred[~valid] == 0).all()
    rep = Report()
    rep.add("duration loss", losses[0], l_dur.detach(), 1e-5)
    rep.add("duration_ce loss", losses[1], l_ce.detach(), 1e-5)
    rep.add("duration", dur, dur64.detach(), 1e-5)
    rep.add("d_pred", d_pred, p64.grad, 1e-5)
    rep.done()
