"""The validation pass on the device (`-m gpu`): the forward-only loss entries of csrc/val_loss.hip against float64 restatements,
the three trainers' validate() against the eval-mode goldens, that validate() leaves no trace on a trainer, and the pass end to end
through stylish_tts_amd.train on the sample dataset."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"


def dev(t):
    return t.to(DEV)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _pair(B, N, seed):
    """a target and a prediction that differ everywhere: the stage tests' audio and a perturbed copy"""
    from tests.test_hip_parity import _test_audio
    gt = _test_audio(B, N, seed)
    g = torch.Generator().manual_seed(seed + 1)
    return gt, 0.8 * gt + 0.05 * torch.randn(B, N, generator=g)


# ---- loss entries: only the reduction is under test -----------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1025), (3, 1200), (2, 7200), (2, 24000)])
def test_mel_loss_fwd_vs_float64_restatement(B, N):
    """The features are the device's own (read back from the call's workspace); every summed term |t - p|, |t| is a non-negative
    fp32 value added in float64 and the result is rounded once: 1e-6 relative.  per_item reproduces loss[0] to the bit, the
    training entry agrees to 1 fp32 ulp, and a second call on the same buffers gives equal bits."""
    from stylish_tts_amd import lib as L
    from stylish_tts_amd.losses import acoustic_loss, mel_loss
    lib = L.load()
    gt, pr = _pair(B, N, 21)
    gt, pr = dev(gt), dev(pr)
    loss, items, feats = mel_loss(gt, pr, per_item=True, features=True)
    torch.cuda.synchronize()
    acc = 0.0
    it = items.cpu()
    for r, (t, p) in enumerate(feats):
        t, p = t.cpu(), p.cpu()
        assert t.shape == (128, B, N // (128 << r) + 1)
        num, den = (t - p).abs().double(), t.abs().double()
        acc += float(num.sum()) / (float(den.sum()) + 1e-6)
        for b in range(B):  # every utterance's own numerator and denominator
            for k, want in ((0, float(num[:, b].sum())), (1, float(den[:, b].sum()))):
                assert abs(float(it[b, r, k]) - want) <= 1e-12 * want, (r, b, k)
    want = float(np.float32(acc / 3.0))
    got = loss.item()
    print(f"\n  mel B={B} N={N}: {got:.9g} vs float64 restatement {want:.9g} (rel {abs(got - want) / want:.2e})")
    assert abs(got - want) <= 1e-6 * want
    mel = 0.0
    for r in range(3):  # per_item, items in index order, is what loss[0] is made of
        num = den = 0.0
        for b in range(B):
            num += float(it[b, r, 0])
            den += float(it[b, r, 1])
        mel += num / (den + 1e-6)
    assert float(np.float32(mel / 3.0)) == got
    both, _ = acoustic_loss(gt, pr)
    torch.cuda.synchronize()
    assert abs(both[0].item() - got) <= _ulp32(got), (both[0].item(), got)
    # the same buffers twice
    need = C.c_size_t()
    L.check(lib.sty_mel_loss_workspace_bytes(B, N, C.byref(need)))
    ws = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
    out = [(torch.empty(1, device=DEV), torch.empty(B, 3, 2, dtype=torch.float64, device=DEV)) for _ in range(2)]
    for lo, pi in out:
        L.check(lib.sty_mel_loss_fwd(B, N, L.ptr(gt), L.ptr(pr), L.ptr(lo), L.ptr(pi), L.ptr(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32)) and out[0][0].item() == got
    assert torch.equal(out[0][1].view(torch.int64), out[1][1].view(torch.int64))
    L.check(lib.sty_mel_loss_fwd(B, N, L.ptr(gt), L.ptr(pr), L.ptr(out[0][0]), None, L.ptr(ws), ws.numel(), _stream()))  # per_item NULL
    torch.cuda.synchronize()
    assert out[0][0].item() == got


def _sl1(d):
    return torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)


@pytest.mark.parametrize("T", [1, 2, 65])
def test_pitch_loss_fwd_vs_float64_restatement(T):
    from stylish_tts_amd import lib as L
    from stylish_tts_amd.textual import pitch_loss, pitch_loss_value
    lib = L.load()
    B = 3
    g = torch.Generator().manual_seed(T)
    tg = 200.0 + 50.0 * torch.randn(B, T, generator=g)
    pr = tg + 1.5 * torch.randn(B, T, generator=g)  # |d| on both sides of the smooth-L1 knee
    a = float(_sl1(pr - tg).double().sum())  # fp32 terms, as the kernel forms them, added in float64
    c = float(_sl1((pr[:, 1:] - pr[:, :-1]) - (tg[:, 1:] - tg[:, :-1])).double().sum()) if T > 1 else 0.0
    want = float(np.float32(a / (B * T) + (c / (B * (T - 1)) if T > 1 else 0.0)))
    d_tg, d_pr = dev(tg), dev(pr)
    got = pitch_loss_value(d_tg, d_pr).item()
    print(f"\n  pitch T={T}: {got:.9g} vs {want:.9g} (rel {abs(got - want) / want:.2e})")
    assert abs(got - want) <= 1e-6 * want
    grad = torch.zeros(B, T, device=DEV)
    assert abs(pitch_loss(d_tg, d_pr, 1.0, grad).item() - got) <= _ulp32(got)
    ws = torch.zeros(16 * B, dtype=torch.uint8, device=DEV)
    out = [torch.empty(1, device=DEV) for _ in range(2)]
    for lo in out:
        L.check(lib.sty_pitch_loss_fwd(B, T, L.ptr(d_tg), L.ptr(d_pr), L.ptr(lo), L.ptr(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)) and out[0].item() == got


def _exact_duration_case(lengths, L_, NC, seed):
    """Logits whose softmax is exact in fp32 -- k = 2, 4 or 8 classes at the maximum, the rest 203 below it (expf gives 0) -- so
    that every per-token term the kernel forms is known on the host: p = 1 / k, S = 1, E = mean of the chosen table entries
    (dyadic), the target class among the chosen.  What is left to the device is logf(1 / k) (1 ulp) and the reduction."""
    from stylish_tts_amd.duration import CLASS_TO_DUR
    rs = np.random.RandomState(seed)
    B = len(lengths)
    pred = np.full((B, L_, NC), -200.0, np.float32)
    tgt = rs.randint(1, 50, (B, L_)).astype(np.float32)
    cls = np.zeros((B, L_), np.int64)
    cw = np.sqrt(np.linspace(0.5, 2.0, NC)).astype(np.float32)
    tab = np.asarray(CLASS_TO_DUR, np.float32)
    dur, ce, wsum = np.zeros(B), np.zeros(B), np.zeros(B)
    for b in range(B):
        for l in range(L_):
            k = int(rs.choice([2, 4, 8]))
            chosen = rs.choice(NC, k, replace=False)
            pred[b, l, chosen] = 3.0
            cls[b, l] = y = int(chosen[0])
            if l < lengths[b]:
                d = np.float32(tab[chosen].sum() / k) - tgt[b, l]
                dur[b] += float(0.5 * d * d if abs(d) < 1 else abs(d) - 0.5)
                ce[b] += float(np.float32(cw[y]) * np.float32(-np.log(np.float32(1.0 / k))))
                wsum[b] += float(cw[y])
    want = (float(np.float32(sum(dur[b] / (lengths[b] * B) for b in range(B)))),
            float(np.float32(sum(ce[b] / (wsum[b] * B) for b in range(B)))))
    return torch.from_numpy(pred), torch.tensor(lengths), torch.from_numpy(tgt), torch.from_numpy(cls), torch.from_numpy(cw), want


@pytest.mark.parametrize("lengths,L_", [((1, 1), 1), ((9,), 9), ((70, 1, 33), 70)])
def test_duration_loss_fwd_vs_float64_restatement(lengths, L_):
    from stylish_tts_amd import lib as L
    from stylish_tts_amd.duration import CLASS_TO_DUR, duration_loss_values, duration_losses
    lib = L.load()
    NC, B = 16, len(lengths)
    pred, tl, tgt, cls, cw, want = _exact_duration_case(lengths, L_, NC, 7 + L_)
    got = duration_loss_values(dev(pred), dev(tl), dev(tgt), dev(cls), dev(cw)).cpu().tolist()
    print(f"\n  duration B={B} L={L_}: duration {got[0]:.9g} vs {want[0]:.9g}, ce {got[1]:.9g} vs {want[1]:.9g}")
    for a, w in zip(got, want):
        assert abs(a - w) <= 1e-6 * w
    # ordinary logits: against the training entry, 1 fp32 ulp
    g = torch.Generator().manual_seed(5)
    pred = 2.0 * torch.randn(B, L_, NC, generator=g)
    a = duration_loss_values(dev(pred), dev(tl), dev(tgt), dev(cls), dev(cw)).cpu().tolist()
    b, _ = duration_losses(dev(pred), dev(tl), dev(tgt), dev(cls), dev(cw), 1.0, 1.0)
    b = b.cpu().tolist()
    for x, y in zip(a, b):
        assert abs(x - y) <= _ulp32(y), (a, b)
    d = [dev(t) for t in (pred, tl, tgt, cls, torch.tensor(CLASS_TO_DUR, dtype=torch.float32), cw)]
    ws = torch.zeros(16 * B, dtype=torch.uint8, device=DEV)
    out = [torch.empty(2, device=DEV) for _ in range(2)]
    for lo in out:
        L.check(lib.sty_duration_loss_fwd(B, L_, NC, *[L.ptr(t) for t in d], L.ptr(lo), L.ptr(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)) and out[0].cpu().tolist() == a


def test_loss_entries_refuse_bad_arguments_with_device_buffers():
    from stylish_tts_amd import lib as L
    from stylish_tts_amd.lib import StyError
    from stylish_tts_amd.losses import mel_loss
    lib = L.load()
    x = torch.zeros(2, 2048, device=DEV)
    need = C.c_size_t()
    L.check(lib.sty_mel_loss_workspace_bytes(2, 2048, C.byref(need)))
    ws = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    assert lib.sty_mel_loss_fwd(2, 2048, L.ptr(x), L.ptr(x), None, None, L.ptr(ws), ws.numel(), _stream()) != 0  # NULL output
    assert lib.sty_mel_loss_fwd(2, 1024, L.ptr(x), L.ptr(x), L.ptr(loss), None, L.ptr(ws), ws.numel(), _stream()) != 0
    assert lib.sty_mel_loss_fwd(2, 2048, L.ptr(x), L.ptr(x), L.ptr(loss), None, L.ptr(ws), ws.numel() - 1, _stream()) != 0
    assert lib.sty_pitch_loss_fwd(2, 8, L.ptr(x), L.ptr(x), L.ptr(loss), L.ptr(ws), 31, _stream()) != 0
    torch.cuda.synchronize()
    assert loss.item() == 7.0  # nothing was launched
    with pytest.raises(StyError):
        mel_loss(torch.zeros(2, 1024, device=DEV), torch.zeros(2, 1024, device=DEV))
    with pytest.raises(StyError):
        mel_loss(torch.zeros(2, 2048), torch.zeros(2, 2048))  # no CPU path


# ---- validate() of the three trainers ---------------------------------------------------------------------------------------------
def _snapshot(tr, models):
    import copy
    assert hasattr(tr, "_rng"), type(tr).__name__  # every trainer draws from `_rng`: the no-draw check must not pass vacuously
    return dict(state=[{k: v.detach().clone() for k, v in m.state_dict().items()} for m in models],
                rng=[copy.deepcopy(getattr(tr, n).getstate()) for n in ("_rng", "_shared_rng") if hasattr(tr, n)],
                t=[o.t for o in tr.opt.values()],
                opts=[bytes(m._train_opts) if getattr(m, "_train_opts", None) is not None else None for m in models])


def _assert_untouched(tr, models, before):
    after = _snapshot(tr, models)
    for a, b in zip(before["state"], after["state"]):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k  # parameters AND buffers (BatchNorm statistics, spectral-norm u / v)
    assert before["rng"] == after["rng"] and before["t"] == after["t"]
    assert before["opts"] == after["opts"]  # the train opts the next train_batch runs with


from tests.test_hip_parity import env  # noqa: E402,F401  (the module fixture of the parity tests: case, weights, oracle audio)


def test_acoustic_validate_vs_oracle_and_leaves_no_trace(env):
    """validate_acoustic on the eval-mode fixture of test_acoustic_train_step_gradients: the mel loss within that test's bound
    (1e-4 relative); the trainer's models, generators, optimizers and train opts are untouched, and a train_batch (lr = 0,
    train_mode=False) logs after it what it logged before it."""
    from oracle import losses as ol, speech_predictor as osp
    from tests.test_hip_parity import _test_audio, _train_setup
    cs = env["cs"]
    B, T = cs["pitch"].shape
    audio_gt = _test_audio(B, 300 * T, 21)
    tr, P, Pse = _train_setup(env, 0.0)
    want = {}
    with torch.no_grad():
        ref = osp.acoustic_forward(P, Pse, audio_gt, cs["texts"], cs["text_lengths"], cs["pitch"], cs["durations"], cs["noise"], want)
        mel, _, _ = ol.acoustic_losses(audio_gt, ref.squeeze(1))
    kw = dict(audio_gt=dev(audio_gt), texts=dev(cs["texts"]), text_lengths=dev(cs["text_lengths"]), pitch=dev(cs["pitch"]),
              durations=dev(cs["durations"]), noise=dev(cs["noise"]), prior_override=dev(want["prior"]))
    first = tr.train_batch(**kw).cpu()
    models = (tr.sp, tr.se)
    before = _snapshot(tr, models)
    assert len(before["rng"]) == 2  # `_rng` and `_shared_rng` (which discriminator a step trains)
    log, out = tr.validate(**kw)
    torch.cuda.synchronize()
    _assert_untouched(tr, models, before)
    got = log["mel"].item()
    print(f"\n  validate_acoustic mel {got:.6f} vs oracle {mel.item():.6f}")
    assert set(log) == {"mel"} and abs(got - mel.item()) <= 1e-4 * abs(mel.item())
    assert out["audio"].shape == (B, 1, 300 * T) and out["per_item"].shape == (B, 3, 2)
    again, _ = tr.validate(**kw)
    assert again["mel"].item() == got  # the same batch twice: the same bits
    second = tr.train_batch(**kw).cpu()
    assert abs(second[0] - first[0]) <= 1e-4 * first[0] and abs(second[1] - first[1]) <= 1e-3 * first[1], (first, second)


def _shell(cls, P, **kw):
    m = cls(**kw)
    m.load_state_dict({k: v.detach() for k, v in P.items()}, strict=False)
    return m.to(DEV)


def test_textual_validate_vs_reference_golden_and_leaves_no_trace():
    """validate_textual against what the REFERENCE logged on these inputs with every model in .eval()
    (tests/golden/stages_small.safetensors `textual.log.*`), at the bound of test_textual_train_step_vs_oracle: 2e-3."""
    import stylish_tts_amd as S
    from oracle import stages
    from stylish_tts_amd.discriminators import PitchDiscriminator
    from stylish_tts_amd.textual import TextualTrainer
    from tests.test_oracle_golden import stage_inputs
    fx, P, cs = stage_inputs()
    want = {}
    with torch.no_grad():  # the harmonic source's output of the oracle's run pins SineGen's phase accumulation, as in that test
        stages.train_textual(P["pep"], P["pse"], P["sp"], P["se"], P["pitch_disc"], fx["audio_gt"], cs["texts"], cs["text_lengths"],
                             cs["pitch"], cs["durations"], cs["noise"], want)
    pd = PitchDiscriminator(dim_in=2, kernel=21)
    pd.load_state_dict(P["pitch_disc"])
    tr = TextualTrainer(_shell(S.PitchEnergyPredictor, P["pep"]), _shell(S.PitchStyleEncoder, P["pse"]),
                        _shell(S.SpeechPredictor, P["sp"]), _shell(S.MelStyleEncoder, P["se"]), pd.to(DEV), lr=0.0, train_mode=False)
    kw = dict(audio_gt=dev(fx["audio_gt"]), texts=dev(cs["texts"]), text_lengths=dev(cs["text_lengths"]), pitch=dev(cs["pitch"]),
              durations=dev(cs["durations"]), noise=dev(cs["noise"]), prior_override=dev(want["prior"]))
    first = {k: v.item() for k, v in tr.train_batch(**kw).items()}
    models = (tr.pep, tr.pse, tr.sp, tr.se, tr.pitch_disc)
    before = _snapshot(tr, models)
    log, out = tr.validate(**kw)
    torch.cuda.synchronize()
    _assert_untouched(tr, models, before)
    assert set(log) == {"mel", "pitch", "energy"}
    print("\n  validate_textual " + "  ".join(f"{k} {log[k].item():.5f} (reference {fx['textual.log.' + k].item():.5f})" for k in log))
    for k in log:
        ref = fx["textual.log." + k].item()
        assert abs(log[k].item() - ref) <= 2e-3 * ref, (k, log[k].item(), ref)
    assert out["audio"].shape == (2, 1, fx["audio_gt"].shape[1])
    second = {k: v.item() for k, v in tr.train_batch(**kw).items()}
    for k in first:
        assert abs(second[k] - first[k]) <= 2e-3 * abs(first[k]), (k, first[k], second[k])


def test_duration_validate_vs_reference_golden_audio_and_leaves_no_trace():
    """validate_duration: the two losses against the reference's eval-mode log (stages_small `duration.log.*`, 1e-4 as
    test_duration_train_step_vs_oracle), and the B = 1 synthesis from the PREDICTED durations against what the reference's own
    validate_duration produced (tests/golden/validate_small.safetensors, tools/gen_golden_validate.py): equal frame totals; the
    audio at the two bounds test_export_model_text_to_audio_vs_oracle applies (waveform mse <= 1e-6, mel-L1 <= 1e-3; the fixture's
    strided sample is the whole waveform at these lengths) and the L2 norm within what that mse allows (sqrt(n 1e-6)).
    Measured: profiles/validate_parity_table.txt."""
    import stylish_tts_amd as S
    from safetensors.torch import load_file
    from stylish_tts_amd.discriminators import PitchDiscriminator
    from stylish_tts_amd.duration import DurationTrainer
    from stylish_tts_amd.lib import StyError
    from tests.test_hip_parity import _mel_l1
    from tests.test_oracle_golden import stage_inputs
    fx, P, cs = stage_inputs()
    gold = load_file(os.path.join(G, "validate_small.safetensors"))
    dd = PitchDiscriminator(dim_in=1, kernel=5)
    dd.load_state_dict(P["dur_disc"])
    synth = {"pe_style_encoder": _shell(S.PitchStyleEncoder, P["pse"]), "pitch_energy_predictor": _shell(S.PitchEnergyPredictor, P["pep"]),
             "speech_predictor": _shell(S.SpeechPredictor, P["sp"]), "speech_style_encoder": _shell(S.MelStyleEncoder, P["se"])}
    tr = DurationTrainer(_shell(S.DurationPredictor, P["dp"]), _shell(S.MelStyleEncoder, P["dse"]), dd.to(DEV), fx["class_weights"],
                         lr=0.0, train_mode=False, synth_models=synth)
    B = cs["texts"].shape[0]
    frames = [int(v) for v in gold["frames"].tolist()]
    noise = {}
    for i in range(B):  # the draw the reference consumed under torch.manual_seed(noise_seed.<i>): rand[1, 9], then randn[1, 300 T, 9]
        g = torch.Generator().manual_seed(int(gold[f"noise_seed.{i}"]))
        torch.rand(1, 9, generator=g)
        noise[i] = dev(torch.randn(1, 300 * frames[i], 9, generator=g))
    prior = {i: dev(gold[f"prior.{i}"]) for i in range(B)}
    kw = dict(audio_gt=dev(fx["audio_gt"]), texts=dev(cs["texts"]), text_lengths=dev(cs["text_lengths"]), durations=dev(cs["durations"]))
    first = {k: v.item() for k, v in tr.train_batch(**kw).items()}
    models = (tr.dp, tr.se, tr.dur_disc) + tuple(synth.values())
    before = _snapshot(tr, models)
    log, out = tr.validate(pitch=dev(cs["pitch"]), samples=list(range(B)), noise=noise, prior_override=prior, **kw)
    torch.cuda.synchronize()
    _assert_untouched(tr, models, before)
    assert set(log) == {"duration", "duration_ce"}
    for k in log:
        ref = fx["duration.log." + k].item()
        print(f"\n  validate_duration {k} {log[k].item():.6f} (reference {ref:.6f})")
        assert abs(log[k].item() - ref) <= 1e-4 * ref, (k, log[k].item(), ref)
    assert out["frames"] == frames
    assert torch.allclose(out["duration"].cpu(), gold["duration"], rtol=1e-4, atol=1e-4)
    for i in range(B):
        a = out["audio"][i]
        assert not isinstance(a, Exception), a
        a = a.reshape(-1).cpu()
        n = a.numel()
        assert n == int(gold[f"audio_len.{i}"]) == 300 * frames[i]
        ref = gold[f"audio_sub.{i}"]
        whole = ref.numel() == n  # (the generator keeps at most 16384 values: these utterances whole)
        sub = a if whole else a[::n // 16384][:16384]
        mse = ((sub - ref) ** 2).mean().item()
        dn = abs(a.norm().item() - gold[f"audio_norm.{i}"].item())
        l1 = _mel_l1(a.reshape(1, 1, -1), ref.reshape(1, 1, -1)) if whole else float("nan")
        print(f"  utterance {i}: {frames[i]} frames, waveform mse {mse:.3e}, mel-L1 {l1:.3e}, |norm - golden| {dn:.3e} of {a.norm().item():.3f}")
        assert whole and mse <= 1e-6 and l1 <= 1e-3 and dn <= math.sqrt(n * 1e-6)
    # the numbers do not depend on the samples; an utterance the host checks refuse holds the error instead of audio
    log2, out2 = tr.validate(**kw)
    assert out2["audio"] == {} and all(log2[k].item() == log[k].item() for k in log)
    with pytest.raises(StyError):
        DurationTrainer._synthesize(synth, dev(cs["texts"][:1, :3]), 3, dev(torch.tensor([3])), torch.zeros(1, 3, device=DEV), 0,
                                    None, None, None, 0, None)
    second = {k: v.item() for k, v in tr.train_batch(**kw).items()}
    for k in first:
        assert abs(second[k] - first[k]) <= 1e-4 * abs(first[k]), (k, first[k], second[k])


def test_acoustic_validate_bf16_is_finite(env):
    """compute="bf16": the stage's operand mode also runs the validation forward, as the reference's autocast does.  Finite
    losses; the distance from the fp32 value is printed (profiles/validate_parity_table.txt), not gated: nobody has measured it.
    The train opts are the constructor's afterwards (the train_mode=False / bf16 path sets them once)."""
    from tests.test_hip_parity import _test_audio, _train_setup
    cs = env["cs"]
    B, T = cs["pitch"].shape
    kw = dict(audio_gt=dev(_test_audio(B, 300 * T, 21)), texts=dev(cs["texts"]), text_lengths=dev(cs["text_lengths"]),
              pitch=dev(cs["pitch"]), durations=dev(cs["durations"]), noise=dev(cs["noise"]))
    vals = {}
    for compute in ("fp32", "bf16"):
        tr, _, _ = _train_setup(env, 0.0, compute=compute)
        before = _snapshot(tr, (tr.sp, tr.se))
        log, out = tr.validate(**kw)
        torch.cuda.synchronize()
        _assert_untouched(tr, (tr.sp, tr.se), before)
        assert bool(torch.isfinite(out["audio"]).all())
        vals[compute] = log["mel"].item()
    print(f"\n  validate_acoustic mel: fp32 {vals['fp32']:.6f}, bf16 {vals['bf16']:.6f}, "
          f"relative distance {abs(vals['bf16'] - vals['fp32']) / vals['fp32']:.3e}")
    assert math.isfinite(vals["bf16"]) and vals["bf16"] > 0


def test_validate_on_a_train_mode_trainer_draws_nothing(env):
    """train_mode=True: train_batch draws the smoothing widths and the dropout seed from `_rng` and sets the models' train opts
    itself; validate() in between draws nothing and runs on BatchNorm running statistics (the same batch twice: equal bits, the
    running statistics unchanged)."""
    from tests.test_hip_parity import _test_audio, _train_setup
    cs = env["cs"]
    B, T = cs["pitch"].shape
    kw = dict(audio_gt=dev(_test_audio(B, 300 * T, 21)), texts=dev(cs["texts"]), text_lengths=dev(cs["text_lengths"]),
              pitch=dev(cs["pitch"]), durations=dev(cs["durations"]), noise=dev(cs["noise"]))
    tr, _, _ = _train_setup(env, 1e-4, train_mode=True)
    tr.train_batch(**kw)
    assert tr.sp._train_opts.dropout_seed != 0 and tr.sp._train_opts.bn_batch_stats == 1  # what the step left set
    before = _snapshot(tr, (tr.sp, tr.se))
    a, _ = tr.validate(**kw)
    b, _ = tr.validate(**kw)
    torch.cuda.synchronize()
    _assert_untouched(tr, (tr.sp, tr.se), before)
    assert a["mel"].item() == b["mel"].item() and math.isfinite(a["mel"].item())
    # eval-mode behaviour with those opts set: a fresh train_mode=False trainer (no train opts at all) holding the SAME weights
    # and buffers validates to the same value -- the acoustic parity bound, 1e-4; dropout at 0.2, smoothing or batch statistics
    # would move the loss by orders of magnitude more
    ev, _, _ = _train_setup(env, 0.0)
    ev.sp.load_state_dict(tr.sp.state_dict())
    ev.se.load_state_dict(tr.se.state_dict())
    assert getattr(ev.sp, "_train_opts", None) is None
    c, _ = ev.validate(**kw)
    torch.cuda.synchronize()
    print(f"\n  validate after a train-mode step {a['mel'].item():.9g} vs an eval-mode trainer with the same weights {c['mel'].item():.9g}")
    assert abs(a["mel"].item() - c["mel"].item()) <= 1e-4 * c["mel"].item()
    assert bool(torch.isfinite(tr.train_batch(**kw)).all())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _wav_info(path):
    import wave
    with wave.open(path, "rb") as f:
        return f.getframerate(), f.getsampwidth(), f.getnchannels(), f.getnframes()


def _tree(d):
    return {os.path.relpath(os.path.join(r, f), d): (os.path.getsize(os.path.join(r, f)), os.stat(os.path.join(r, f)).st_mtime_ns)
            for r, _, fs in os.walk(d) for f in fs}


def test_validation_pass_end_to_end_on_the_sample_dataset(tmp_path):
    """train(..., "acoustic", max_steps=4) at val_interval=2 on the 8-utterance sample dataset, batch 2: two validation lines, two
    JSON lines with finite totals, best_loss in checkpoint_final = the smaller total, the samples as 24 kHz PCM16; --validate-only
    on that checkpoint reproduces the last total and leaves the checkpoint directory as it was; then the duration stage from a
    chained checkpoint (one textual step, two duration steps), where an untrained model's sample may be skipped with a line."""
    import yaml
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_sample_dataset import make
    from stylish_tts_amd import stage_io as IO
    from stylish_tts_amd import train as T
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    root = tmp_path / "data"
    make(str(root), 8, 11)
    cfg, mdl, out = tmp_path / "config.yml", tmp_path / "model.yml", tmp_path / "out"
    d = yaml.safe_load(_default_config_yaml(root, acoustic=dict(epochs=3), duration=dict(epochs=3)))
    d["training"]["val_interval"] = 2
    cfg.write_text(yaml.safe_dump(d))
    mdl.write_text(_default_model_yaml())
    logs = []
    ctx = T.train(str(cfg), str(mdl), str(out), "acoustic", max_steps=4, log=logs.append)
    torch.cuda.synchronize()
    lines = [ln for ln in logs if ln.startswith("Validation step")]
    assert len(lines) == 2 and lines[0].startswith("Validation step 2: loss: ") and ", mel: " in lines[0]
    assert "best was" not in lines[0] and "(best was " in lines[1]
    ev = os.path.join(str(out), "acoustic", "eval")
    recs = [json.loads(ln) for ln in open(os.path.join(ev, "validation.jsonl"))]
    assert [r["step"] for r in recs] == [2, 4] and all(math.isfinite(r["total"]) and r["batches"] == 2 and not r["skipped"] for r in recs)  # (the two val utterances fall in two length bins)
    assert recs[0]["best_before"] is None and recs[1]["best_before"] == recs[0]["total"]
    assert abs(recs[0]["total"] - 5 * recs[0]["metrics"]["mel"]) <= 1e-9 * recs[0]["total"]  # loss_weight.mel = 5
    final = os.path.join(str(out), "acoustic", "checkpoint_final")
    man = IO.Manifest()
    IO.load_checkpoint(final, {}, manifest=man)
    best = min(r["total"] for r in recs)
    assert math.isfinite(man.best_loss) and man.best_loss == best == ctx.manifest.best_loss
    for name in (os.path.join(ev, "step_2", "sample_0.wav"), os.path.join(ev, "step_4", "sample_0.wav"), os.path.join(ev, "sample_0_gt.wav")):
        sr, width, ch, n = _wav_info(name)
        assert (sr, width, ch) == (24000, 2, 1) and n > 0, name
    assert recs[1]["samples"][0]["file"] == os.path.join("step_4", "sample_0.wav") and math.isfinite(recs[1]["samples"][0]["mel"])
    del ctx
    # --validate-only: one pass, no training, no save
    before = _tree(final)
    out2 = tmp_path / "out_val"
    T.main([str(cfg), "--model-config", str(mdl), "--out", str(out2), "--stage", "acoustic", "--checkpoint", final, "--validate-only"])
    torch.cuda.synchronize()
    assert _tree(final) == before
    rec = [json.loads(ln) for ln in open(os.path.join(str(out2), "acoustic", "eval", "validation.jsonl"))]
    assert len(rec) == 1 and rec[0]["step"] == 4
    assert abs(rec[0]["total"] - recs[1]["total"]) <= 1e-4 * recs[1]["total"], (rec[0]["total"], recs[1]["total"])
    assert not os.path.exists(os.path.join(str(out2), "acoustic", "checkpoint_final"))
    # the duration stage from a chained checkpoint
    T.train(str(cfg), str(mdl), str(out), "textual", checkpoint=final, max_steps=1, log=logs.append)
    tfinal = os.path.join(str(out), "textual", "checkpoint_final")
    assert not os.path.exists(os.path.join(str(out), "textual", "eval"))  # one step at val_interval = 2: no pass
    n0 = len(logs)
    ctx = T.train(str(cfg), str(mdl), str(out), "duration", checkpoint=tfinal, max_steps=2, log=logs.append)
    torch.cuda.synchronize()
    dlines = [ln for ln in logs[n0:] if ln.startswith("Validation step")]
    assert len(dlines) == 1 and "duration_ce: " in dlines[0] and "duration: " in dlines[0]
    dev_ = os.path.join(str(out), "duration", "eval")
    drec = [json.loads(ln) for ln in open(os.path.join(dev_, "validation.jsonl"))]
    assert len(drec) == 1 and math.isfinite(drec[0]["total"]) and ctx.manifest.best_loss == drec[0]["total"]
    assert [s["sample"] for s in drec[0]["samples"]] == [0, 1]  # validation.sample_count = 2: utterance 0 of both batches
    for s in drec[0]["samples"]:
        if "skipped" in s:  # untrained models: a refused sample is a log line, never an error
            assert any(f"sample {s['sample']} " in ln and "skipped" in ln for ln in logs[n0:])
        else:
            sr, width, ch, n = _wav_info(os.path.join(dev_, s["file"]))
            assert (sr, width, ch) == (24000, 2, 1) and n > 0 and n % 300 == 0
    assert _wav_info(os.path.join(dev_, "sample_0_gt.wav"))[3] > 0
    del ctx
    # the natural end of a stage: one epoch of the duration stage (four batches) at val_interval = 3 -- a pass after step 3 and one
    # where the epochs run out, in front of checkpoint_final (a pass that had just run at that step would not be repeated)
    d["training"]["val_interval"] = 3
    d["training_plan"]["duration"]["epochs"] = 1
    cfg3, out3 = tmp_path / "config3.yml", tmp_path / "out_end"
    cfg3.write_text(yaml.safe_dump(d))
    n0 = len(logs)
    ctx = T.train(str(cfg3), str(mdl), str(out3), "duration", checkpoint=tfinal, log=logs.append)
    torch.cuda.synchronize()
    erec = [json.loads(ln) for ln in open(os.path.join(str(out3), "duration", "eval", "validation.jsonl"))]
    steps = ctx.manifest.current_total_step
    assert [r["step"] for r in erec] == [steps - 1, steps] and len([ln for ln in logs[n0:] if ln.startswith("Validation step")]) == 2
    man = IO.Manifest()
    IO.load_checkpoint(os.path.join(str(out3), "duration", "checkpoint_final"), {}, manifest=man)
    assert man.best_loss == min(r["total"] for r in erec) and erec[0]["best_before"] is None  # best_loss starts over per stage
