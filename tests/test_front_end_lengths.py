"""The audio-side front end (csrc/frontend.hip, csrc/val_loss.hip) at the lengths where its kernels change path, against the
float64 oracle.

Under every training step sit the three-resolution STFT features, the mel and multi-phase losses and the gradient the acoustic
stage starts from; tests/test_hip_parity.py checks them against the oracle at N = 24000 (N % 4 == 0) and the mel front end at
N = 26100 (an even frame count: no trim).  The lengths here (tests/cases.py FRONT_END_CASES, MEL_FRONT_CASES) sit on the edges
of stft_fft_kernel's 16-byte path, of the 16- and 8-frame tiles, of the workgroup map, of span_gather_kernel's mirrors, of the
time differences of the loss kernels across utterance borders and of launch_mel's frame trim.
tests/test_front_end_oracle.py pins on the CPU what the gates here assume: the fp32 oracle inside half of each of them, a
one-sample framing error far outside them, and the kink margins that make the element-wise check take its signs from the device.

Runs on the GPU box only (`-m gpu`).
"""
import functools

import pytest
import torch

from tests.cases import FRONT_END_CASES, MEL_FRONT_CASES
from tests.test_front_end_oracle import (CASE_IDS, FP32_D_WORST, GATE_COS, GATE_D, GATE_FEAT, GATE_L2, GATE_MEL, GATE_MELFE,
                                         GATE_MELFE_L1, GATE_MPH, GATE_PHASE, edge_errors, frame_counts, injected_grad,
                                         mel_cotangents, mel_front_audio, oracle64, rel, rel_l2_cos, wrapped_phase_err)
from tests.test_ragged_lengths import Report

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = pytest.mark.parametrize("i", range(len(FRONT_END_CASES)), ids=CASE_IDS)
N_FFTS = (512, 1024, 2048)


def dev(t):
    return t.to(DEV)


def _features(gt, pred):
    """mel_loss(features=True) -> [(T, P)] x 3 on the CPU, [B,128,frames] (the device keeps them [128,B,frames])"""
    from stylish_tts_amd.losses import mel_loss
    _, feats = mel_loss(dev(gt), dev(pred), features=True)
    torch.cuda.synchronize()
    return [(t.cpu().permute(1, 0, 2).contiguous(), p.cpu().permute(1, 0, 2).contiguous()) for t, p in feats]


def _loss(gt, pred, **kw):
    from stylish_tts_amd.losses import acoustic_loss
    losses, d = acoustic_loss(dev(gt), dev(pred), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(d).all() and torch.isfinite(losses).all()
    return losses.cpu(), d.cpu()


@functools.lru_cache(maxsize=None)
def _hip_features(i):
    o = oracle64(i)
    return _features(o["gt"], o["pred"])


@CASES
def test_loss_features_vs_float64_oracle(i):
    """(a) The log1p-mel tensors of target and prediction that the mel term reduces (launch_loss_features: stft_fft_kernel,
    magphase_kernel, fb_sparse_fwd_kernel), all three resolutions, at the gate test_multi_spectrogram has for the same tensor,
    and the frame counts."""
    B, N = FRONT_END_CASES[i]
    o = oracle64(i)["full"]
    feats = _hip_features(i)
    assert [t.shape[2] for t, _ in feats] == frame_counts(N)
    rep = Report()
    for r, n_fft in enumerate(N_FFTS):
        for side, got in zip("TP", feats[r]):
            assert got.shape == o[side][r][0].shape == (B, 128, N // (128 << r) + 1)
            rep.add(f"log1p mel128 {n_fft} {side} ({got.shape[2]} frames)", got, o[side][r][0], GATE_FEAT)
    print(f"\n  B={B} N={N}")
    rep.done()


@CASES
def test_multi_spectrogram_vs_float64_oracle(i):
    """(b) MultiSpectrogram.calculate -- frame_kernel + the dense DFT and filter-bank GEMMs of sty_multispec_fwd, the other
    implementation of the same features -- with the gates of test_multi_spectrogram: |X| and log1p-mel 1e-5 of the maximum,
    phase 5e-3 rad where the reference |X| > 2e-3."""
    from stylish_tts_amd.frontend import MultiSpectrogram
    B, N = FRONT_END_CASES[i]
    o = oracle64(i)
    ms = MultiSpectrogram(sample_rate=24000)
    rep = Report()
    for side, audio in (("T", o["gt"]), ("P", o["pred"])):
        with torch.no_grad():
            mags, phases, ffts = ms.calculate(dev(audio))
        torch.cuda.synchronize()
        for r, n_fft in enumerate(N_FFTS):
            r_mag, r_phase, r_fft = o["full"][side][r]
            assert mags[r].shape == (B, 1, 128, r_mag.shape[2]) and phases[r].shape == r_phase.shape
            rep.add(f"fft_mag {n_fft} {side}", ffts[r][:, 0], r_fft, GATE_FEAT)
            rep.add(f"log1p mel128 {n_fft} {side}", mags[r][:, 0], r_mag, GATE_FEAT)
            err = wrapped_phase_err(phases[r], r_phase, r_fft)
            rep.rows.append(f"  phase {n_fft:5d} {side} (gated){'':30s} max wrapped err {err:9.3e}  tol {GATE_PHASE:.1e}")
            if not err <= GATE_PHASE:
                rep.bad.append(f"phase {n_fft} {side}")
    print(f"\n  B={B} N={N}")
    rep.done()


@functools.lru_cache(maxsize=None)
def _hip_loss(i, w_phase=8.0):
    o = oracle64(i)
    return _loss(o["gt"], o["pred"], w_mel=5.0, w_phase=w_phase)


@CASES
def test_loss_values_vs_float64_oracle(i):
    """(c) acoustic_loss: mel 1e-5 and multi-phase 1e-4 relative (loss_sums_kernel's time and frequency differences inside
    [F][B][frames], loss_finalize_kernel's element counts)."""
    B, N = FRONT_END_CASES[i]
    o = oracle64(i)["full"]
    losses, _ = _hip_loss(i)
    e_mel, e_mph = abs(losses[0].item() - o["mel"]) / o["mel"], abs(losses[1].item() - o["mph"]) / o["mph"]
    print(f"\n  B={B} N={N}: mel {losses[0].item():.7f} vs {o['mel']:.7f} (rel {e_mel:.2e})   "
          f"multi_phase {losses[1].item():.7f} vs {o['mph']:.7f} (rel {e_mph:.2e})")
    assert e_mel <= GATE_MEL and e_mph <= GATE_MPH


@CASES
def test_mel_term_gradient_element_by_element(i):
    """(d) The smooth part of the backward chain -- log1p_bwd_kernel, fb_sparse_bwd_kernel, magphase_bwd_kernel,
    stft_fft_adj_kernel in span mode, span_gather_kernel -- held element by element.  acoustic_loss(w_mel=5, w_phase=0) against
    float64 autograd through the oracle's log1p-mel features of the prediction under the cotangent -k_r sign(T_dev - P_dev),
    k_r = w_mel / (mel + 1e-9) / 3 / (sum |T_dev| + 1e-6): the signs and sums are those of the device's own features (read back
    through mel_loss, which holds bit for bit what the loss call reduces), so no kink can move -- the two-halves idiom of
    tests/test_discriminators.py.  Error relative to the reference's maximum.

    Gate: the fp32 oracle deviates from the float64 oracle by at most 1.24e-6 under the same kind of cotangent on these cases
    (FP32_D_WORST, test_front_end_oracle.py); GATE_D = 20 x 1.25e-6 = 2.5e-5.  The margin is for the LDS FFT and the tile-wise
    overlap-add ordering their sums differently from torch.stft's backward, nothing else.  Measured on an MI355X: 1.5e-6 ...
    2.7e-6 over the seven cases, the same at the two ends of the signal as in the middle.  (span_gather_kernel without the left
    mirror of sample 1, or adding one of the two tiles that cover a position only: 0.20 ... 0.41.)"""
    B, N = FRONT_END_CASES[i]
    o = oracle64(i)
    feats = _hip_features(i)
    cots = mel_cotangents([t for t, _ in feats], [p for _, p in feats])
    ref = injected_grad(o["pred"], cots, torch.float64)
    _, d = _hip_loss(i, 0.0)
    e = rel(d, ref)
    edges = edge_errors(d, ref, N)
    print(f"\n  B={B} N={N}: d_audio (mel term) rel_err {e:.3e}  gate {GATE_D:.1e} (fp32 oracle {FP32_D_WORST:.2e})  "
          f"max|ref| {ref.abs().max().item():.3e}")
    for k, n_fft in enumerate(N_FFTS):
        print(f"    first / last {n_fft // 2} samples: {edges[2 * k]:.3e} / {edges[2 * k + 1]:.3e}")
    assert e <= GATE_D


@CASES
def test_full_gradient_vs_float64_oracle(i):
    """(e) Default weights (mel 5, multi-phase 8): loss_grad_kernel's phase term with its time differences, magphase_bwd_kernel's
    phase branch.  Signs flip at kinks, so in aggregate: relative L2 2e-2, cosine 0.9995 -- at these lengths a one-sample framing
    error moves the relative L2 by 0.10 or more (test_front_end_oracle.py).  (What this gate does NOT see at every length is a
    time difference of loss_grad_kernel that crosses an utterance border: with `t > 0` replaced by `i > 0` the relative L2 is
    2.5e-2 ... 8.3e-2 up to N = 4096 but 1.2e-2 from N = 8700 on.  test_a_batch_equals_its_rows sees it at every length.)"""
    B, N = FRONT_END_CASES[i]
    ref = oracle64(i)["full"]["grad"]
    _, d = _hip_loss(i)
    l2, cos = rel_l2_cos(d, ref)
    print(f"\n  B={B} N={N}: d_audio relative L2 {l2:.3e}  cosine {cos:.7f}  max|ref| {ref.abs().max().item():.3e}")
    assert l2 <= GATE_L2 and cos >= GATE_COS


def _bits(t):
    return t.contiguous().view(torch.int32)


@CASES
def test_target_computed_ahead_equals_the_one_call_form(i):
    """(f) acoustic_loss(target=acoustic_loss_target(gt)) -- audio_gt = NULL in the library, the target features already in the
    workspace -- gives the bits of the one-call form in the losses and in d_audio.  (loss_sums_kernel adds its five sums with
    float64 atomics in no fixed order; the terms are fp32 values, so the order moves a sum by about 1e-16 of itself and the
    fp32 values formed from it -- the losses, the two scale factors of loss_grad_kernel -- come out the same.)"""
    from stylish_tts_amd.losses import acoustic_loss_target
    o = oracle64(i)
    losses, d = _hip_loss(i)
    tg = acoustic_loss_target(dev(o["gt"]))
    losses2, d2 = _loss(o["gt"], o["pred"], target=tg)
    assert torch.equal(_bits(losses), _bits(losses2)), (losses.tolist(), losses2.tolist())
    assert torch.equal(_bits(d), _bits(d2)), (d - d2).abs().max().item()
    # a second loss call on the same target: the prediction side leaves the target side of the workspace alone
    losses3, d3 = _loss(o["gt"], o["pred"], target=tg)
    assert torch.equal(_bits(losses), _bits(losses3)) and torch.equal(_bits(d), _bits(d3))


@CASES
def test_a_batch_equals_its_rows(i):
    """(f) No tolerance.  The features of the batch are, row by row, the bits of every utterance run alone (a frame tile or a
    workgroup id reaching into the neighbouring utterance shows here).  For d_audio the cotangent scale depends on the batch's
    sums, so the batch is one utterance repeated: every row must then carry the same bits, with the mel term alone and with
    default weights -- the first row has no utterance before it and the last none after it, so a time difference, a span or a
    mirror that crosses an utterance border makes them differ."""
    B, N = FRONT_END_CASES[i]
    o = oracle64(i)
    feats = _hip_features(i)
    for b in range(B):
        alone = _features(o["gt"][b:b + 1], o["pred"][b:b + 1])
        for r in range(3):
            for side in range(2):
                assert torch.equal(_bits(alone[r][side][0]), _bits(feats[r][side][b])), (b, N_FFTS[r], "TP"[side])
    rows = max(B, 2)
    b = B - 1
    gt, pred = o["gt"][b:b + 1].repeat(rows, 1), o["pred"][b:b + 1].repeat(rows, 1)
    for w_phase in (0.0, 8.0):
        _, d = _loss(gt, pred, w_mel=5.0, w_phase=w_phase)
        assert d.abs().max().item() > 0
        for k in range(1, rows):
            assert torch.equal(_bits(d[0]), _bits(d[k])), (w_phase, k, (d[0] - d[k]).abs().max().item())


@functools.lru_cache(maxsize=None)
def _mel_oracle64(N, n_fft, win):
    from oracle import frontend as ofe
    audio = mel_front_audio(N, n_fft)
    ref = ofe.calculate_mel(audio.double(), n_fft, win, 300)
    return audio, ref, ofe.log_energy(ref)


@pytest.mark.parametrize("n_fft,win", [(512, 512), (2048, 1200)])
@pytest.mark.parametrize("N", MEL_FRONT_CASES)
def test_mel_front_end_vs_float64_oracle(N, n_fft, win):
    """(g) calculate_mel + log energy (sty_mel_fwd: stft_fft_kernel on 16- and 8-frame tiles, power_kernel, fb_sparse_fwd_kernel,
    mel_finalize_kernel) with the gates of test_mel_front_end, the trimmed frame count and the returned length."""
    from stylish_tts_amd.frontend import MelSpec, calculate_mel
    audio, ref, ref_e = _mel_oracle64(N, n_fft, win)
    mel, length, energy = calculate_mel(dev(audio), MelSpec(n_fft, win, 300), -4.0, 4.0, want_energy=True)
    torch.cuda.synchronize()
    frames = N // 300 + 1
    frames -= frames % 2
    assert mel.shape == ref.shape == (3, 80, frames) and energy.shape == (3, frames)
    assert length.tolist() == [frames] * 3
    l1 = (mel.cpu().double() - ref).abs().mean().item()
    print(f"\n  N={N} n_fft={n_fft} win={win}: {frames} frames  L1 {l1:.3e}")
    rep = Report()
    rep.add(f"mel n_fft={n_fft}", mel, ref, GATE_MELFE)
    rep.add("energy", energy, ref_e, GATE_MELFE)
    rep.done()
    assert l1 <= GATE_MELFE_L1
