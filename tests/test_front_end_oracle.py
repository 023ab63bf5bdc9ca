"""What tests/test_front_end_lengths.py (GPU) assumes about the reference arithmetic of the audio-side front end, pinned on the
CPU with the oracle alone on exactly the inputs of the GPU module (tests/cases.py FRONT_END_CASES, MEL_FRONT_CASES):

  * the reference is oracle.frontend / oracle.losses run in float64 (the mel filter bank and the phase weights are formed in
    fp32 inside the oracle, as the reference forms them, and cast); the fp32 oracle stays inside HALF of every gate of the GPU
    module against it, so no gate is tighter than the reference arithmetic itself allows;
  * the gates can see a framing error: a float64 restatement (manual padding, center=False) whose right-hand padding is
    `symmetric` instead of `reflect` -- one sample off -- moves the mel-only gradient and the full gradient by a stated factor
    over their gates; with `reflect` the restatement IS the oracle (1e-12);
  * the kink margins: the smallest non-zero |T - P| over the log1p-mel features is within a few fp32 roundings of a feature, so
    an fp32 implementation may put sign(T - P) on the other side there.  That is why the GPU module's element-wise gradient
    check takes the signs from the device's own features.
"""
import functools

import pytest
import torch

from tests.cases import FRONT_END_CASES, MEL_FRONT_CASES

SEED = 31  # the prediction's noise takes SEED + 1 (test_validation_gpu._pair)
# the gates of the GPU module.  All but GATE_D are the project's own (test_hip_parity.py: test_multi_spectrogram,
# test_acoustic_losses_forward_backward, test_mel_front_end)
GATE_FEAT = 1e-5     # log1p-mel features and |X|, of the tensor's maximum
GATE_PHASE = 5e-3    # wrapped phase error (rad) where the reference |X| > PHASE_ON
PHASE_ON = 2e-3
GATE_MEL = 1e-5      # mel loss, relative
GATE_MPH = 1e-4      # multi-phase loss, relative
GATE_L2 = 2e-2       # full gradient: relative L2 error ...
GATE_COS = 0.9995    # ... and cosine
GATE_MELFE = 1e-4    # calculate_mel: mel and log energy, of the tensor's maximum ...
GATE_MELFE_L1 = 1e-3  # ... and mean |error| of the mel
# Mel-only gradient under an injected cotangent, element by element, of the reference's maximum: 20 x the worst deviation of the
# fp32 oracle from the float64 oracle under the same cotangent on FRONT_END_CASES (FP32_D_WORST, measured by
# test_loss_oracle_on_front_end_cases, which asserts that it still holds)
FP32_D_WORST = 1.25e-6  # 1.24e-6 at (2, 8704)
GATE_D = 20 * FP32_D_WORST
# the symmetric-for-reflect framing error must move the gradients by at least this factor over their gates
SENS_D, SENS_L2 = 1000, 3
CASE_IDS = [f"B{B}-N{N}" for B, N in FRONT_END_CASES]


def rel(a, b):
    """max |a - b| relative to the maximum of the reference tensor b"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def rel_l2_cos(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return ((a - b).norm() / b.norm()).item(), torch.nn.functional.cosine_similarity(a, b, dim=0).item()


def wrapped_phase_err(got, ref_phase, ref_fft):
    """max |got - ref| modulo 2 pi over the bins where the reference |X| > PHASE_ON (test_multi_spectrogram)"""
    got, ref_phase = got.detach().double().cpu(), ref_phase.detach().double().cpu()
    d = torch.remainder(got - ref_phase + torch.pi, 2 * torch.pi) - torch.pi
    return (d.abs() * (ref_fft.detach().cpu() > PHASE_ON)).max().item()


def front_end_pair(B, N):
    """target and prediction [B, N]: the recipe of tests/test_validation_gpu._pair"""
    from tests.test_validation_gpu import _pair
    return _pair(B, N, SEED)


def mel_front_audio(N, n_fft):
    """[3, N], seeded as test_mel_front_end seeds it (by n_fft)"""
    from tests.test_hip_parity import _test_audio
    return _test_audio(3, N, n_fft)


def _restated_single(audio, n_fft, hop, right):
    """multi_spectrogram_single with the centre padding written out: left reflect, right `reflect` or `symmetric`"""
    from oracle.frontend import mel_filterbank
    h = n_fft // 2
    rp = audio[:, -h - 1:-1] if right == "reflect" else audio[:, -h:]
    x = torch.cat([audio[:, 1:h + 1].flip(1), audio, rp.flip(1)], dim=1)
    st = torch.stft(x, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, dtype=audio.dtype),
                    center=False, return_complex=True)
    fft_mag = torch.abs(st)
    phase = (fft_mag > 1e-3).detach() * torch.angle(st)
    fb = mel_filterbank(n_fft // 2 + 1, 128, 24000).to(fft_mag.dtype)
    return torch.log1p(torch.matmul(fft_mag.transpose(1, 2), fb).transpose(1, 2))[:, None], phase, fft_mag[:, None]


def features(audio, right=None):
    """three resolutions of (log1p-mel [B,128,frames], gated phase [B,F,frames], |X| [B,F,frames]) in audio's dtype through the
    oracle (right=None) or the restatement"""
    from oracle.frontend import RESOLUTIONS, multi_spectrogram_single
    out = []
    for fft, hop, win in RESOLUTIONS:
        m, ph, fm = multi_spectrogram_single(audio, fft, hop, win) if right is None else _restated_single(audio, fft, hop, right)
        out.append((m[:, 0], ph, fm[:, 0]))
    return out


def oracle_losses(gt, pred, dtype, w_mel=5.0, w_phase=8.0, right=None):
    """-> dict: mel, mph (python floats), grad = d backwards_total / d pred [B,N], T / P = the features of both sides (detached).
    w_phase == 0 leaves the phase term out of the graph (the mel-only call of the library)."""
    from oracle import losses as ol
    gt = gt.to(dtype)
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    with torch.no_grad():
        T = features(gt, right)
    P = features(p, right)
    mel = ol.mel_loss([t[0] for t in T], [q[0] for q in P])
    mph = ol.multi_phase_loss([q[1] for q in P], [t[1] for t in T])
    tot = w_mel * (mel / (mel.detach() + 1e-9))
    if w_phase:
        tot = tot + w_phase * (mph / (mph.detach() + 1e-9))
    tot.backward()
    return dict(mel=mel.item(), mph=mph.item(), grad=p.grad, T=T, P=[tuple(x.detach() for x in q) for q in P])


def mel_cotangents(T_mags, P_mags, w_mel=5.0):
    """What loss_grad_kernel leaves in d_mag for the mel term, formed in float64 from ANY pair of feature lists ([B,128,frames]
    per resolution): -k_r sign(T - P), k_r = w_mel / (mel + 1e-9) / 3 / (sum |T_r| + 1e-6)"""
    T = [t.detach().double().cpu() for t in T_mags]
    P = [p.detach().double().cpu() for p in P_mags]
    mel = sum((t - p).abs().sum() / (t.abs().sum() + 1e-6) for t, p in zip(T, P)) / 3
    return [-(w_mel / (mel + 1e-9) / 3 / (t.abs().sum() + 1e-6)) * torch.sign(t - p) for t, p in zip(T, P)]


def injected_grad(pred, cots, dtype, right=None):
    """d sum_r <P_r, cot_r> / d pred through the log1p-mel features of pred in `dtype`: the smooth part of the backward chain
    (log1p, filter bank, |X|, STFT, framing) with the signs held fixed"""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    P = features(p, right)
    sum((q[0] * c.to(dtype)).sum() for q, c in zip(P, cots)).backward()
    return p.grad


def edge_errors(got, ref, N):
    """max |got - ref| of the reference's maximum over the first and the last n_fft / 2 samples (the ones the mirrors feed), for
    n_fft = 512, 1024, 2048 -> six numbers"""
    e = (got.detach().double().cpu() - ref.detach().double().cpu()).abs() / ref.abs().max().item()
    return [f(e, h) for h in (256, 512, 1024) for f in (lambda e, h: e[:, :h + 1].max().item(), lambda e, h: e[:, N - 1 - h:].max().item())]


@functools.lru_cache(maxsize=None)
def oracle64(i):
    """the float64 reference of case i, computed once and shared: default weights (`full`), mel term alone (`mel_only`)"""
    B, N = FRONT_END_CASES[i]
    gt, pred = front_end_pair(B, N)
    return dict(gt=gt, pred=pred, full=oracle_losses(gt, pred, torch.float64),
                mel_only=oracle_losses(gt, pred, torch.float64, w_mel=5.0, w_phase=0.0))


def frame_counts(N):
    return [N // hop + 1 for hop in (128, 256, 512)]


@pytest.mark.parametrize("i", range(len(FRONT_END_CASES)), ids=CASE_IDS)
def test_loss_oracle_on_front_end_cases(i):
    """Measured on FRONT_END_CASES (fp32 oracle vs float64 oracle, worst case): log1p-mel features 5.0e-7 and |X| 1.7e-7 of the
    maximum, gated phase 7.1e-4 rad, mel 1.9e-6, multi-phase 1.4e-7 relative, full gradient relative L2 6.7e-4 (1 - cosine
    2.3e-7); mel-only gradient under the float64 oracle's cotangent, of its maximum, per case: 2.4e-7, 5.1e-7, 7.5e-7, 4.0e-7,
    5.8e-7, 1.24e-6, 7.3e-7 (FP32_D_WORST; GATE_D = 20 x that = 2.5e-5).
    One sample of framing error on the right: mel-only gradient 0.062 .. 0.43 of its maximum (2 400 x GATE_D or more), full
    gradient relative L2 0.10 .. 1.3 (5 x its gate or more).
    Smallest non-zero |T - P| of the log1p-mel features per case: 1.3e-4, 1.4e-4, 2.0e-5, 4.3e-5, 6.9e-6, 4.0e-5, 4.3e-5 -- the
    feature gate allows 1e-5 of a maximum of 4.8, i.e. 4.8e-5: a sign there belongs to whoever computes the features."""
    B, N = FRONT_END_CASES[i]
    o = oracle64(i)
    gt, pred, f64, m64 = o["gt"], o["pred"], o["full"], o["mel_only"]
    f32 = oracle_losses(gt, pred, torch.float32)
    assert [t[0].shape[2] for t in f64["T"]] == frame_counts(N)
    assert all(t[0].shape == (B, 128, fr) and t[1].shape == (B, n // 2 + 1, fr)
               for t, fr, n in zip(f64["T"], frame_counts(N), (512, 1024, 2048)))
    # fp32 inside half of every gate
    rows = []
    for side in ("T", "P"):
        for r, n_fft in enumerate((512, 1024, 2048)):
            e_mag, e_fft = rel(f32[side][r][0], f64[side][r][0]), rel(f32[side][r][2], f64[side][r][2])
            e_ph = wrapped_phase_err(f32[side][r][1], f64[side][r][1], f64[side][r][2])
            rows.append(f"    {side} {n_fft:4d}: log1p-mel {e_mag:.2e}  |X| {e_fft:.2e}  gated phase {e_ph:.2e}")
            assert e_mag <= GATE_FEAT / 2 and e_fft <= GATE_FEAT / 2 and e_ph <= GATE_PHASE / 2, rows[-1]
    e_mel, e_mph = abs(f32["mel"] - f64["mel"]) / f64["mel"], abs(f32["mph"] - f64["mph"]) / f64["mph"]
    l2, cos = rel_l2_cos(f32["grad"], f64["grad"])
    cots = mel_cotangents([t[0] for t in f64["T"]], [p[0] for p in f64["P"]])
    d64 = injected_grad(pred, cots, torch.float64)
    d32 = injected_grad(pred, cots, torch.float32)
    e_d = rel(d32, d64)
    print(f"\n  B={B} N={N}: fp32 oracle vs float64 oracle\n" + "\n".join(rows))
    print(f"    mel {e_mel:.2e}  multi-phase {e_mph:.2e}  full gradient rel L2 {l2:.2e} 1-cos {1 - cos:.2e}  "
          f"mel-only gradient (injected cotangent) {e_d:.2e}")
    assert e_mel <= GATE_MEL / 2 and e_mph <= GATE_MPH / 2
    assert l2 <= GATE_L2 / 2 and 1 - cos <= (1 - GATE_COS) / 2
    assert e_d <= FP32_D_WORST and e_d <= GATE_D / 2
    # the injected cotangent IS the mel term's gradient: autograd through |T - P| gives the same thing
    assert rel(d64, m64["grad"]) <= 1e-12
    # sensitivity: `reflect` restated is the oracle; `symmetric` on the right moves the gradients far past their gates
    same = oracle_losses(gt, pred, torch.float64, right="reflect")
    assert rel(same["grad"], f64["grad"]) <= 1e-12 and abs(same["mel"] - f64["mel"]) <= 1e-12 * f64["mel"]
    off = oracle_losses(gt, pred, torch.float64, right="symmetric")
    moved_d = rel(injected_grad(pred, cots, torch.float64, right="symmetric"), d64)
    moved_l2, moved_cos = rel_l2_cos(off["grad"], f64["grad"])
    print(f"    one sample off on the right: mel-only gradient {moved_d:.2e} ({moved_d / GATE_D:.0f} x gate)  "
          f"full gradient rel L2 {moved_l2:.2e} ({moved_l2 / GATE_L2:.1f} x gate) cos {moved_cos:.4f}")
    assert moved_d >= SENS_D * GATE_D
    assert moved_l2 >= SENS_L2 * GATE_L2
    # kink margins
    margin = min(d[d > 0].min().item() for d in ((t[0] - p[0]).abs() for t, p in zip(f64["T"], f64["P"])))
    top = max(t[0].max().item() for t in f64["T"])
    print(f"    smallest non-zero |T - P| of the log1p-mel features {margin:.2e}  (feature gate {GATE_FEAT:.0e} x max {top:.2f})")
    assert 0 < margin < 10 * GATE_FEAT * top


@pytest.mark.parametrize("n_fft,win", [(512, 512), (2048, 1200)])
@pytest.mark.parametrize("N", MEL_FRONT_CASES)
def test_mel_oracle_on_mel_front_cases(N, n_fft, win):
    """calculate_mel + log energy: the fp32 oracle against the float64 oracle, inside half of the gates of test_mel_front_end, and
    the trimmed frame count"""
    from oracle import frontend as ofe
    audio = mel_front_audio(N, n_fft)
    m64 = ofe.calculate_mel(audio.double(), n_fft, win, 300)
    m32 = ofe.calculate_mel(audio, n_fft, win, 300)
    frames = N // 300 + 1
    assert m64.shape == m32.shape == (3, 80, frames - frames % 2)
    e_mel, e_en = rel(m32, m64), rel(ofe.log_energy(m32), ofe.log_energy(m64))
    l1 = (m32.double() - m64).abs().mean().item()
    print(f"\n  N={N} n_fft={n_fft}: fp32 vs float64 oracle: mel {e_mel:.2e} (L1 {l1:.2e})  energy {e_en:.2e}")
    assert e_mel <= GATE_MELFE / 2 and e_en <= GATE_MELFE / 2 and l1 <= GATE_MELFE_L1 / 2
