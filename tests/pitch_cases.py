"""Shared cases of the pitch tests (tests/test_pitch.py on the CPU, tests/test_pitch_gpu.py on the device) and of
tools/gen_pitch_golden.py: the key-named weight fill, the network inputs, and torch restatements -- float64 by default -- of
the parts of the RMVPE path that have no importable reference here:

  resample_kernel / resample   torchaudio Resample(24000, 16000, lowpass_filter_width=128), sinc_interp_hann, rolloff 0.99
  mel_basis                    librosa.filters.mel(sr=16000, n_fft=1024, n_mels=128, fmin=30, fmax=8000, htk=True) (Slaney norm)
  stft_mag / logmel            MelSpectrogram(128, 16000, 1024, 200, None, 30, 8000) of train/dataprep/rmvpe/spec.py
  decode                       to_local_average_f0 (train/dataprep/rmvpe/utils.py:114-131) with an exact cents mapping

torchaudio and librosa are not installed: the first three are restated from the packages' documented closed forms (PARITY
UNPINNED at that boundary).  The decode IS pinned: the fixture holds the reference function's own outputs.
"""
import math

import torch

SMALL = dict(n_blocks=2, inter_layers=2, en_out_channels=4)   # 2.8 M parameters
FULL = dict(n_blocks=4, inter_layers=4, en_out_channels=16)   # RMVPE's E2E0(4, 1, (2, 2)): 90 M parameters
SEED = 11
NET_FRAMES = (17, 32, 33, 61, 64)  # reflection pad 15 / 0 / 31 / 3 / 0
N_MELS, N_CLASS, CONST = 128, 360, 1997.3794084376191
WIDTH, TAPS = 194, 391  # ceil(128 * 3 / 1.98), 2 * WIDTH + 3


def rmvpe_weights(cfg, seed=SEED):
    """reference-layout state_dict of the key-named fill (weights are never committed: both sides regenerate them)"""
    from stylish_tts_amd.manifest import rmvpe_manifest
    from stylish_tts_amd.synthetic_weights import fill_state_dict
    return fill_state_dict(rmvpe_manifest(**cfg), seed)


def net_input(n, B=2, seed=SEED):
    """log-mel-like input [B, 128, n]: 2 * randn - 5"""
    g = torch.Generator().manual_seed(1000 * seed + n)
    return 2.0 * torch.randn(B, N_MELS, n, generator=g) - 5.0


def forward_gate(ref64, ref32):
    """tests/test_align_gpu.py::forward_gate: max(1e-5 max|ref64|, 4 x max|ref32 - ref64|) and its three numbers"""
    scale = ref64.abs().max().item()
    own = (ref32.double() - ref64.double()).abs().max().item()
    return max(1e-5 * scale, 4 * own), scale, own


# ---- front end ------------------------------------------------------------------------------------------------------------
def resample_kernel(dtype=torch.float64):
    """[2, 391]: phase p, tap j in [-194, 197): t = clamp((-p / 2 + j / 3) * 1.98, +-128), sinc(pi t) cos^2(pi t / 256) * 1.98 / 3,
    evaluated in float64 and rounded once"""
    base, lpw = 2 * 0.99, 128.0
    idx = torch.arange(-WIDTH, WIDTH + 3, dtype=torch.float64)[None, :] / 3.0
    t = (-torch.arange(2, dtype=torch.float64)[:, None] / 2.0 + idx) * base
    t = t.clamp(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2.0) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t)
    return (k * window * (base / 3.0)).to(dtype)


def resample(audio, dtype=torch.float64):
    """audio [B, N] at 24 kHz -> [B, ceil(2 N / 3)] at 16 kHz"""
    B, N = audio.shape
    k = resample_kernel(torch.float32).to(dtype)  # the table the transform holds is fp32
    x = torch.nn.functional.pad(audio.to(dtype), (WIDTH, WIDTH + 3))
    y = torch.nn.functional.conv1d(x[:, None], k[:, None], stride=3)  # [B, 2, N / 3 + 1]
    return y.transpose(1, 2).reshape(B, -1)[:, :(2 * N + 2) // 3]


def mel_basis(dtype=torch.float64):
    """[128, 513]"""
    hz2mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    lo, hi = hz2mel(30.0), hz2mel(8000.0)
    mels = lo + (hi - lo) * torch.arange(N_MELS + 2, dtype=torch.float64) / (N_MELS + 1)
    f = 700.0 * (10.0 ** (mels / 2595.0) - 1.0)
    fft = 8000.0 * torch.arange(513, dtype=torch.float64) / 512.0
    lower = (fft[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    upper = (f[2:, None] - fft[None, :]) / (f[2:] - f[1:-1])[:, None]
    w = torch.minimum(lower, upper).clamp(min=0.0)
    return (w * (2.0 / (f[2:] - f[:-2]))[:, None]).to(dtype)


def stft_mag(x, dtype=torch.float64):
    """x [B, M] at 16 kHz -> |STFT| [B, 513, M // 200 + 1]: periodic hann of 1024, centre / reflect, hop 200"""
    x = torch.nn.functional.pad(x.to(dtype)[:, None], (512, 512), mode="reflect")[:, 0]
    frames = x.unfold(1, 1024, 200)  # [B, n, 1024]
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64).to(dtype)
    spec = torch.fft.rfft(frames * win, dim=2)
    return torch.sqrt(spec.real ** 2 + spec.imag ** 2).transpose(1, 2)


def mel_linear(audio, dtype=torch.float64):
    """audio [B, N] at 24 kHz -> the mel spectrum before the log, [B, 128, n]"""
    basis = mel_basis(torch.float32).to(dtype)  # registered as an fp32 buffer (spec.py:30-31)
    return torch.matmul(basis, stft_mag(resample(audio, dtype), dtype))


def logmel(audio, dtype=torch.float64):
    return torch.log(torch.clamp(mel_linear(audio, dtype), min=1e-5))


def harmonic_audio(N, B=2, seed=3, lead=2400):
    """what audio_list hands out: `lead` zeros, a harmonic signal quantised to PCM16, zeros to the end"""
    g = torch.Generator().manual_seed(seed + N)
    t = torch.arange(N, dtype=torch.float64) / 24000.0
    out = torch.zeros(B, N, dtype=torch.float64)
    for b in range(B):
        f0 = 110.0 * (1 + b) + 40.0 * torch.sin(2 * math.pi * 1.5 * t)
        ph = 2 * math.pi * torch.cumsum(f0, 0) / 24000.0
        w = sum(torch.sin((h + 1) * ph) / (h + 1) for h in range(8)) * 0.15
        w = w + 0.01 * torch.randn(N, generator=g, dtype=torch.float64)
        w = torch.clamp(torch.round(w * 32767.0), -32768, 32767) / 32768.0
        end = N - lead // 2 - 300 * b
        out[b, lead:end] = w[lead:end]
    return out.float()


# ---- decode ---------------------------------------------------------------------------------------------------------------
def decode(hidden, thred=0.03):
    """hidden [..., 360] -> f0 [...] in float64: arg-max (lowest index on a tie), the window [c - 4, c + 5) clipped to [0, 360),
    cents = sum s (20 i + CONST) / sum s, f0 = 10 * 2^(cents / 1200), 0 where the row's maximum is < thred"""
    h = hidden.double()
    idx = torch.arange(N_CLASS)
    cents_map = 20.0 * idx.double() + CONST
    center = torch.argmax(h, dim=-1, keepdim=True)  # the first maximal index
    mask = (idx >= (center - 4).clamp(min=0)) & (idx < (center + 5).clamp(max=N_CLASS))
    w = h * mask
    ws = w.sum(-1)
    cents = (w * cents_map).sum(-1) / (ws + (ws == 0))
    f0 = 10.0 * 2.0 ** (cents / 1200.0)
    return f0 * ~(hidden.max(dim=-1)[0] < thred)  # (compared in hidden's own dtype, as the reference compares)


def bump(k, values=(0.25, 0.5, 1.0, 0.5, 0.25), floor=0.0):
    """a row with a symmetric bump centred on bin k (clipped at the ends)"""
    row = torch.full((N_CLASS,), floor)
    half = len(values) // 2
    for j, v in enumerate(values):
        i = k - half + j
        if 0 <= i < N_CLASS:
            row[i] = v
    return row


def decode_cases():
    """name -> row [360] fp32.  Symmetric bumps (one-hot and five wide), peaks at bins 0-3 and 356-359 (clipped window, on a
    floor so that the window's other bins count), an exact tie, a row of all values < 0.03, noise"""
    g = torch.Generator().manual_seed(SEED)
    cases = {}
    for k in (4, 100, 355):
        cases[f"onehot_{k}"] = bump(k, (1.0,))
        cases[f"bump_{k}"] = bump(k)
    for k in (0, 1, 2, 3, 356, 357, 358, 359):
        cases[f"edge_{k}"] = bump(k, (0.2, 0.6, 0.9, 0.6, 0.2), floor=0.05)
    tie = torch.full((N_CLASS,), 0.01)
    tie[120] = tie[200] = 0.7
    tie[121], tie[199] = 0.3, 0.4
    cases["tie"] = tie
    cases["quiet"] = 0.0299 * torch.rand(N_CLASS, generator=g)
    cases["at_threshold"] = bump(50, (0.01, 0.03, 0.01))
    cases["noise"] = torch.rand(N_CLASS, generator=g)
    return cases
