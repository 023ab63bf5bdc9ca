"""Shared cases of the slm tests (tests/test_slm.py on the CPU, tests/test_slm_gpu.py on the device) and of
tools/gen_slm_golden.py: the two WavLM configurations, the case lists, the key-named weight fill, the seeded waves, and a torch
restatement -- float64 by default -- of the one part of the path that has no importable reference here:

  resample_kernel / resample   torchaudio.transforms.Resample(orig, new) with its defaults: sinc_interp_hann,
                               lowpass_filter_width 6, rolloff 0.99 (24000 -> 16000: two phases of 23 taps at stride 3)

torchaudio is not installed: restated from the package's documented closed form (PARITY UNPINNED at that boundary).  The network
IS pinned: tests/golden/slm_small.* hold runs of transformers' own WavLMModel on the CPU.
"""
import math

import torch

# hidden 64, 2 layers, 4 heads x 16, FFN 128, conv dims 32 x 7, pos conv k = 16 in 4 groups, 32 buckets, max distance 64
SMALL = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, conv_dim=(32,) * 7,
             num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, num_buckets=32, max_bucket_distance=64)
FULL2 = dict(num_hidden_layers=2)   # full width (the class defaults), two layers
FULL12 = dict()                     # the class defaults: what microsoft/wavlm-base-plus is
CONFIGS = dict(small=SMALL, full2=FULL2, full12=FULL12)
SEED = 23
# name -> (config, N16, B, T, hidden states stored)
CASES = {
    "small_400": ("small", 400, 2, 1, (0, 1, 2)),        # the shortest legal wave; 399 is refused
    "small_5200": ("small", 5200, 2, 16, (0, 1, 2)),
    "small_7777": ("small", 7777, 2, 24, (0, 1, 2)),     # a remainder dropped at several strides
    "small_22800": ("small", 22800, 2, 71, (0, 1, 2)),   # distances beyond max_bucket_distance: the bucket function's clamp
    "small_104000": ("small", 104000, 1, 324, (0, 1, 2)),  # GroupNorm rows of 20 799 frames: the long reduction at its real length
    "full2_8000": ("full2", 8000, 2, 24, (0, 1, 2)),
    "full12_26000": ("full12", 26000, 1, 81, (0, 6, 12)),
}
BUCKET_TABLES = ((71, 32, 64), (1024, 320, 800))  # (T, num_buckets, max_distance); the second crosses 800
RESAMPLE_N = (7800, 11666, 34200)


def wavlm_weights(cfg, seed=SEED):
    """WavLMModel-layout state_dict (without masked_spec_embed) of the key-named fill: weights are never committed, both sides
    regenerate them"""
    from stylish_tts_amd.manifest import wavlm_manifest
    from stylish_tts_amd.synthetic_weights import fill_state_dict
    return fill_state_dict(wavlm_manifest(**cfg), seed)


def wave(n, B, which=0, seed=SEED):
    """[B, n] at the slm rate: a few sines under noise, amplitude about 0.3; which = 0 the "ground truth", 1 the "prediction"
    (the same wave plus 10 % of another draw)"""
    g = torch.Generator().manual_seed(100003 * seed + n)
    t = torch.arange(n, dtype=torch.float64)[None, :] / 16000.0
    f = 80.0 + 400.0 * torch.rand(B, 3, generator=g, dtype=torch.float64)
    x = sum(torch.sin(2 * math.pi * f[:, i:i + 1] * t) / (i + 1) for i in range(3)) * 0.15
    x = x + 0.05 * torch.randn(B, n, generator=g, dtype=torch.float64)
    if which:
        x = x + 0.03 * torch.randn(B, n, generator=g, dtype=torch.float64)
    return x.float()


def frames(n16, cfg):
    """frames of n16 samples: floor((n - k) / s) + 1 per feature conv; 0 when a layer is left without one"""
    from stylish_tts_amd.manifest import WAVLM_DEFAULT_CFG
    n = int(n16)
    for k, s in zip(cfg.get("conv_kernel", WAVLM_DEFAULT_CFG["conv_kernel"]), cfg.get("conv_stride", WAVLM_DEFAULT_CFG["conv_stride"])):
        if n < k:
            return 0
        n = (n - k) // s + 1
    return n


def forward_gate(ref64_max, own):
    """the gate this project uses for a third-party network (profiles/pitch_parity_table.txt): max(1e-5 max|ref64|,
    4 x max|ref32 - ref64|), both numbers taken from the reference alone"""
    return max(1e-5 * ref64_max, 4 * own)


# ---- resampler ----------------------------------------------------------------------------------------------------------------
def resample_dims(orig, new, lpw=6, rolloff=0.99):
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    base = min(orig, new) * rolloff
    return orig, new, base, math.ceil(lpw * orig / base)


def resample_kernel(orig=24000, new=16000, dtype=torch.float64, lpw=6, rolloff=0.99):
    """[new', 2 width + orig']: phase p, tap j in [-width, width + orig'): t = clamp((-p / new' + j / orig') * base, +-lpw),
    sinc(pi t) cos^2(pi t / lpw / 2) * base / orig', evaluated in float64 and rounded once"""
    o, n, base, width = resample_dims(orig, new, lpw, rolloff)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, :] / o
    t = (-torch.arange(n, dtype=torch.float64)[:, None] / n + idx) * base
    t = t.clamp(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2.0) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t)
    return (k * window * (base / o)).to(dtype)


def resample(audio, orig=24000, new=16000, dtype=torch.float64):
    """audio [B, N] at `orig` -> [B, ceil(N new / orig)] at `new`"""
    B, N = audio.shape
    o, n, _, width = resample_dims(orig, new)
    k = resample_kernel(orig, new, torch.float32).to(dtype)  # the table the transform holds is fp32
    x = torch.nn.functional.pad(audio.to(dtype), (width, width + o))
    y = torch.nn.functional.conv1d(x[:, None], k[:, None], stride=o)
    return y.transpose(1, 2).reshape(B, -1)[:, :(N * n + o - 1) // o]


def resample_input(N, B=2, seed=SEED):
    """[B, N] at 24 kHz"""
    g = torch.Generator().manual_seed(7919 * seed + N)
    t = torch.arange(N, dtype=torch.float64)[None, :] / 24000.0
    f = 100.0 + 5000.0 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    return (0.3 * torch.sin(2 * math.pi * f * t) + 0.1 * torch.randn(B, N, generator=g, dtype=torch.float64)).float()
