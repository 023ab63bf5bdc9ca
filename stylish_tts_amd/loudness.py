"""ITU-R BS.1770-4 integrated loudness and gain normalisation, on the host (numpy + scipy.signal.lfilter): what
`pyloudnorm.Meter(rate).integrated_loudness` / `pyloudnorm.normalize.loudness` do for the reference's `speak`
(tts/cli.py:60, 86-87) with the meter's defaults.  The audio is on the host to be written to a file anyway.

  K-weighting, two biquads DESIGNED AT THE SAMPLE RATE (audio-EQ-cookbook forms, not the standard's 48 kHz table):
      high shelf  +4 dB, Q 1/sqrt(2), 1500 Hz;   high pass  Q 0.5, 38 Hz
  0.4 s blocks with 75 % overlap, mean square per block; block loudness -0.691 + 10 log10(sum over channels of G z)
  absolute gate -70 LUFS, relative gate 10 LU under the loudness of the blocks that pass the absolute gate
  integrated loudness = -0.691 + 10 log10(mean z of the blocks above both gates)

pyloudnorm itself is not a dependency of this path, so parity with it is UNPINNED; what is pinned is the
standard's own reference point: a full-scale 997 Hz sine reads -3.01 LKFS within the ITU compliance tolerance of 0.1 LU.
"""
import math

import numpy as np

BLOCK_SECONDS, OVERLAP = 0.4, 0.75
ABSOLUTE_GATE, RELATIVE_GATE = -70.0, -10.0
CHANNEL_GAIN = (1.0, 1.0, 1.0, 1.41, 1.41)  # L, R, C, Ls, Rs


def k_weighting(rate):
    """[(b, a)] of the two stages, a[0] = 1"""
    def common(fc, q):
        w0 = 2.0 * math.pi * fc / rate
        return math.cos(w0), math.sin(w0) / (2.0 * q)

    cw, alpha = common(1500.0, 1.0 / math.sqrt(2.0))
    A = 10.0 ** (4.0 / 40.0)
    sq = 2.0 * math.sqrt(A) * alpha
    b = np.array([A * ((A + 1) + (A - 1) * cw + sq), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - sq)])
    a = np.array([(A + 1) - (A - 1) * cw + sq, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - sq])
    shelf = (b / a[0], a / a[0])
    cw, alpha = common(38.0, 0.5)
    b = np.array([(1 + cw) / 2, -(1 + cw), (1 + cw) / 2])
    a = np.array([1 + alpha, -2 * cw, 1 - alpha])
    return [shelf, (b / a[0], a / a[0])]


def block_samples(rate):
    return int(BLOCK_SECONDS * rate)


def integrated_loudness(audio, rate):
    """audio [samples] or [samples, channels] (at most 5), float -> LUFS (-inf when every block is under the absolute gate).
    Raises ValueError when the audio is shorter than one 0.4 s block."""
    from scipy.signal import lfilter
    x = np.asarray(audio, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, ch = x.shape
    if ch > 5:
        raise ValueError("integrated_loudness: at most five channels")
    if n < BLOCK_SECONDS * rate:
        raise ValueError(f"integrated_loudness: audio must be at least {BLOCK_SECONDS} s long")
    for b, a in k_weighting(rate):
        x = lfilter(b, a, x, axis=0)
    seconds = n / rate
    step = 1.0 - OVERLAP
    blocks = int(np.round((seconds - BLOCK_SECONDS) / (BLOCK_SECONDS * step)) + 1)
    z = np.zeros((ch, blocks))
    for j in range(blocks):
        lo = int(BLOCK_SECONDS * (j * step) * rate)
        hi = int(BLOCK_SECONDS * (j * step + 1) * rate)
        z[:, j] = np.sum(np.square(x[lo:hi]), axis=0) / (BLOCK_SECONDS * rate)
    G = np.array(CHANNEL_GAIN[:ch])[:, None]
    with np.errstate(divide="ignore"):
        loud = -0.691 + 10.0 * np.log10(np.sum(G * z, axis=0))
        keep = loud >= ABSOLUTE_GATE
        if not keep.any():
            return -math.inf
        relative = -0.691 + 10.0 * np.log10(np.sum(G[:, 0] * z[:, keep].mean(axis=1))) + RELATIVE_GATE
        keep = (loud > relative) & (loud > ABSOLUTE_GATE)
        if not keep.any():
            return -math.inf
        return float(-0.691 + 10.0 * np.log10(np.sum(G[:, 0] * z[:, keep].mean(axis=1))))


def normalize(audio, target_lufs, rate=24000, log=None):
    """Gain the audio to target_lufs (pyloudnorm.normalize.loudness(data, measured, target): one gain, no limiter).  Audio
    shorter than one block, or under the absolute gate throughout, cannot be measured: it is returned unchanged, with a
    logged warning."""
    x = np.asarray(audio)
    if x.shape[0] < BLOCK_SECONDS * rate:
        if log:
            log(f"warning: {x.shape[0] / rate:.3f} s of audio is shorter than one {BLOCK_SECONDS} s loudness block: not normalised")
        return audio
    measured = integrated_loudness(x, rate)
    if not math.isfinite(measured):
        if log:
            log("warning: audio is under the -70 LUFS gate throughout: not normalised")
        return audio
    gain = 10.0 ** ((target_lufs - measured) / 20.0)
    return (x * gain).astype(x.dtype) if np.issubdtype(x.dtype, np.floating) else x * gain
