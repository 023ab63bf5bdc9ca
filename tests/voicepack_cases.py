"""Seeded inputs and plain CPU restatements shared by tools/gen_golden_voicepack.py (reference side) and the voicepack tests
(host / HIP side).  Nothing here touches the GPU or the reference tree."""
import math

import numpy as np
import torch

ROWS, DIM = 512, 192

# name -> (seed, what the histogram of text lengths is for)
HISTOGRAMS = {
    "wrap": 31,    # ~600 lengths in 16..200: `lower` goes negative for the short rows and wraps to the longest texts
    "inside": 32,  # 100 rows in the first and in the last bucket + 150 scattered: every window resolves inside [0, 512)
}
# windows that run off the table (the reference's hard-coded 100): bucket -> rows
EXIT_CASES = {
    "99_in_one_bucket": {50: 99},
    "100_in_one_bucket": {50: 100},
    "100_split_over_both_ends": {0: 50, 511: 50},
    "100_in_the_last_bucket": {511: 100},
    "99_spread": {b: 1 for b in range(100, 199)},
    "100_spread": {b: 1 for b in range(100, 200)},
}


def make_rows(name):
    """(rows [N, 192] fp32, text_lengths [N] int64): style-like rows (a common offset, a trend in the length, noise)"""
    g = torch.Generator().manual_seed(HISTOGRAMS[name])
    if name == "wrap":
        lengths = torch.randint(16, 201, (600,), generator=g)
    else:
        scattered = torch.tensor([7, 40, 41, 97, 130, 200, 256, 257, 300, 384, 450, 505])
        lengths = torch.cat([torch.full((100,), 1), torch.full((100,), ROWS),
                             scattered[torch.randint(0, len(scattered), (150,), generator=g)]])
        lengths = lengths[torch.randperm(len(lengths), generator=g)]
    n = len(lengths)
    rows = 0.5 + 0.3 * torch.randn(n, DIM, generator=g) + (lengths.float() / ROWS)[:, None] * torch.randn(1, DIM, generator=g)
    return rows.float().contiguous(), lengths.to(torch.int64)


def counts_of(lengths, rows=ROWS):
    return torch.bincount(torch.as_tensor(lengths, dtype=torch.int64) - 1, minlength=rows).tolist()


def exit_case_lengths(name):
    return [b + 1 for b, c in EXIT_CASES[name].items() for _ in range(c)]


def window_content(counts, lo, hi):
    """(first non-empty bucket, last non-empty bucket, rows held) of [lo, hi): what identifies a window's content"""
    held = [b for b in range(lo, hi) if counts[b]]
    return [held[0], held[-1], sum(counts[b] for b in held)] if held else [-1, -1, 0]


def float64_means(rows, lengths, contents):
    """[len(contents), D] float64: the mean of the rows whose bucket lies in [first, last], per entry of `contents`"""
    bucket = torch.as_tensor(lengths, dtype=torch.int64) - 1
    r64 = rows.double()
    out = torch.empty(len(contents), rows.shape[1], dtype=torch.float64)
    cache = {}
    for i, (first, last, _) in enumerate(contents):
        if (first, last) not in cache:
            sel = (bucket >= first) & (bucket <= last)
            cache[(first, last)] = r64[sel].sum(0) / int(sel.sum())
        out[i] = cache[(first, last)]
    return out


def ulp32(x):
    """the fp32 unit in the last place at |x| (float64 tensor in, float64 out; the smallest normal's for tiny values)"""
    x = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 23)


# ---- a plain BS.1770-4 meter, written for the tests as the standard words it (block loop, no vectorisation) --------------
def k_filter_plain(x, rate):
    """two direct-form-I biquads designed at `rate`: high shelf (+4 dB, Q 1/sqrt 2, 1500 Hz), high pass (Q 0.5, 38 Hz)"""
    def run(b, a, x):
        y = np.zeros_like(x)
        x1 = x2 = y1 = y2 = 0.0
        for n in range(len(x)):
            y[n] = (b[0] * x[n] + b[1] * x1 + b[2] * x2 - a[1] * y1 - a[2] * y2) / a[0]
            x2, x1, y2, y1 = x1, x[n], y1, y[n]
        return y
    A = 10 ** (4.0 / 40)
    w = 2 * math.pi * 1500.0 / rate
    al = math.sin(w) / (2 * (1 / math.sqrt(2)))
    c, s = math.cos(w), 2 * math.sqrt(A) * al
    x = run([A * ((A + 1) + (A - 1) * c + s), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - s)],
            [(A + 1) - (A - 1) * c + s, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - s], x)
    w = 2 * math.pi * 38.0 / rate
    al = math.sin(w) / (2 * 0.5)
    c = math.cos(w)
    return run([(1 + c) / 2, -(1 + c), (1 + c) / 2], [1 + al, -2 * c, 1 - al], x)


def loudness_plain(x, rate):
    y = k_filter_plain(np.asarray(x, dtype=np.float64), rate)
    blk, hop = int(0.4 * rate), int(0.1 * rate)
    z = [float(np.mean(y[s:s + blk] ** 2)) for s in range(0, len(y) - blk + 1, hop)]
    ld = [-0.691 + 10 * math.log10(v) if v > 0 else -math.inf for v in z]
    z1 = [v for v, l in zip(z, ld) if l >= -70.0]
    rel = -0.691 + 10 * math.log10(sum(z1) / len(z1)) - 10.0
    z2 = [v for v, l in zip(z, ld) if l > rel and l > -70.0]
    return -0.691 + 10 * math.log10(sum(z2) / len(z2))
