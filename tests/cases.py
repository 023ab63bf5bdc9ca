"""Seeded synthetic inputs shared by tools/gen_golden.py (reference side) and the tests (oracle / HIP side)."""
import torch


def _pitch(g, B, T):
    pitch = torch.rand(B, T, generator=g) * 200 + 80          # 80..280 Hz
    seg = torch.rand(B, (T + 9) // 10, generator=g) < 0.3       # ~30 % unvoiced, in 10-frame runs
    unv = seg.repeat_interleave(10, dim=1)[:, :T]
    pitch[unv] = 0
    return pitch


# Ragged text batches (L, lengths).  The edges are those of attn_kernel (32 queries per wave, 128 per workgroup, key tiles of
# 32): 32 / 64 / 96 / 128 each have a length on, below and above them, and two cases hold a row of length 1.  The other
# kernels on the masked path tile the text axis by multiples of 32 as well -- conv1d_mfma_kernel 64 / 128 / 256 / 512
# (TT_BLK = 32 * NT * WN of the configurations launch_tiled picks), convk1 128 samples per LDS row, the
# weight-gradient kernels 128 (WG_TW) and 64 (W1_TW) samples per chunk, attn_bwd 32-key tiles and 128-query workgroups --
# so at L <= 130 every edge that applies is 64 or 128, both straddled here (63 / 64 / 65, 127 / 128 / 129, and L = 130
# itself puts two columns into a second 128-wide tile); no further length is needed.
RAGGED_CASES = [(100, [100, 65, 64, 63, 33, 17, 16, 1]), (37, [37, 36, 2]), (130, [130, 129, 128, 127, 5]),
                (64, [64, 1, 32, 31]), (100, [100, 97, 96, 95, 32])]
RAGGED_PAD_IDS = (170, 178)  # ids that no valid position uses: variant B writes them onto the padded positions


def make_ragged(L, lengths, T=None, seed=21):
    """A ragged text batch: valid tokens randint(1, 170); texts_a has id 0 on the padded positions, texts_b ids drawn from
    RAGGED_PAD_IDS.  With T: integer durations, 1 on every valid token plus a multinomial split of the remaining T - len
    frames, 0 on padding, so every row sums to T (the recipe of bench.make_inputs, per row length), and the frame-rate
    inputs of the speech predictor (pitch, energy, style, noise) as make_case("sp_small") draws them."""
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    text_lengths = torch.tensor(lengths, dtype=torch.int64)
    assert int(text_lengths.max()) == L and int(text_lengths.min()) >= 1
    valid = torch.arange(L)[None, :] < text_lengths[:, None]
    tok = torch.randint(1, RAGGED_PAD_IDS[0], (B, L), generator=g)
    pad = torch.randint(RAGGED_PAD_IDS[0], RAGGED_PAD_IDS[1], (B, L), generator=g)
    d = dict(texts_a=tok * valid, texts_b=torch.where(valid, tok, pad), text_lengths=text_lengths, valid=valid,
             style=torch.randn(B, 64, generator=g))
    if T is not None:
        dur = torch.zeros(B, L)
        for b, n in enumerate(lengths):
            assert T >= n
            dur[b, :n] = 1
            if T > n:
                idx = torch.multinomial(torch.ones(n), T - n, replacement=True, generator=g)
                dur[b, :n] += torch.bincount(idx, minlength=n).float()
        noise_seed = 123
        gn = torch.Generator().manual_seed(noise_seed)
        _ = torch.rand(B, 9, generator=gn)
        d.update(durations=dur, pitch=_pitch(g, B, T), energy=torch.randn(B, T, generator=g),
                 noise=torch.randn(B, 300 * T, 9, generator=gn), noise_seed=noise_seed)
    return d


def make_case(name):
    g = torch.Generator().manual_seed({"sp_small": 11, "se_small": 12, "blocks": 13}[name])
    if name == "sp_small":
        B, T, L = 2, 80, 40
        texts = torch.randint(1, 178, (B, L), generator=g)
        lengths = torch.tensor([40, 35])
        dur = torch.ones(B, L) * 2
        dur[1, 35:] = 0
        dur[1, :10] += 1                                          # both rows sum to T = 80
        texts[1, 35:] = 0
        noise_seed = 123
        gn = torch.Generator().manual_seed(noise_seed)
        # same stream the reference consumes under torch.manual_seed(noise_seed): rand[B,9] then randn[B,300T,9]
        _ = torch.rand(B, 9, generator=gn)
        noise = torch.randn(B, 300 * T, 9, generator=gn)
        return dict(texts=texts, text_lengths=lengths, durations=dur, pitch=_pitch(g, B, T),
                    energy=torch.randn(B, T, generator=g), style=torch.randn(B, 64, generator=g),
                    noise=noise, noise_seed=noise_seed)
    if name == "se_small":
        return dict(mel=torch.randn(2, 1, 80, 80, generator=g))
    if name == "blocks":
        return dict(x32=torch.randn(2, 32, 600, generator=g), x195=torch.randn(2, 195, 80, generator=g),
                    style=torch.randn(2, 64, generator=g), wave=torch.randn(2, 2400, generator=g) * 0.3)
    raise KeyError(name)
