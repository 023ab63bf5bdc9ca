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


# Signal lengths for the audio-side front end (csrc/frontend.hip), (B, N).  The loss features are three STFTs, (n_fft, hop) =
# (512, 128), (1024, 256), (2048, 512), N // hop + 1 frames each.  The edges, as the kernels stand:
#   * N > 1024 is required (reflection of the 2048-point transform), so 1025 is the smallest length;
#   * stft_fft_kernel / stft_fft_adj_kernel own TF = 16 frames per workgroup at 512 and 1024 points, 8 at 2048 (fft_tf);
#     fft_grid rounds the ntx * B tiles up to a multiple of eight workgroups and the rest return early (fft_tile);
#   * a tile is read with 16-byte loads when N % 4 == 0, it is full, f0 * hop >= n_fft / 2 and
#     (f0 + TF - 1) * hop + n_fft / 2 <= N: the first candidate is the second tile, which needs N >= 4224 / 8448 / 8704;
#   * span_gather_kernel adds a sample's own position, its left mirror (1 <= i <= n_fft / 2) and its right mirror
#     (N - 1 - n_fft / 2 <= i <= N - 2): a sample has both when N <= n_fft + 1, and up to two tiles cover a position;
#   * loss_sums_kernel / loss_grad_kernel take the time difference inside [F][B][frames]: t + 1 < frames and t > 0 alone
#     keep it inside an utterance.
FRONT_END_CASES = [
    (1, 1025),  # 9 / 5 / 3 frames.  Smallest accepted length: at 2048 points every frame reflects at both ends and samples
                # 1 .. 1023 have both mirrors; one tile per resolution, ntx * B = 1 (seven workgroups return early)
    (3, 1201),  # 10 / 5 / 3.  Odd N; B = 3: two utterance borders inside every row of the [F][B][frames] tensors
    (4, 4095),  # 32 / 16 / 8.  Every resolution an exact multiple of its tile; ntx * B = 8 / 4 / 4; odd N
    (3, 4096),  # 33 / 17 / 9.  One frame into the next tile everywhere; ntx * B = 9 / 6 / 6 tiles on grids of 18 / 8 / 8 workgroups (the
                # rest return early); N % 4 == 0, yet no tile is interior (4096 < 4224)
    (2, 8700),  # 68 / 34 / 17.  N % 4 == 0; tiles 1-3 (512 points; tile 4 is partial) and tile 1 (1024 points: 8448 <= N) take
                # the 16-byte path; the second 2048-point tile is four samples short (8704 > N)
    (2, 8704),  # 69 / 35 / 18.  The interior condition of the second 2048-point tile holds with equality
    (3, 8707),  # 69 / 35 / 18.  As 8704, but N % 4 != 0: everything on the scalar path; ntx * B = 15 / 9 / 9
]

# Signal lengths for the mel front end (sty_mel_fwd) at hop 300, B = 3, on (n_fft, win) = (512, 512) and (2048, 1200).
# launch_mel keeps N // 300 + 1 frames less one when that is odd; the tiles are 16 frames (512 points) and 8 (2048), and the
# 16-byte path needs N % 4 == 0 (hop % 4 == 0 holds) and, for the second tile, N >= 31 * 300 + 256 = 9556 (512 points) or
# N >= 15 * 300 + 1024 = 5524 (2048 points).
MEL_FRONT_CASES = [
    1025,  # 4 frames: smallest accepted length for 2048 points (every frame reflects at both ends there)
    1200,  # 5 -> 4: trim; reflection on both ends
    4799,  # 16: odd N; one full 16-frame tile, two full 8-frame tiles
    4800,  # 17 -> 16: the trimmed frame is the one that would open a second 16-frame (third 8-frame) tile
    5524,  # 19 -> 18: the interior condition of the second 8-frame tile (2048 points) holds with equality; trim
    9556,  # 32: the interior condition of the second 16-frame tile (512 points) holds with equality; at 2048 points the
           # second and third tiles are interior and the fourth is not
    9600,  # 33 -> 32: trim, one frame past a full tile at both tile sizes
]


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
