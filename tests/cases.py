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


# ---------------------------------------------------------------------------------------------------------------------
# Discriminator shapes (csrc/disc.hip, csrc/cfdisc.hip, csrc/disc_common.h), derived from the kernels as they stand.  Every case
# keeps >= 16 elements in its smallest score map (the selected set of the relativistic term stays non-empty); the smallest map's
# element count B * H * Wl[3] (spectrogram), B * t * 16 (waveform), B * T (sequences) is the number in brackets.
#
# Spectrogram discriminator, (B, H, W).  SdRun::geometry: widths Wl = W, ceil(W/2), ceil(./2), ceil(./2), same; row pitches
# Wp[3] = align4(Wl[3] + 4), Wp[0] = 8 Wp[3], halved per level.  sd_l0_kernel and sd_score4_kernel<4> own 4 columns per thread and
# 1024 per workgroup in x; sd_score4_kernel<4> owns RH = 4 rows per thread (grid.y = ceil(H / 4)); its loads row[-1] (w0 > 0) and
# row[4] stay inside the row because Wp[i] >= Wl[i] + 4 at every level.  In fp32 mode every conv, input-gradient conv included, is
# conv1d_mfma_kernel in flat-image mode (the bf16-only families refuse it): <1,4,1,2> for the 32-wide outputs, <2,2,1,1> for the
# 64-wide input gradients of levels 1-3 (profiles/disc_edges_table.txt lists the family per conv).
DISC_SPEC_CASES = [
    (2, 2, 32),    # [16] Wl 32/16/8/4, pitches 64/32/16/8: the largest width on Wp[0] = 64; level 3 has exactly the 4 zero columns of
                   # the 3x9 window's reach (Wl[3] % 4 == 0); even at every halving; H < RH: one row group, rows 2, 3 of it empty, and
                   # no row has both neighbours
    (1, 4, 25),    # [16] Wl 25/13/7/4: the smallest width with Wl[3] = 4 (again 4 zero columns), odd at the first three halvings;
                   # H = RH: one exactly full row group
    (3, 7, 33),    # [105] Wl 33/17/9/5, pitches 96/48/24/12: the first Wp[3] = 12 (three float4 groups per row at level 3, pitches no
                   # power of two); H = 7: the second row group holds 3 rows; two batch borders
    (4, 1, 40),    # [20] H = 1: every kh != 1 tap and every +-Wp shift of the flat-image convs leaves the slab; Wl 40/20/10/5
    (2, 6, 9),     # [24] Wl 9/5/3/2, pitches 64/32/16/8: a single tile at every level, 6 pad columns at level 3; H = 6: second row
                   # group with 2 rows
    (1, 3, 1024),  # [384] Wp[0] = 1056: the second sd_l0 workgroup (blockIdx.x = 1) writes pad columns only; the level-0 sd_score4
                   # workgroup is exactly full (256 threads x 4 columns) and there is no second one
    (2, 3, 1025),  # [774] Wl 1025/513/257/129, Wp[0] = 1088: one valid column in the second workgroup of sd_l0 and of the level-0
                   # sd_score4 (one live thread with one valid column)
]
# compute_bf16 mode, same gates as test_spec_discriminator_bf16_mode.  (3, 7, 33) and (2, 3, 1025) stay below convp16_kernel's
# threshold (48 tiles of 128 flat positions) at every level, so their convs run conv1d_mfma_kernel<.., true> followed by
# sd_post_kernel; no case above reaches convp16_kernel's flat-image mode with its LeakyReLU + column-split output stage.
# (4, 45, 25) is the smallest shape of the table's kind that does: level 1 has 45 * 32 = 1440 flat positions, 12 tiles x B = 48,
# so the level-1 conv and its input gradient run convp16_kernel while levels 2-4 (24 / 12 / 12 tiles) stay on the tiled kernel.
DISC_SPEC_BF16_CASES = [(3, 7, 33), (2, 3, 1025), (4, 45, 25)]
DISC_SPEC_TIED = (3, 9, 25)  # rows 0 and 1 of pred equal target: two thirds of every real - gen map are +0.0, the median is 0

# Waveform discriminator, (B, N).  CfRun::geometry: t = (N - 1024) // 512 + 1 windows of 1024 samples every 512, the tail is
# dropped; level-l tensors are [B][C][t * P_l], P = 1280/320/80/40/20 with L = 1024/256/64/32/16 valid positions.  cf_fold_kernel
# adds the (at most two) windows w1 - 1, w1 = n // 512 that cover sample n and must leave the dropped tail at exactly zero.
DISC_WAVE_CASES = [
    (1, 1024),  # [16] one window, no tail; the level-4 tensors are 20 positions per row, far below any conv tile
    (2, 1535),  # [32] one window and the longest dropped tail (511 samples): d_pred[:, 1024:] stays exactly zero
    (1, 1536),  # [32] the first two-window length; samples 512 .. 1023 lie in both windows
    (3, 2047),  # [96] two windows + a 511-sample tail, three rows
    (2, 2560),  # [128] four windows, no tail
    (1, 3583),  # [80] five windows (odd count) + a 511-sample tail
]

# Pitch / duration discriminators, (name, dim_in, K, B, T); name "pitch" / "dur": the fixture's weights, "seeded": disc_seq_params.
# pd_score_kernel / pd_gz_kernel own 64 columns per workgroup; K = 21 and K = 5 take pd_score_wgrad_kernel<K>, every other odd
# K <= 31 takes pd_score_wgrad_generic_kernel.  The dense convs are conv1d_mfma_kernel<2,2,1,1> (64 couts x 64 columns; <1,4,1,2>
# for the input gradient of layer 0, whose packed Cout is 32).
DISC_SEQ_CASES = [
    ("pitch", 2, 21, 2, 63), ("pitch", 2, 21, 2, 64), ("pitch", 2, 21, 2, 65),  # [126 ..] one column below / on / above a workgroup
    ("dur", 1, 5, 2, 63), ("dur", 1, 5, 2, 64), ("dur", 1, 5, 2, 65),
    ("pitch", 2, 21, 4, 7),    # [28] T < K // 2 = 10: every tap row is clipped on both sides, taps 0 .. 3 and 17 .. 20 never land
    ("dur", 1, 5, 8, 2),       # [16] T = K // 2: the duration discriminator sees token counts
    ("seeded", 3, 7, 3, 65),   # [195] K = 7: the generic score weight-gradient kernel; one column into the second workgroup
    ("seeded", 1, 1, 4, 5),    # [20] K = 1: pad 0, the generic kernel with a single tap
]
DISC_SEQ_TIED = ("dur", 1, 5, 3, 64)  # rows 0 and 1 of pred equal target


def disc_spec_inputs(B, H, W, tied=False):
    """magnitude-like target and prediction [B, 1, H, W] (the recipe of test_discriminators.py); tied: rows 0, 1 of pred = target.
    The noise of 0.6 puts the level-0 relativistic term of the fixture's weights at 0.02 .. 0.037, below tau = 0.04 at every level
    of every case (its gradient is live, test_disc_oracle.py asserts it) and large enough for the choice of the median to show in
    the loss VALUES; at the 0.4 of test_discriminators.py the upper median would move them by less than two gates."""
    g = torch.Generator().manual_seed(B * 1000 + W + 7 * H)
    t = torch.rand(B, 1, H, W, generator=g) ** 2 * 3
    q = (t + (0.1 if tied else 0.6) * torch.randn(B, 1, H, W, generator=g)).abs()
    if tied:
        q[:2] = t[:2]
    return t, q


def disc_wave_inputs(B, N):
    """(the seed's + 1: with N + B alone the cases (2, 2560) and (1, 3583) hold a unit of the ReLU behind last.0 whose
    pre-activation is 3e-7, inside the fp32 rounding of that tensor (2e-6) -- at such a kink the gradient is whatever side the
    rounding falls on, and there is nothing to compare; test_disc_oracle.py asserts the margin of every case)"""
    g = torch.Generator().manual_seed(N + B + 1)
    t = 0.3 * torch.randn(B, N, generator=g)
    return t, t + 0.1 * torch.randn(B, N, generator=g)


def disc_seq_inputs(dim_in, B, T, tied=False):
    g = torch.Generator().manual_seed(9 + 100 * T + B)
    t = torch.randn(B, dim_in, T, generator=g) * 2
    q = t + (0.1 if tied else 0.5) * torch.randn(t.shape, generator=g)
    if tied:
        q[:2] = t[:2]
    return t, q


def disc_seq_params(dim_in, K, seed=31):
    """PitchDiscriminator state_dict for a tap count the fixtures do not hold: original1 normal, original0 = the row norm times
    (1 + 0.1 normal), small biases."""
    g = torch.Generator().manual_seed(seed + 1000 * K + dim_in)
    p = {}
    for name, shapes in (("discriminators", [(64, dim_in, K)] + [(64, 64, K)] * 4), ("out", [(1, 64, K)] * 5)):
        for i, s in enumerate(shapes):
            v = torch.randn(s, generator=g) / (s[1] * s[2]) ** 0.5
            p[f"{name}.{i}.parametrizations.weight.original1"] = v
            p[f"{name}.{i}.parametrizations.weight.original0"] = (
                v.flatten(1).norm(dim=1) * (1 + 0.1 * torch.randn(s[0], generator=g))).view(-1, 1, 1)
            p[f"{name}.{i}.bias"] = 0.05 * torch.randn(s[0], generator=g)
    return p


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
