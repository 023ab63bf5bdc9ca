"""Leaf reductions of the backward that no longer run as passes of their own on the main stream: the bias
gradient of the many-tap 32 -> 32-channel convs as a by-product of their weight-gradient kernel (wgradp32_kernel, K 13 .. 24),
and the second stage of the two-stage reductions (bias gradient of a dense conv, weight / bias gradient of a depthwise conv)
as one wave per output with a fixed-order float64 shuffle reduction."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _wgrad(lib, L, B, Ci, Co, K, T, x_dev, w_dev, g_dev, mode):
    need = C.c_size_t()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.sty_conv1d_bwd_workspace_bytes(B, Ci, Co, K, T, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    dw, db = torch.empty(Co, Ci, K, device=DEV), torch.empty(Co, device=DEV)
    L.prof_report(256)
    lib.sty_prof_enable(1)
    try:
        L.check(lib.sty_conv1d_bwd(B, Ci, Co, K, 1, T, L.ptr(x_dev), L.ptr(w_dev), L.ptr(g_dev), L.ptr(dw), L.ptr(db), None,
                                   L.ptr(ws), ws.numel(), mode, st))
        torch.cuda.synchronize()
    finally:
        lib.sty_prof_enable(0)
    return dw.cpu(), db.cpu(), [r["name"] for r in L.prof_report(256)]


@pytest.mark.parametrize("T", [64, 200, 260])
@pytest.mark.parametrize("K", [13, 21, 24])
def test_many_tap_weight_gradient_kernel_produces_the_bias_gradient(K, T, monkeypatch):
    """32 -> 32 channels with bias, bf16 mode, dilation 1, B = 2: wgradp32_kernel<6,...> (K 13 .. 24) leaves the bias gradient
    behind like its K <= 12 instantiation, so no bias_grad_part_kernel runs.  dbias against the float64 sum of the same fp32
    gradient tensor at the bound of the fused bias gradient of K <= 12 (test_hip_parity.test_dense_conv1d_vs_torch: 2e-5 of the
    largest element); dw at that test's bound on the bf16-rounded operands.  T = 64: one exact chunk of 64 samples (plus the
    halo's); 200: several chunks, a ragged last one; 260: T % 64 != 0 with T % 4 == 0."""
    from stylish_tts_amd import lib as L
    lib = L.load()
    monkeypatch.setenv("STY_CONV32P_MIN_TILES", "1")
    B, Ci, Co = 2, 32, 32
    g = torch.Generator().manual_seed(1000 * K + T)
    x, w = torch.randn(B, Ci, T, generator=g), torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5
    gy = torch.randn(B, Co, T, generator=g)
    rnd = lambda t: t.bfloat16().double()
    # 'same' padding as the entry point pads it: (K - 1) / 2 samples on the left, the rest of K - 1 on the right (K may be even)
    xp = torch.nn.functional.pad(rnd(x), ((K - 1) // 2, K - 1 - (K - 1) // 2))
    wr = rnd(w).requires_grad_(True)
    (torch.nn.functional.conv1d(xp, wr, None) * rnd(gy)).sum().backward()
    ref_dw, ref_db = wr.grad.float(), gy.double().sum((0, 2)).float()
    dw, db, names = _wgrad(lib, L, B, Ci, Co, K, T, x.to(DEV), w.to(DEV), gy.to(DEV), 1)
    e_dw = (dw - ref_dw).abs().max().item() / ref_dw.abs().max().item()
    e_db = (db - ref_db).abs().max().item() / ref_db.abs().max().item()
    print(f"\n  K {K} T {T}: dw {e_dw:.3e}  dbias {e_db:.3e} (relative to the largest element); kernels {names}")
    assert any(n.startswith("wgradp32_kernel<6,true>") for n in names), names
    assert not any(n.startswith("bias_grad") for n in names), names
    assert e_dw <= 2e-5 and e_db <= 2e-5


def test_many_tap_weight_gradient_bias_with_a_two_byte_x(monkeypatch):
    """the same with x stored as a bf16 tensor (the 75T-rate activations of the bf16 mode): K = 21, T = 200"""
    from stylish_tts_amd import lib as L
    lib = L.load()
    monkeypatch.setenv("STY_CONV32P_MIN_TILES", "1")
    B, Ci, Co, K, T = 2, 32, 32, 21, 200
    g = torch.Generator().manual_seed(77)
    x, w = torch.randn(B, Ci, T, generator=g), torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5
    gy = torch.randn(B, Co, T, generator=g)
    rnd = lambda t: t.bfloat16().double()
    xr, wr = rnd(x).requires_grad_(True), rnd(w).requires_grad_(True)
    (torch.nn.functional.conv1d(xr, wr, None, padding=(K - 1) // 2) * rnd(gy)).sum().backward()
    ref_dw, ref_db = wr.grad.float(), gy.double().sum((0, 2)).float()
    dw, db, names = _wgrad(lib, L, B, Ci, Co, K, T, x.bfloat16().to(DEV), w.to(DEV), gy.to(DEV), 3)
    e_dw = (dw - ref_dw).abs().max().item() / ref_dw.abs().max().item()
    e_db = (db - ref_db).abs().max().item() / ref_db.abs().max().item()
    print(f"\n  two-byte x, K {K} T {T}: dw {e_dw:.3e}  dbias {e_db:.3e}; kernels {names}")
    assert any(n.startswith("wgradp32_kernel<6,true>") for n in names), names
    assert not any(n.startswith("bias_grad") for n in names), names
    assert e_dw <= 2e-5 and e_db <= 2e-5


@pytest.mark.parametrize("C_", [1, 32])
@pytest.mark.parametrize("nblk", [1, 63, 64, 65, 320])
def test_partial_sums_are_the_rounded_float64_sum_and_repeat_to_the_bit(nblk, C_):
    """bias_grad_sum_kernel and dwconv_bwd_w_sum_kernel (K = 7) on partials of the caller: every output equals the float64 sum
    of its partials rounded once to fp32, to the last bit, and a second run gives the same bits.  Partial counts below, at,
    and above one stride of the 64 lanes and at the 75T rate's 320.  (The partials are fp32 values on a 2^-16 grid below 8:
    their float64 sum is exact in any order, so the host's order and the kernel's cannot differ by a rounding.)"""
    from stylish_tts_amd import lib as L
    lib = L.load()
    K = 7
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(10 * nblk + C_)
    grid = lambda *s: (torch.randn(*s, generator=g).clamp(-7.9, 7.9) * 65536).round() / 65536
    pb, pw = grid(C_, nblk), grid(C_, nblk, K + 1)
    ref_b = pb.double().sum(1).float()
    ref_w = pw.double().sum(1).float()
    pbd, pwd = pb.to(DEV), pw.to(DEV)
    runs = []
    for _ in range(2):
        db0, dw1, db1 = torch.zeros(C_, device=DEV), torch.zeros(C_, K, device=DEV), torch.zeros(C_, device=DEV)
        L.check(lib.sty_partial_sum(0, L.ptr(pbd), C_, 0, nblk, None, L.ptr(db0), st))
        L.check(lib.sty_partial_sum(1, L.ptr(pwd), C_, K, nblk, L.ptr(dw1), L.ptr(db1), st))
        torch.cuda.synchronize()
        runs.append((db0.cpu(), dw1.cpu(), db1.cpu()))
    assert torch.equal(runs[0][0], ref_b)
    assert torch.equal(runs[0][1], ref_w[:, :K]) and torch.equal(runs[0][2], ref_w[:, K])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


def test_partial_sums_repeat_to_the_bit_on_full_mantissa_partials():
    """The same two kernels on partials that use the whole fp32 mantissa and 30 binades (randn x 2^randint): here the float64 sum
    DOES depend on the order (the host's differs from the kernel's in the last bits of the double, so no host reference to the
    bit), and a reduction whose order varied from launch to launch -- an atomic one -- would not repeat.  Eight launches each,
    C = 32, 320 partials: every launch gives the bits of the first, and the value is the host's float64 sum to one fp32 ulp."""
    from stylish_tts_amd import lib as L
    lib = L.load()
    C_, K, nblk = 32, 7, 320
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(4321)
    wide = lambda *s: torch.randn(*s, generator=g) * torch.pow(2.0, torch.randint(-15, 15, s, generator=g).float())
    pb, pw = wide(C_, nblk), wide(C_, nblk, K + 1)
    pbd, pwd = pb.to(DEV), pw.to(DEV)
    runs = []
    for _ in range(8):
        db0, dw1, db1 = torch.zeros(C_, device=DEV), torch.zeros(C_, K, device=DEV), torch.zeros(C_, device=DEV)
        L.check(lib.sty_partial_sum(0, L.ptr(pbd), C_, 0, nblk, None, L.ptr(db0), st))
        L.check(lib.sty_partial_sum(1, L.ptr(pwd), C_, K, nblk, L.ptr(dw1), L.ptr(db1), st))
        torch.cuda.synchronize()
        runs.append(torch.cat([db0.cpu(), dw1.cpu().flatten(), db1.cpu()]))
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    ref_w = pw.double().sum(1)
    ref = torch.cat([pb.double().sum(1), ref_w[:, :K].flatten(), ref_w[:, K]])
    ulp = torch.pow(2.0, torch.floor(torch.log2(ref.abs().clamp_min(1e-300))) - 23)
    assert ((runs[0].double() - ref).abs() <= ulp).all()


# ---- the harmonic-prior branch beside the trunk ----
@pytest.fixture(scope="module")
def sp_case():
    from oracle import frontend
    from oracle.manifest import speech_predictor_manifest
    from oracle.weights import fill_state_dict
    from tests.cases import make_ragged
    P = fill_state_dict(speech_predictor_manifest(), 0)
    cs = make_ragged(12, [12, 9], T=40)  # B = 2, L = 12, T = 40
    cs["alignment"] = frontend.duration_to_alignment(cs["durations"])
    cs["voiced"] = (cs["pitch"] > 20).float()
    return P, cs


def _steps(P, cs, n, with_stream, expect_beside=False):
    """n train steps (forward + backward, gradients zeroed in between) of one model object -> per step a dict of tensors.
    expect_beside: after every forward the library must report that the prior branch ran on the style stream (else: in place)"""
    import stylish_tts_amd as S
    from stylish_tts_amd import lib as L
    m = S.SpeechPredictor()
    m.load_state_dict({k: v.clone() for k, v in P.items()}, strict=False)
    m = m.to(DEV).enable_training().set_train_opts(compute_bf16=True)
    d = lambda k: cs[k].to(DEV)
    side = torch.cuda.Stream(device=DEV) if with_stream else None
    out = []
    for _ in range(n):
        for p in m.parameters():
            if p.grad is not None:
                p.grad.zero_()
        if side is not None:  # `style` arrives on the style stream, as the style encoder's output does
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                style = d("style") * 1.0
        else:
            style = d("style")
        audio = m.forward_train(d("texts_a"), d("text_lengths"), d("alignment"), d("pitch"), d("energy"), d("voiced"), style,
                                d("pitch"), noise=d("noise"), style_stream=side)
        where = C.c_void_p()
        L.check(L.load().sty_speech_branch_stream(m._handle, C.byref(where)))
        assert (where.value or 0) == (side.cuda_stream if expect_beside else 0), (where.value, expect_beside)
        d_style, d_energy = m.backward(torch.sign(audio) / audio.numel())
        torch.cuda.synchronize()
        r = {"audio": audio.cpu(), "d_style": d_style.cpu(), "d_energy": d_energy.cpu()}
        for k, p in m.named_parameters():
            if p.grad is not None:
                r["grad " + k] = p.grad.detach().cpu().clone()
        out.append(r)
    return out


N_SINGLE, N_MULTI = 24, 48


def test_prior_branch_beside_the_trunk_equals_the_single_stream_step(sp_case, monkeypatch):
    """One speech-predictor train step (B = 2, T = 40, L = 12, bf16 mode, the persistent 32-channel kernel forced onto the small
    launches) with a style stream -- the prior branch's resblocks and their backward on that stream (the library says so:
    sty_speech_branch_stream), its head in front of the wait for `style` -- against the step as it was issued before the branch
    was moved, in both its forms: every internal stream off (sty_set_single_stream(1), N_SINGLE = 24 steps) and the multi-stream
    step without a style stream (branch in place on the main stream, weight gradients on their stream: N_MULTI = 48 steps).
    The same kernels with the same arguments, so every tensor -- audio, d_style, d_energy, every parameter gradient -- is held
    to what those 72 steps do among themselves, tensor by tensor:

      * the 72 steps give every element its envelope [min, max] and every tensor its own spread (the largest envelope width);
      * a tensor whose spread is zero has to be BIT-IDENTICAL in the overlapped steps: the audio and every gradient summed in a
        fixed order, which includes the prior branch's own d alpha accumulators and the consumers of its dgb slices (two
        addends at B = 2: a float-atomic sum of two commutes);
      * a tensor with a spread (the float-atomic sums of DESIGN.md section 7 item 7 that show at this shape: d_style and the
        decoder's three one-channel convs, ten tensors) may leave its envelope by at most its own spread.

    Why the baseline holds multi-stream steps: these sums are a few atomic adds whose order depends on what shares the chip.
    Alone on the chip (single-stream) a tensor can show a spread of one ulp of an element over 24 steps and three ulp beside the
    weight-gradient stream: measured over 4 x (24 single-stream + 24 multi-stream + 24 overlapped) steps, the multi-stream steps
    left the single-stream envelope by up to 2 of the tensor's single-stream spread and the overlapped ones by up to 3
    (decoder.N_conv.bias: 7.3e-12 against 1.5e-11 and 2.2e-11), while the overlapped steps left the envelope of 24 multi-stream
    steps by at most 0.66 of the tensor's multi-stream spread (decoder.F0_conv ... weight.original1).  In those 288 steps no tensor outside
    the ten moved in any mode.

    The overlapped step runs four times in a row on one model object: a buffer recycled too early shows up as a difference."""
    from stylish_tts_amd import lib as L
    lib = L.load()
    P, cs = sp_case
    for k in ("STY_CONV32P_MIN_TILES", "STY_CONVK1_MIN_TILES"):
        monkeypatch.setenv(k, "1")
    try:
        lib.sty_set_single_stream(1)
        base = _steps(P, cs, N_SINGLE, True)
        lib.sty_set_single_stream(0)
        base += _steps(P, cs, N_MULTI, False)
        over = _steps(P, cs, 4, True, expect_beside=True)
    finally:
        lib.sty_set_single_stream(0)
    assert base[0].keys() == over[0].keys()
    assert float(base[0]["audio"].abs().max()) > 1e-3 and sum(k.startswith("grad ") for k in base[0]) > 100
    bad, moving = [], 0
    for k in base[0]:
        st = torch.stack([r[k] for r in base])
        lo, hi = st.min(0).values, st.max(0).values
        spread = (hi - lo).max().item()
        excess = [torch.maximum(lo - r[k], r[k] - hi).clamp_min(0).max().item() for r in over]
        if spread > 0 or max(excess) > 0:
            moving += spread > 0
            print(f"\n    {k:60s} spread of the {len(base)} baseline steps {spread:.3e}; overlapped steps outside their envelope: "
                  + " ".join(f"{e:.3e}" for e in excess) + f"  (scale {st.abs().max().item():.3e})", end="")
        if max(excess) > spread:
            bad.append((k, spread, excess))
    print(f"\n  {len(base[0])} tensors compared; {moving} differ among the baseline steps, the others are bit-identical throughout")
    assert not bad, bad
    assert all(torch.equal(r["audio"], base[0]["audio"]) for r in base + over)
    assert moving < 20  # (the float-atomic sums are a handful; more would mean the baseline steps themselves do not repeat)
