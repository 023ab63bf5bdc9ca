"""convp16_up_kernel (csrc/convp16.hip): the generator's K = 11 pixel-shuffle up-sampling convs and their input-gradient convs on
the persistent bf16 kernel -- forward with a shuffled store, input gradient from a shuffled source, both through the unit entries
sty_conv1d_fwd_shuffle / sty_conv1d_bwd_shuffle, which also return dw / dbias from the shuffled gradient.

Shapes (Cin, Cout, s, K), B = 2: the three layers; (72, 80, 5): Cin no multiple of 32, Cout no multiple of a 32-row block, groups
of s rows that straddle blocks; (64, 96, 3): groups cut by the 64-row tile edge (as in 384 and 320); (64, 160, 5) at K = 7, the
other end of the K range the predicate admits.  T = 132: one 128-column tile and four columns; 36; 8: shorter than the halo;
130: the shuffled store asks T % 4 == 0, so the forward falls back to the tiled kernel there (the input gradient does not ask).

References: float64 on the bf16-rounded operands (x, w, the un-shuffled gradient), shuffled with a reshape.  dbias: the weight
gradient kernels of these layers are the ones they were (conv1d_wgrad_kernel), and sum the gradient as fp32, unrounded; its
reference is the float64 sum of the unrounded gradient.

Bound: 2e-5 of the quantity's scale, the block-level bf16 bound (test_small_column_convs.py), which was stated for <= 1 536
products; these reductions have up to 2 816.  So the tiled kernels (the route switched off: the parent's kernels) were measured
on the same cases; worst over all of them, tiled / this kernel: y 4.3e-7 / 6.9e-7, y with bias 3.4e-7 / 4.8e-7, dx 4.5e-7 /
9.2e-7, dx accumulated 4.2e-7 / 6.8e-7, dw 1.6e-7, dbias 1.6e-7 (the same kernels on both sides).  No parent figure exceeds 1e-5,
so the bound was not widened.  This kernel against the tiled one: at most 9.6e-7 (bit-equal on many cases: the same reduction
order chunk -> tap -> 16-channel half).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 2e-5
B = 2
SHAPES = [(256, 384, 3, 11), (128, 320, 5, 11), (64, 160, 5, 11), (72, 80, 5, 11), (64, 96, 3, 11), (64, 160, 5, 7)]
LENGTHS = [132, 36, 8, 130]
SWITCHES = ("STY_NO_CONVP16_UP", "STY_CONVP16_UP_MIN_TILES", "STY_NO_CONVP16", "STY_CONVP16_MIN_TILES", "STY_CONVK1_MIN_TILES")
K_P16, K_TILED = 5, 6  # STY_CONV_* of include/stylish_hip.h
F_RESIDUAL, F_IN_MASK, F_OUT_MASK, F_RELU, F_Y16, F_X16 = 2, 1, 4, 8, 64, 128
F_STORE, F_SOURCE, F_SHIFT = 512, 1024, 16


def _lib():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from stylish_tts_amd import lib as L
    return L, L.load()


def _shuffle(v, s):  # [B][C][T] -> [B][C / s][T s], element (c, t) at row c / s, column t s + c % s
    b, c, t = v.shape
    return v.reshape(b, c // s, s, t).permute(0, 1, 3, 2).reshape(b, c // s, t * s).contiguous()


def _unshuffle(v, s):
    b, r, ts = v.shape
    return v.reshape(b, r, ts // s, s).permute(0, 1, 3, 2).reshape(b, r * s, ts // s).contiguous()


def _reference(x, w, bias, gy, dx0, s):
    """float64 on the rounded operands: y without / with bias (shuffled), dx without / on top of dx0, dw, dbias"""
    rnd = lambda v: v.bfloat16().double()
    K = w.shape[2]
    pad = (K - 1) // 2
    xr, wr = rnd(x).requires_grad_(True), rnd(w).requires_grad_(True)
    y = torch.nn.functional.conv1d(xr, wr, None, padding=pad)
    (y * rnd(_unshuffle(gy, s))).sum().backward()
    y = y.detach()
    return dict(y=_shuffle(y, s), yb=_shuffle(y + bias.double()[None, :, None], s), dx=xr.grad, dxa=xr.grad + dx0.double(),
                dw=wr.grad, db=_unshuffle(gy, s).double().sum((0, 2)))


def _run(L, lib, shape, T, t):
    """every quantity once: (dict of CPU tensors, kernel names of the forward launches, of the backward launches)"""
    Ci, Co, s, K = shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need, need_b = C.c_size_t(), C.c_size_t()
    L.check(lib.sty_conv1d_workspace_bytes(Co, Ci, K, C.byref(need)))
    L.check(lib.sty_conv1d_bwd_workspace_bytes(B, Ci, Co, K, T, C.byref(need_b)))
    ws = torch.zeros(max(need.value, need_b.value), dtype=torch.uint8, device=DEV)
    out = {}
    L.prof_report(64)
    lib.sty_prof_enable(1)
    try:
        for key, bias in (("y", None), ("yb", L.ptr(t["b"]))):
            y = torch.full((B, Co // s, T * s), float("nan"), device=DEV)
            L.check(lib.sty_conv1d_fwd_shuffle(B, Ci, Co, K, 1, T, s, L.ptr(t["x"]), L.ptr(t["w"]), bias, L.ptr(y), L.ptr(ws),
                                               ws.numel(), 1, st))
            torch.cuda.synchronize()
            out[key] = y.cpu()
    finally:
        lib.sty_prof_enable(0)
    fwd = [r["name"] for r in L.prof_report(64)]
    lib.sty_prof_enable(1)
    try:
        for key, acc in (("dx", 0), ("dxa", 1)):
            dx = t["dx0"].clone() if acc else torch.full((B, Ci, T), float("nan"), device=DEV)
            dw, db = torch.empty(Co, Ci, K, device=DEV), torch.empty(Co, device=DEV)
            L.check(lib.sty_conv1d_bwd_shuffle(B, Ci, Co, K, 1, T, s, L.ptr(t["x"]), L.ptr(t["w"]), L.ptr(t["gy"]), L.ptr(dw),
                                               L.ptr(db), L.ptr(dx), acc, L.ptr(ws), ws.numel(), 1, st))
            torch.cuda.synchronize()
            out[key] = dx.cpu()
            if not acc:
                out["dw"], out["db"] = dw.cpu(), db.cpu()
    finally:
        lib.sty_prof_enable(0)
    bwd = [r["name"] for r in L.prof_report(64)]
    return out, fwd, bwd


_UP = "convp16_up_kernel"


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "ci%d-co%d-s%d-k%d" % s)
def test_up_conv_vs_float64_and_the_tiled_kernel(shape, T, monkeypatch):
    """Forward without / with bias, input gradient without / with a prior content of the buffer, dw, dbias: against float64 on
    the rounded operands, against the route switched off (the tiled kernel: same operands, another fp32 summation order, the
    same bound), and two runs bit-identical.  The kernels that ran are checked by name."""
    L, lib = _lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    Ci, Co, s, K = shape
    g = torch.Generator().manual_seed(1000 * Ci + 10 * Co + K + T)
    x, w = torch.randn(B, Ci, T, generator=g), torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5
    b, gy = torch.randn(Co, generator=g), torch.randn(B, Co // s, T * s, generator=g)
    dx0 = torch.randn(B, Ci, T, generator=g)
    t = {k: v.to(DEV) for k, v in dict(x=x, w=w, b=b, gy=gy, dx0=dx0).items()}
    ref = _reference(x, w, b, gy, dx0, s)
    monkeypatch.setenv("STY_CONVP16_UP_MIN_TILES", "1")
    y1, fwd, bwd = _run(L, lib, shape, T, t)
    store_takes = T % 4 == 0
    assert any(n.startswith(_UP + "<store>") for n in fwd) == store_takes, fwd
    assert any(n.startswith("conv1d_mfma_kernel") for n in fwd) != store_takes, fwd
    assert any(n.startswith(_UP + "<source>") for n in bwd) and not any(n.startswith("conv1d_mfma_kernel") for n in bwd), bwd
    y2, _, _ = _run(L, lib, shape, T, t)
    monkeypatch.setenv("STY_NO_CONVP16_UP", "1")
    y0, fwd0, bwd0 = _run(L, lib, shape, T, t)
    assert not any(n.startswith(_UP) for n in fwd0 + bwd0), (fwd0, bwd0)
    for key in ("y", "yb", "dx", "dxa", "dw", "db"):
        scale = ref[key].abs().max().item()
        e64 = (y1[key].double() - ref[key]).abs().max().item() / scale
        e64_off = (y0[key].double() - ref[key]).abs().max().item() / scale
        eoff = (y1[key] - y0[key]).abs().max().item() / scale
        print(f"  {shape} T {T} {key:3s}: vs float64 {e64:.3e}  tiled vs float64 {e64_off:.3e}  vs tiled {eoff:.3e}  scale {scale:.2f}")
        assert bool(torch.isfinite(y1[key]).all()), key
        assert torch.equal(y1[key], y2[key]), f"two runs differ: {shape} T {T} {key}"
        assert e64 <= TOL and eoff <= TOL, (shape, T, key, e64, eoff)


def _route(lib, Bn, Ci, Co, K, T, flags=0, s=0, bf16=1):
    from stylish_tts_amd import lib as L
    k = C.c_int(-2)
    L.check(lib.sty_conv1d_route(Bn, Ci, Co, K, 1, T, bf16, flags | (s << F_SHIFT), C.byref(k)))
    return k.value


C3_UP = [(256, 384, 3, 520), (128, 320, 5, 1560), (64, 160, 5, 7800)]  # B = 32


def test_routes_of_the_up_convs(monkeypatch):
    """At the model's shapes the forward and the input-gradient conv take the kernel by themselves; the test shapes take it with the
    override; the switch, the fp32 mode and every operand outside the up-convs' own fall back."""
    L, lib = _lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for Ci, Co, s, T in C3_UP:
        assert _route(lib, 32, Ci, Co, 11, T, F_STORE, s) == K_P16, (Ci, Co)
        assert _route(lib, 32, Co, Ci, 11, T, F_SOURCE, s) == K_P16, (Ci, Co)
        assert _route(lib, 32, Co, Ci, 11, T, F_SOURCE | F_RESIDUAL, s) == K_P16, (Ci, Co)
        assert _route(lib, 32, Ci, Co, 11, T, F_STORE, s, bf16=0) == K_TILED and _route(lib, 32, Co, Ci, 11, T, F_SOURCE, s, bf16=0) == K_TILED
        for extra in (F_RESIDUAL, F_IN_MASK, F_OUT_MASK, F_RELU, F_Y16, F_X16):
            assert _route(lib, 32, Ci, Co, 11, T, F_STORE | extra, s) == K_TILED, (Ci, Co, extra)
        for extra in (F_IN_MASK, F_OUT_MASK, F_RELU, F_Y16, F_X16):
            assert _route(lib, 32, Co, Ci, 11, T, F_SOURCE | extra, s) == K_TILED, (Ci, Co, extra)
        assert _route(lib, 32, Ci, Co, 11, T + 2, F_STORE, s) == K_TILED  # T % 4
        assert _route(lib, 32, Ci, Co, 13, T, F_STORE, s) == K_TILED and _route(lib, 32, Ci, Co, 5, T, F_STORE, s) == K_TILED
    assert _route(lib, 32, 256, 385, 11, 520, F_STORE, 3) == K_TILED  # Cout no multiple of s
    # the K = 11 conv without a shuffle stays where it was
    assert _route(lib, 32, 256, 384, 11, 520) == K_TILED
    for Ci, Co, s, K in SHAPES:
        assert _route(lib, B, Ci, Co, K, 132, F_STORE, s) == K_TILED and _route(lib, B, Co, Ci, K, 132, F_SOURCE, s) == K_TILED
    monkeypatch.setenv("STY_CONVP16_MIN_TILES", "1")  # (the neighbouring family's override does not move these)
    assert _route(lib, B, 64, 160, 11, 132, F_STORE, 5) == K_TILED
    monkeypatch.delenv("STY_CONVP16_MIN_TILES")
    monkeypatch.setenv("STY_CONVP16_UP_MIN_TILES", "1")
    for Ci, Co, s, K in SHAPES:
        assert _route(lib, B, Ci, Co, K, 132, F_STORE, s) == K_P16 and _route(lib, B, Co, Ci, K, 132, F_SOURCE, s) == K_P16
        assert _route(lib, B, Ci, Co, K, 130, F_STORE, s) == K_TILED and _route(lib, B, Co, Ci, K, 130, F_SOURCE, s) == K_P16
    monkeypatch.delenv("STY_CONVP16_UP_MIN_TILES")
    for var in ("STY_NO_CONVP16_UP", "STY_NO_CONVP16"):
        monkeypatch.setenv(var, "1")
        for Ci, Co, s, T in C3_UP:
            assert _route(lib, 32, Ci, Co, 11, T, F_STORE, s) == K_TILED and _route(lib, 32, Co, Ci, 11, T, F_SOURCE, s) == K_TILED
        monkeypatch.delenv(var)


def test_speech_predictor_step_with_the_up_convs_on_and_off(monkeypatch):
    """One bf16-mode training step of the speech predictor at the small golden shape (B = 2, L = 40, T = 80), the up-sampling form on
    (forced onto the small shape) against off: two dispatch realisations of the same graph, built as the step test of
    test_small_column_convs.py is and held to its bounds: audio 0.1, d_style and the gradients (all of them, and those of
    upconvs.*.weight / .bias alone) 1.5 of the norm, everything finite."""
    L, lib = _lib()
    import stylish_tts_amd as S
    from oracle import frontend
    from oracle.manifest import speech_predictor_manifest
    from oracle.weights import fill_state_dict
    from tests.cases import make_case
    P = fill_state_dict(speech_predictor_manifest(), 0)
    cs = make_case("sp_small")
    ali = frontend.duration_to_alignment(cs["durations"])
    voiced = (cs["pitch"] > 20).float()
    dev = lambda v: v.to(DEV)
    out = {}
    for mode in ("off", "on"):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("STY_NO_CONVP16_UP" if mode == "off" else "STY_CONVP16_UP_MIN_TILES", "1")
        sp = S.SpeechPredictor()
        sp.load_state_dict({k: v.clone() for k, v in P.items()}, strict=False)
        sp = sp.to(DEV).enable_training().set_train_opts(compute_bf16=True)
        L.prof_report(512)
        lib.sty_prof_enable(1)
        try:
            audio = sp.forward_train(dev(cs["texts"]), dev(cs["text_lengths"]), dev(ali), dev(cs["pitch"]), dev(cs["energy"]),
                                     dev(voiced), dev(cs["style"]), dev(cs["pitch"]), noise=dev(cs["noise"]))
            d_style, _ = sp.backward(torch.sign(audio) / audio.numel(), want_energy=False)
            torch.cuda.synchronize()
        finally:
            lib.sty_prof_enable(0)
        rows = L.prof_report(512)
        n_up = sum(r["launches"] for r in rows if r["name"].startswith(_UP))
        assert (n_up == 6) if mode == "on" else (n_up == 0), (mode, n_up)  # three layers, forward and input gradient
        named = dict(sp.named_parameters())
        up = [n for n in named if "upconvs." in n and n.endswith((".weight", ".bias"))]
        assert len(up) == 6, up
        out[mode] = dict(audio=audio.cpu(), d_style=d_style.cpu(), g=torch.cat([p.grad.flatten().cpu() for p in sp.parameters()]),
                         g_up=torch.cat([named[n].grad.flatten().cpu() for n in up]))
    a, b = out["off"], out["on"]
    rel = lambda x, y: ((x - y).norm() / y.norm()).item()
    print(f"\n  up-convs on vs off (bf16 mode): audio {rel(b['audio'], a['audio']):.2e}  predictor grads {rel(b['g'], a['g']):.2e}  "
          f"upconvs grads {rel(b['g_up'], a['g_up']):.2e}  d_style {rel(b['d_style'], a['d_style']):.2e}")
    assert all(bool(torch.isfinite(v).all()) for v in b.values())
    assert rel(b["audio"], a["audio"]) <= 0.1 and rel(b["g"], a["g"]) <= 1.5 and rel(b["g_up"], a["g_up"]) <= 1.5
    assert rel(b["d_style"], a["d_style"]) <= 1.5
