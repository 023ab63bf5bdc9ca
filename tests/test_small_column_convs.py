"""convsc_kernel (csrc/convsc.hip): the bf16-mode kernel for dense convs with few output columns -- the text encoder's convs.

Shapes: the four (Cin, Cout, K) of the text encoder, a Cout that is no multiple of the 64-row tile (80: the second tile has one
32-row block past CoutP) and two Cin that are no multiple of 64 (100: the last channel octet is half empty; 96: the waves' shares
of the reduction differ); 128 -> 512 takes the cout-split form of the kernel (256-row tiles, a wave per 64 rows), and so does
64 -> 330 at K = 5, whose second tile has three live 32-row blocks, the last of them ten rows.  B = 3; T = 100 leaves a 4-column remainder in the last 32-column tile and, with K = 1, puts utterance
boundaries inside a tile of the flattened axis; T = 36 is one tile and a 4-column one; T = 4 is shorter than the K = 5 halo.
Bound: 2e-5 of the output scale against float64 on the same bf16-rounded operands, the bound of the block-level bf16 tests
(test_persistent_conv16_on_bf16_operand_twins_vs_torch): fp32 accumulation of <= 1 536 products.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 2e-5
SHAPES = [(128, 128, 1), (128, 128, 5), (128, 512, 3), (512, 128, 3), (128, 80, 3), (100, 128, 3), (96, 64, 1), (64, 330, 5)]
LENGTHS = {100: [100, 1, 63], 36: [36, 1, 17], 4: [4, 1, 3]}  # ragged, one of them 1
# (in_mask, residual, out_mask: 0 none / 1 before the residual / 2 behind it, relu, bias)
OPTIONS = [(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 2, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1),
           (1, 1, 1, 1, 1), (1, 1, 2, 1, 1)]
SWITCHES = ("STY_NO_CONVSC", "STY_CONVSC_MAX_COLS", "STY_CONVK1_MIN_TILES", "STY_CONVP16_MIN_TILES", "STY_NO_CONVK1", "STY_NO_CONVP16")
K_SC, K_K1, K_P16, K_TILED = 2, 3, 5, 6  # STY_CONV_* of include/stylish_hip.h
F_IN_MASK, F_RESIDUAL, F_OUT_MASK, F_RELU, F_TWO_BYTE_X, F_STATS, F_Y16, F_X16 = 1, 2, 4, 8, 16, 32, 64, 128


def _lib():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from stylish_tts_amd import lib as L
    return L, L.load()


def _run(L, lib, shape, T, t, opt, ws):
    Ci, Co, K = shape
    in_mask, res, om, relu, bias = opt
    y = torch.empty(3, Co, T, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.sty_conv1d_fwd_ex(3, Ci, Co, K, 1, T, L.ptr(t["x"]), L.ptr(t["w"]), L.ptr(t["b"]) if bias else None,
                                  L.ptr(t["m"]) if in_mask else None, L.ptr(t["r"]) if res else None,
                                  L.ptr(t["m"]) if om else None, int(om == 2), relu, L.ptr(y), L.ptr(ws), ws.numel(), 1, st))
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("T", [100, 36, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "ci%d-co%d-k%d" % s)
def test_small_column_conv_vs_float64_and_the_other_families(shape, T, monkeypatch):
    """Every option alone and all together: against float64 on the rounded operands, against the kernel the conv takes with the
    family switched off (same operands, another fp32 summation order: the same bound), and two runs bit-identical."""
    L, lib = _lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    Ci, Co, K = shape
    B = 3
    g = torch.Generator().manual_seed(1000 * Ci + 10 * Co + K + T)
    x, w = torch.randn(B, Ci, T, generator=g), torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5
    b, r = torch.randn(Co, generator=g), torch.randn(B, Co, T, generator=g)
    m = (torch.arange(T)[None, :] < torch.tensor(LENGTHS[T])[:, None]).float()
    t = {k: v.to(DEV) for k, v in dict(x=x, w=w, b=b, r=r, m=m).items()}
    need = C.c_size_t()
    L.check(lib.sty_conv1d_workspace_bytes(Co, Ci, K, C.byref(need)))
    ws = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
    rnd = lambda v: v.bfloat16().double()
    conv = {im: torch.nn.functional.conv1d(rnd(x * m[:, None, :]) if im else rnd(x), rnd(w), None, padding=(K - 1) // 2) for im in (0, 1)}
    worst = [0.0, 0.0]
    for opt in OPTIONS:
        in_mask, res, om, relu, bias = opt
        ref = conv[in_mask] + (b.double()[None, :, None] if bias else 0.0)
        if relu:
            ref = ref.clamp_min(0.0)
        if om == 1:
            ref = ref * m.double()[:, None, :]
        if res:
            ref = ref + r.double()
        if om == 2:
            ref = ref * m.double()[:, None, :]
        scale = ref.abs().max().item()
        L.prof_report(64)
        lib.sty_prof_enable(1)
        try:
            y1 = _run(L, lib, shape, T, t, opt, ws)
        finally:
            lib.sty_prof_enable(0)
        names = [row["name"] for row in L.prof_report(64)]
        assert any(n.startswith("convsc_kernel") for n in names), names
        y2 = _run(L, lib, shape, T, t, opt, ws)
        monkeypatch.setenv("STY_NO_CONVSC", "1")
        lib.sty_prof_enable(1)
        try:
            y0 = _run(L, lib, shape, T, t, opt, ws)
        finally:
            lib.sty_prof_enable(0)
        monkeypatch.delenv("STY_NO_CONVSC")
        names = [row["name"] for row in L.prof_report(64)]
        assert not any(n.startswith("convsc_kernel") for n in names), names
        e64 = (y1.double() - ref).abs().max().item() / scale
        eoff = (y1 - y0).abs().max().item() / scale
        worst = [max(worst[0], e64), max(worst[1], eoff)]
        print(f"  {shape} T {T} opt {opt}: vs float64 {e64:.3e}  vs family off {eoff:.3e}  of scale {scale:.2f}")
        assert bool(torch.isfinite(y1).all())
        assert torch.equal(y1, y2), f"two runs differ: {shape} T {T} opt {opt}"
        assert e64 <= TOL and eoff <= TOL, (shape, T, opt, e64, eoff)
    print(f"\n  convsc {shape} T {T}: worst vs float64 {worst[0]:.3e}, vs family off {worst[1]:.3e} (bound {TOL:.0e})")


def _route(lib, B, Ci, Co, K, T, flags=0, dil=1, bf16=1):
    from stylish_tts_amd import lib as L
    k = C.c_int(-2)
    L.check(lib.sty_conv1d_route(B, Ci, Co, K, dil, T, bf16, flags, C.byref(k)))
    return k.value


C3_TEXT_ENCODER = [(128, 128, 1), (512, 128, 3), (128, 512, 3), (128, 128, 5)]  # B = 32, L = 100


def test_route_takes_the_text_encoder_shapes_and_declines_the_rest(monkeypatch):
    L, lib = _lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for Ci, Co, K in C3_TEXT_ENCODER:
        for flags in (0, F_IN_MASK | F_RESIDUAL | F_OUT_MASK | F_RELU):
            assert _route(lib, 32, Ci, Co, K, 100, flags) == K_SC, (Ci, Co, K, flags)
        assert _route(lib, 32, Ci, Co, K, 100, bf16=0) == K_TILED  # fp32 mode never takes it
    # the decoder's convs at 16 640 columns stay where they are
    assert _route(lib, 32, 256, 1024, 3, 520) == K_P16 and _route(lib, 32, 1024, 256, 1, 520) == K_K1
    # every declined field falls through
    assert _route(lib, 32, 128, 128, 3, 100, F_TWO_BYTE_X) == -1  # (refused: the persistent 32-channel kernel alone takes two bytes)
    assert _route(lib, 32, 128, 128, 3, 100, F_STATS) == -1
    for flags, kw in ((F_Y16, {}), (F_X16, {}), (0, dict(dil=2))):
        assert _route(lib, 32, 128, 128, 3, 100, flags, **kw) not in (K_SC, -1), (flags, kw)
    assert _route(lib, 32, 128, 128, 7, 100) not in (K_SC, -1)
    assert _route(lib, 32, 128, 128, 3, 102) not in (K_SC, -1)   # T % 4
    assert _route(lib, 32, 1024, 128, 3, 100) not in (K_SC, -1)  # Cin beyond the largest instantiation
    # the switches: off, the column bound, and an explicit threshold of a neighbouring family
    monkeypatch.setenv("STY_CONVSC_MAX_COLS", "3199")
    assert _route(lib, 32, 128, 128, 1, 100) == K_K1
    monkeypatch.setenv("STY_CONVSC_MAX_COLS", "3200")
    assert _route(lib, 32, 128, 128, 1, 100) == K_SC
    monkeypatch.delenv("STY_CONVSC_MAX_COLS")
    monkeypatch.setenv("STY_NO_CONVSC", "1")
    assert _route(lib, 32, 128, 128, 1, 100) == K_K1 and _route(lib, 32, 128, 512, 3, 100) == K_P16
    monkeypatch.delenv("STY_NO_CONVSC")
    for var in ("STY_CONVK1_MIN_TILES", "STY_CONVP16_MIN_TILES"):
        monkeypatch.setenv(var, "1")
        for Ci, Co, K in C3_TEXT_ENCODER:
            assert _route(lib, 32, Ci, Co, K, 100) in (K_K1, K_P16, K_TILED), (var, Ci, Co, K)
        monkeypatch.delenv(var)


def test_speech_predictor_step_with_the_family_on_and_off(monkeypatch):
    """One bf16-mode training step of the speech predictor at the small golden shape (B = 2, L = 40, T = 80), family on against
    off: two dispatch realisations of the same graph.  Bounds: those of
    test_bf16_mode_persistent_kernels_match_the_tiled_kernels_in_the_graphs for two realisations (a 1e-7 difference flips bf16
    roundings downstream, which the vocoder's phase path amplifies): audio 0.1, gradients 1.5 of the norm, everything finite."""
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
        if mode == "off":
            monkeypatch.setenv("STY_NO_CONVSC", "1")
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
        n_sc = sum(r["launches"] for r in rows if r["name"].startswith("convsc_kernel"))
        assert (n_sc >= 20) if mode == "on" else (n_sc == 0), (mode, n_sc)
        out[mode] = dict(audio=audio.cpu(), d_style=d_style.cpu(), g=torch.cat([p.grad.flatten().cpu() for p in sp.parameters()]))
    a, b = out["off"], out["on"]
    rel = lambda x, y: ((x - y).norm() / y.norm()).item()
    print(f"\n  convsc on vs off (bf16 mode): audio {rel(b['audio'], a['audio']):.2e}  predictor grads {rel(b['g'], a['g']):.2e}  "
          f"d_style {rel(b['d_style'], a['d_style']):.2e}")
    assert all(bool(torch.isfinite(v).all()) for v in b.values())
    assert rel(b["audio"], a["audio"]) <= 0.1 and rel(b["g"], a["g"]) <= 1.5 and rel(b["d_style"], a["d_style"]) <= 1.5
