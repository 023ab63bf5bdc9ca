"""Sums of the backward's normalisation glue without passes of their own: the GRN backward from the per-channel
norms the forward kept, the GRN term coef * h formed inside the activation backward, and AdaIN's mean / rstd written by the
kernel that folds them.  Unit entries: sty_grn_bwd, sty_act_bwd, sty_adain_finalize.

The 2 x rule used below: the new route's error against a float64 computation may be at most twice the old route's on the same
inputs, with a floor of 1e-4 of the tensor's scale (the block gate of test_hip_parity.test_block_backward_vs_float64_oracle)."""
import ctypes as C
from fractions import Fraction

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR = 1e-4


def _lib():
    from stylish_tts_amd import lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err(got, ref):
    """max |got - ref| relative to the reference tensor's scale"""
    ref = ref.double().cpu()
    return (got.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _profiled(L, lib, fn):
    """run fn with the in-situ kernel timers on -> rows of (family, instantiations)"""
    L.prof_report(256)
    lib.sty_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.sty_prof_enable(0)
    return {r["name"]: r for r in L.prof_report(256)}


# ---- GRN ----
@pytest.mark.parametrize("B,C4,T", [(2, 128, 520), (2, 1024, 520), (2, 128, 4104), (2, 1024, 4104), (2, 128, 40000),
                                    (1, 128, 33 * 4096 - 5)])
def test_grn_backward_from_the_forwards_norms(B, C4, T):
    """sty_grn_bwd (row statistics, grn_finalize, grn_bwd): coef and dgamma with the backward starting from the norms the forward
    kept (from_gx = 1) and rebuilding them from the partial sums (from_gx = 0), both against float64 under the 2 x rule; how many
    coef elements differ between the two at all is printed (the two double sums of a channel's segments run in different orders:
    none, or a handful in the last bit).  T = 520: one segment of the statistics pass, 4104: two, 40000: ten; 33 segments (a ragged
    last one) take the wave-per-channel walk of the from-partials form, as the ConvNeXt32 blocks' ~150 tile sums did."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(C4 + T)
    h = torch.randn(B, C4, T, generator=g) * (0.2 + torch.rand(1, C4, 1, generator=g))
    ds = torch.randn(B, C4, generator=g)
    gamma = torch.randn(C4, generator=g) * 0.5
    gx = torch.sqrt((h.double() ** 2).sum(2))
    m = gx.mean(1, keepdim=True) + 1e-6
    dnx = ds.double() * gamma.double()
    dgx = dnx / m - (dnx * gx).sum(1, keepdim=True) / (m * m) / C4
    ref_coef, ref_dg = dgx / gx, (ds.double() * gx / m).sum(0)
    need = C.c_size_t()
    L.check(lib.sty_grn_bwd_workspace_bytes(B, C4, T, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    hd, dsd, gd = h.to(DEV), ds.to(DEV), gamma.to(DEV)
    out = {}
    for from_gx in (1, 0):
        coef, dg = torch.zeros(B, C4, device=DEV), torch.zeros(C4, device=DEV)
        L.check(lib.sty_grn_bwd(B, C4, T, L.ptr(hd), L.ptr(dsd), L.ptr(gd), from_gx, L.ptr(coef), L.ptr(dg), L.ptr(ws), ws.numel(),
                                _stream()))
        torch.cuda.synchronize()
        out[from_gx] = (coef.cpu(), dg.cpu())
    e = {k: (_err(v[0], ref_coef), _err(v[1], ref_dg)) for k, v in out.items()}
    ndiff = int((out[0][0] != out[1][0]).sum())
    print(f"\n  C4 {C4} T {T}: coef from gx {e[1][0]:.3e} from partials {e[0][0]:.3e}; dgamma {e[1][1]:.3e} / {e[0][1]:.3e}; "
          f"{ndiff} of {B * C4} coef elements differ between the two")
    assert e[1][0] <= max(2 * e[0][0], FLOOR) and e[1][1] <= max(2 * e[0][1], FLOOR)


# ---- activation backward with the row term ----
ACT_SNAKE, ACT_GELU = 3, 5


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("T", [4, 37, 520])
@pytest.mark.parametrize("Cc", [4, 256])
@pytest.mark.parametrize("kind", [ACT_SNAKE, ACT_GELU])
def test_activation_backward_forms_the_row_term_itself(kind, Cc, T, acc):
    """sty_act_bwd with the row term d = dy + coef[b][c] h formed in the kernel (fused = 1) against the pass of its own followed by
    the plain kernel (fused = 0): dx BIT-EQUAL -- the kernel writes the fma the separate pass compiles to --, dalpha (float atomics
    over the batch: B = 3 addends per channel) within its own run-to-run spread plus one ulp of its largest element.  T % 4 != 0
    takes the scalar path of both kernels."""
    L, lib = _lib()
    B = 3
    g = torch.Generator().manual_seed(100 * Cc + T + kind)
    x, dy, h = (torch.randn(B, Cc, T, generator=g) for _ in range(3))
    coef = torch.randn(B, Cc, generator=g) * 0.3
    alpha = torch.rand(Cc, generator=g) + 0.5
    dx0 = torch.randn(B, Cc, T, generator=g)
    xd, hd, cd, ad = x.to(DEV), h.to(DEV), coef.to(DEV), alpha.to(DEV)

    def run(fused):
        dyd, dx, dal = dy.to(DEV), dx0.to(DEV), torch.zeros(Cc, device=DEV)
        L.check(lib.sty_act_bwd(kind, B, Cc, T, L.ptr(xd), L.ptr(dyd), L.ptr(ad) if kind == ACT_SNAKE else None, L.ptr(hd), L.ptr(cd),
                                fused, L.ptr(dx), acc, L.ptr(dal) if kind == ACT_SNAKE else None, _stream()))
        torch.cuda.synchronize()
        return dx.cpu(), dal.cpu(), dyd.cpu()

    f = [run(1) for _ in range(3)]
    u = [run(0) for _ in range(3)]
    assert torch.equal(f[0][2], dy)  # the fused form leaves dy alone
    assert torch.equal(f[0][0], u[0][0])
    # against float64 as well (the row term really is in there)
    d64 = dy.double() + coef.double()[:, :, None] * h.double()
    x64 = x.double()
    if kind == ACT_SNAKE:
        a64 = alpha.double()[None, :, None]
        ref = d64 * (1.0 + torch.sin(2 * a64 * x64))
    else:
        ref = d64 * (0.5 * (1.0 + torch.erf(x64 / 2 ** 0.5)) + x64 * torch.exp(-0.5 * x64 * x64) / (2 * torch.pi) ** 0.5)
    assert _err(f[0][0], ref + (dx0.double() if acc else 0.0)) <= FLOOR
    if kind == ACT_SNAKE:
        st = torch.stack([r[1] for r in u])
        lo, hi = st.min(0).values, st.max(0).values
        slack = (hi - lo).max().item() + float(st.abs().max()) * 2.0 ** -23
        for r in f:
            assert float(torch.maximum(lo - r[1], r[1] - hi).max()) <= slack


# ---- AdaIN fold ----
@pytest.mark.parametrize("nseg", [1, 70])
def test_adain_fold_also_writes_the_statistics(nseg):
    """sty_adain_finalize on partials of the caller (B C = 5 rows): mean / rstd bit-equal to the host's float64 computation of
    the same formula from the same partials (values on a 2^-10 grid: their float64 sums are exact in any order), a / s unchanged
    by asking for the statistics."""
    L, lib = _lib()
    B, Cc, T, eps = 1, 5, 300 * nseg, 1e-5
    g = torch.Generator().manual_seed(nseg)
    grid = lambda *s: (torch.randn(*s, generator=g, dtype=torch.float64) * 1024).round() / 1024
    sm = grid(B * Cc, nseg) * 4
    sq = grid(B * Cc, nseg).abs() * 64 + 40 * T / nseg  # (keeps the variance positive)
    part = torch.stack([sm, sq], 2).contiguous()
    gb = torch.randn(B, 2 * Cc, generator=g)
    mean = sm.sum(1) / T
    q = sq.sum(1) / T
    ref_mean = mean.float()
    # var = q - mean * mean: the compiler may contract it to one fma (the exact difference rounded once); both are the formula
    var2 = q - mean * mean
    var1 = torch.tensor([float(Fraction(float(a)) - Fraction(float(b)) ** 2) for a, b in zip(q, mean)], dtype=torch.float64)
    ref_rstd = [(1.0 / torch.sqrt(v.clamp_min(0) + float(torch.tensor(eps, dtype=torch.float32)))).float() for v in (var1, var2)]
    pd, gd = part.to(DEV), gb.to(DEV)
    outs = []
    for want in (1, 0):
        a, s, mo, ro = (torch.zeros(B * Cc, device=DEV) for _ in range(4))
        L.check(lib.sty_adain_finalize(B, Cc, T, nseg, L.ptr(pd), L.ptr(gd), eps, L.ptr(a), L.ptr(s), L.ptr(mo) if want else None,
                                       L.ptr(ro) if want else None, _stream()))
        torch.cuda.synchronize()
        outs.append((a.cpu(), s.cpu(), mo.cpu(), ro.cpu()))
    assert torch.equal(outs[0][2], ref_mean)
    assert torch.equal(outs[0][3], ref_rstd[0]) or torch.equal(outs[0][3], ref_rstd[1]), (outs[0][3], ref_rstd)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], (1.0 + gb[0, :Cc]) * outs[0][3])  # a = (1 + gamma) rstd from the rstd it wrote


# ---- block level ----
@pytest.fixture(scope="module")
def weights():
    from oracle.manifest import speech_predictor_manifest
    from oracle.weights import fill_state_dict
    return fill_state_dict(speech_predictor_manifest(), 0)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("prefix,Cc,T", [("generator.basegen.amp_convnext.2", 256, 120), ("generator.basegen.upblocks.1", 64, 300)])
def test_generic_convnext_block_against_the_float64_oracle(weights, prefix, Cc, T, bf16):
    """The generic ConvNeXt block in the training graph (sty_block_fwd_bwd) as test_block_backward_vs_float64_oracle (fp32: 1e-4 of
    each tensor's scale, y 2e-5) and test_block_bf16_mode_vs_float64_oracle_on_rounded_operands (bf16 mode: the oracle on the same
    bf16-rounded GEMM operands, 1e-3) compare it, and through the in-situ timers: the GRN term ran inside the activation backward
    (no row_scale_add launch with row coefficients) and the GRN backward started from the forward's norms."""
    import contextlib

    import stylish_tts_amd as S
    from oracle import blocks
    L, lib = _lib()
    P = {k: v.clone() for k, v in weights.items()}
    g = torch.Generator().manual_seed(Cc + T)
    x, style, gy = torch.randn(2, Cc, T, generator=g), torch.randn(2, 64, generator=g), torch.randn(2, Cc, T, generator=g)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    keys = [k for k in P64 if k.startswith(prefix + ".") and P64[k].is_floating_point()]
    for k in keys:
        P64[k].requires_grad_(True)
    x64, s64 = x.double().requires_grad_(True), style.double().requires_grad_(True)
    with (blocks.bf16_operands() if bf16 else contextlib.nullcontext()):
        y64 = blocks.convnext_block(P64, prefix, x64, s64)
        (y64 * gy.double()).sum().backward()
    m = S.SpeechPredictor()
    m.load_state_dict(P, strict=False)
    m = m.to(DEV).enable_training()
    m._ensure(torch.device(DEV))
    for p_ in m.parameters():
        p_.grad.zero_()
    out = {}
    rows = _profiled(L, lib, lambda: out.update(r=m.block_forward_backward("convnext", prefix, x.to(DEV), style.to(DEV), gy.to(DEV),
                                                                           compute_bf16=bf16)))
    y, gx, d_style = out["r"]
    by_inst = {n: r["insts"] for n, r in rows.items()}
    print(f"\n  kernels: {sorted(by_inst)}")
    assert "act_bwd_kernel" in by_inst and "grn_bwd_kernel" in by_inst, by_inst
    tol = 1e-3 if bf16 else 1e-4
    bad = []

    def add(name, got, ref, t):
        e = _err(got.detach().float(), ref)
        print(f"  {name:34s} rel_err {e:9.3e}  tol {t:.1e}")
        if not (e <= t and bool(torch.isfinite(got).all())):
            bad.append(name)

    add("y", y, y64.detach().float(), tol if bf16 else 2e-5)
    add("d x", gx, x64.grad.float(), tol)
    add("d style", d_style, s64.grad.float(), tol)
    named = dict(m.named_parameters())
    for k in keys:
        if P64[k].grad is None or k not in named:
            continue
        ref = P64[k].grad.float()
        if ref.abs().max().item() < 1e-7 * max(1.0, gy.abs().max().item()):
            continue
        add("d " + k[len(prefix) + 1:], named[k].grad, ref, tol)
    assert not bad, bad
    assert "row_scale_add_kernel[coef]" not in by_inst  # (the plain add of a residual's gradient is another family)
