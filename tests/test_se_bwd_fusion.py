"""The style encoder's backward with the pooled-shortcut up-sample, the LeakyReLU gate and the operand twin written by the
input-gradient conv's output stage (convq_kernel<.., 1>), one twin per gradient tensor and no fp32 store without a reader
(DESIGN.md section 4.15), against the paths that keep every pass: STY_NO_TWINS=1 and STY_NO_DEFERRED_GATE=1.

Runs on the GPU box only (`-m gpu`).  The comparisons are between two runs of the same library on the same inputs; the
bounds are those of the tests in test_hip_parity.py that compare the same pairs of paths (gradient taps bit for bit between
the twin path and the fp32-operand path, 1e-6 between deferred gates and separate passes)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def _run(B, W, skip_downsamples, compute_bf16, seed):
    """one forward + backward of a fresh MelStyleEncoder under the environment as it stands; returns the style vector, the
    ten activation taps, the six gradient taps, the parameter gradients and the kernel table (family -> launches)"""
    import stylish_tts_amd as S
    from oracle.manifest import DEFAULT_CFG, style_encoder_manifest
    from oracle.weights import fill_state_dict
    from stylish_tts_amd import lib as L
    lib = L.load()
    P = fill_state_dict(style_encoder_manifest(dict(DEFAULT_CFG, se_skip_downsample=skip_downsamples)), 0)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, 80, W, generator=g) * 0.8 - 0.3
    cot = torch.randn(B, 64, generator=g)
    m = S.MelStyleEncoder(skip_downsamples=skip_downsamples)
    m.load_state_dict(P, strict=False)
    m = m.to(DEV).enable_training()
    m.set_train_opts(compute_bf16=compute_bf16)
    L.prof_report(512)
    lib.sty_prof_enable(1)
    try:
        out = m.forward_train(x.to(DEV))
        acts = [m.tap(i).cpu() for i in range(10)]
        m.backward(cot.to(DEV))
        torch.cuda.synchronize()
    finally:
        lib.sty_prof_enable(0)
    names = {r["name"]: r["launches"] for r in L.prof_report(512)}
    taps = [m.tap(i, grad=True).cpu() for i in range(6)]
    grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}
    torch.cuda.synchronize()
    return out.cpu(), acts, taps, grads, names


def _count(names, prefix):
    return sum(v for k, v in names.items() if k.startswith(prefix))


# (B, W, skip_downsamples): a batch of 1; the narrowest input the encoder takes (40 frames: the head's valid region, the
# rows the closing pool averages, is a single column; the last pooled shortcut row has 5); an odd width (the pooled rows
# replicate the last column: the factor 2 of the stage); all four ResBlks down-sampling, where the last one has no shortcut
# conv and its pooled gradient is conv2's output gradient itself (72 frames: 5 x 6 positions behind it, an even count, so
# that block has its twins too)
CASES = [(1, 84, True), (3, 40, True), (2, 131, True), (2, 72, False)]


@pytest.mark.parametrize("B,W,skip", CASES)
def test_up_stage_runs_and_gradients_equal_the_fp32_operand_path_bit_for_bit(B, W, skip, monkeypatch):
    """bf16 compute mode, every conv of the encoder sent to the twin kernels (the tile minimums lowered to 1, as the
    operand-twin test does): the run with twins must have launched the up-sample stage and no avgpool2_bwd_kernel, fewer
    cast and mask passes than gradient tensors, and must give every forward tap and every gradient tap BIT FOR BIT what
    the run on fp32 operands (STY_NO_TWINS=1: every pass in place) gives; weight gradients to the summation order of the
    two weight-gradient kernels, bias gradients to the rounding of the twin (the bounds of
    test_style_encoder_operand_twins_equal_the_fp32_operand_path)."""
    monkeypatch.setenv("STY_CONVP16_MIN_TILES", "1")
    monkeypatch.setenv("STY_CONVQ_MIN_TILES", "1")
    monkeypatch.setenv("STY_NO_TWINS", "1")
    oa, aa, ta, ga, na = _run(B, W, skip, True, 7 + W)
    monkeypatch.delenv("STY_NO_TWINS")
    ob, ab, tb, gb, nb = _run(B, W, skip, True, 7 + W)
    print(f"\n  B={B} W={W} skip={skip}: with twins: " +
          ", ".join(f"{k} x{v}" for k, v in sorted(nb.items()) if any(s in k for s in ("up", "avgpool", "twin", "pro_bwd"))))
    print("  without: " + ", ".join(f"{k} x{v}" for k, v in sorted(na.items()) if any(s in k for s in ("up", "avgpool", "twin", "pro_bwd"))))
    n_pool = 3 if skip else 4
    # without twins every pooled shortcut is up-sampled by the element-wise pass, with them by the conv's output stage
    assert _count(na, "avgpool2_bwd_kernel") == n_pool and _count(na, "convq_kernel<3,true,up>") == 0, na
    assert _count(nb, "convq_kernel<3,true,up>") == n_pool and _count(nb, "avgpool2_bwd_kernel") == 0, nb
    # one twin per gradient tensor: the cast pass is left with the tensors whose last writer has no twin output.  Every
    # configuration: the head conv's output gradient (written by the pool + Linear backward) and the last ResBlk's (the
    # head's input-gradient conv, then the gate pass).  With an identity shortcut in the last ResBlk also the head's input
    # (the shortcut is added behind conv2's twin), conv1's output gradient of that block (it has no down-sampling whose
    # backward would write the twin) and the block's input gradient (accumulated by two writers): 5.  The three shortcut
    # convs, which cast a copy of conv2's twin before, cast nothing
    assert _count(nb, "twin_cast_kernel") == (5 if skip else 2), nb
    # ... and the masked fp32 copy of the shortcut gradient (one mask pass per ResBlk with a shortcut branch in the run
    # without twins) has no reader left: every other pass of that family runs in both
    n_res = 3 if skip else 4
    assert _count(nb, "pro_bwd_kernel") == _count(na, "pro_bwd_kernel") - n_res, (na, nb)
    assert torch.equal(oa, ob)
    for i, (a, b) in enumerate(zip(aa, ab)):
        assert torch.equal(a, b), f"activation tap {i} differs: max {(a - b).abs().max().item():.3e}"
    for i, (a, b) in enumerate(zip(ta, tb)):
        assert torch.isfinite(b).all()
        assert torch.equal(a, b), f"gradient tap {i} differs: max {(a - b).abs().max().item():.3e}"
    assert ga.keys() == gb.keys() and len(ga) > 20
    for k in ga:
        if k.startswith("unshared"):
            assert rel_err(gb[k], ga[k]) <= 1e-6, k
        elif k.endswith(".bias"):
            assert rel_err(gb[k], ga[k]) <= 4e-3, (k, rel_err(gb[k], ga[k]))
        else:
            assert rel_err(gb[k], ga[k]) <= 2e-6, f"d {k} differs: {rel_err(gb[k], ga[k]):.3e}"


@pytest.mark.parametrize("B,W,skip", CASES)
def test_up_stage_equals_the_separate_gate_passes(B, W, skip, monkeypatch):
    """the same bf16 run against STY_NO_DEFERRED_GATE=1 (a gate pass behind every input-gradient conv, the element-wise
    up-sample behind it): the stage multiplies and adds the same numbers in the same order, so the gradient taps agree to
    1e-6 and the parameter gradients to the bounds of test_style_encoder_deferred_gates_equal_the_separate_passes."""
    monkeypatch.setenv("STY_CONVP16_MIN_TILES", "1")
    monkeypatch.setenv("STY_CONVQ_MIN_TILES", "1")
    monkeypatch.setenv("STY_NO_DEFERRED_GATE", "1")
    _, _, ta, ga, na = _run(B, W, skip, True, 11 + W)
    monkeypatch.delenv("STY_NO_DEFERRED_GATE")
    _, _, tb, gb, nb = _run(B, W, skip, True, 11 + W)
    assert _count(na, "convq_kernel<3,true,up>") == 0 and _count(na, "avgpool2_bwd_kernel") > 0, na
    assert _count(nb, "convq_kernel<3,true,up>") > 0 and _count(nb, "avgpool2_bwd_kernel") == 0, nb
    for i, (a, b) in enumerate(zip(ta, tb)):
        assert rel_err(b, a) <= 1e-6, f"gradient tap {i}: {rel_err(b, a):.3e}"
    assert ga.keys() == gb.keys() and len(ga) > 20
    for k in ga:
        tol = 1e-5 if k.startswith("unshared") or "fc" in k else 2e-6
        assert rel_err(gb[k], ga[k]) <= tol, f"d {k}: {rel_err(gb[k], ga[k]):.3e}"


@pytest.mark.parametrize("B,W,skip", [(1, 84, True), (3, 40, True), (2, 72, False)])
def test_fp32_mode_keeps_its_passes_and_equals_the_separate_gate_passes(B, W, skip, monkeypatch):
    """fp32 compute mode has no twins: the pooled shortcut is up-sampled by avgpool2_bwd_kernel behind conv1's input-gradient
    conv as before (the tape records the shortcut branch in front of conv1 now), and the result equals the run with
    STY_NO_DEFERRED_GATE=1 to fp32 rounding (1e-6 on the gradient taps, as the existing test asks)."""
    monkeypatch.setenv("STY_NO_DEFERRED_GATE", "1")
    _, _, ta, ga, na = _run(B, W, skip, False, 13 + W)
    monkeypatch.delenv("STY_NO_DEFERRED_GATE")
    _, _, tb, gb, nb = _run(B, W, skip, False, 13 + W)
    n_pool = 3 if skip else 4
    assert _count(nb, "avgpool2_bwd_kernel") == n_pool and _count(nb, "convq_kernel") == 0, nb
    assert _count(nb, "twin_cast_kernel") == 0, nb
    for i, (a, b) in enumerate(zip(ta, tb)):
        assert rel_err(b, a) <= 1e-6, f"gradient tap {i}: {rel_err(b, a):.3e}"
    assert ga.keys() == gb.keys() and len(ga) > 20
    for k in ga:
        tol = 1e-5 if k.startswith("unshared") or "fc" in k else 2e-6
        assert rel_err(gb[k], ga[k]) <= tol, f"d {k}: {rel_err(gb[k], ga[k]):.3e}"
