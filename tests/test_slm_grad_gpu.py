"""The slm term's gradient on the device (stylish_tts_amd/slm.py, csrc/wavlm.hip, csrc/attn_bwd.hip) against
tests/golden/slm_grad_*: autograd of transformers' own WavLMModel on the CPU in float64 and fp32 on key-filled weights
(tools/gen_slm_grad_golden.py).  Reads tests/golden only; imports neither transformers nor the reference.

Gate of a gradient: the project's rule for a third-party network (tests/slm_cases.forward_gate): device-to-float64 <=
max(1e-5 max|g64|, 4 x max|g32 - g64|), both numbers from the fixture.  Every parity test prints its line before it asserts;
profiles/slm_grad_table.txt keeps them.
"""
import ctypes as C
import functools
import json
import os

import pytest
import torch

from stylish_tts_amd import lib as L
from stylish_tts_amd import slm
from tests import slm_cases as SC
from tests import slm_grad_cases as GC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def golden():
    from safetensors.torch import load_file
    t = {}
    for f in GC.FILES:
        t.update(load_file(os.path.join(GOLDEN, f + ".safetensors")))
    return t


@functools.lru_cache(maxsize=None)
def model(cname):
    m = slm.WavLM(**SC.CONFIGS[cname])
    m.load_state_dict(SC.wavlm_weights(SC.CONFIGS[cname]), strict=True)
    return m.to(DEV).eval()


def gate_of(key):
    t = golden()
    return GC.grad_gate(t[key + ".gmax"].item(), t[key + ".gown"].item())


def report(what, key, got):
    """prints the parity line of gradient `key` and returns (error, gate)"""
    t = golden()
    ref = t[key]
    err = (got.double().cpu() - ref).abs().max().item()
    gate = gate_of(key)
    print(f"slm_grad {what} {key}: max|g64| {t[key + '.gmax'].item():.4e}  reference fp32-to-f64 {t[key + '.gown'].item():.3e}  "
          f"device-to-f64 {err:.3e}  gate {gate:.3e}")
    return err, gate


@pytest.mark.parametrize("name", ["small_7777", "full2_8000"])
def test_forward_keep_gives_the_bits_of_forward(name):
    cname, n16, B, _, _ = SC.CASES[name]
    x = SC.wave(n16, B, 1).to(DEV)
    with torch.no_grad():
        a = model(cname)(x)
        b = model(cname).forward_keep(x)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(GC.CASES))
def test_backward_of_a_smooth_cotangent_vs_autograd_of_the_class(name):
    cname, n16, B, T, _ = SC.CASES[name]
    want_tap = "e_cot" in GC.CASES[name][1]
    m = model(cname)
    cot = GC.cot(name, torch.float32).to(DEV)
    with torch.no_grad():
        h = m.forward_keep(SC.wave(n16, B, 1).to(DEV))
        out = m.backward(cot / h.numel(), tap=want_tap)
    torch.cuda.synchronize()
    d_audio, d_enc = out if want_tap else (out, None)
    assert d_audio.shape == (B, n16) and torch.isfinite(d_audio).all()
    if want_tap:  # first: the tap splits the transformer half from the feature-encoder half
        err, gate = report("tap", f"{name}.e_cot", d_enc)
        assert err <= gate
    err, gate = report("cot", f"{name}.g_cot", d_audio)
    assert err <= gate
    if n16 == 7777:  # remainders dropped at several strides: no frame reads the last two samples
        assert (d_audio[:, -2:] == 0).all() and (d_audio[:, -3] != 0).all()


@pytest.mark.parametrize("name", [n for n, (_, g) in GC.CASES.items() if "g_l1" in g])
def test_backward_of_the_fixture_signs_vs_autograd_of_the_l1(name):
    """the cotangent is the float64 run's sign(h1 - h0) / n: the device forms no sign of its own, so a near-tie cannot move it"""
    cname, n16, B, _, _ = SC.CASES[name]
    shape = GC.stack_shape(name)
    sign = GC.unpack_signs(golden()[f"{name}.sign"], shape).to(DEV)
    m = model(cname)
    with torch.no_grad():
        h = m.forward_keep(SC.wave(n16, B, 1).to(DEV))
        d_audio = m.backward(sign / h.numel())
    torch.cuda.synchronize()
    err, gate = report("l1-by-fixture-signs", f"{name}.g_l1", d_audio)
    assert err <= gate


def test_l1_mean_and_grad_with_planted_ties():
    g = torch.Generator().manual_seed(SC.SEED)
    for shape, scale in (((3, 2, 24, 64), 1.0), ((13, 1, 81, 768), 0.2), ((1, 1, 1, 7), 3.0)):
        a = torch.randn(shape, generator=g).to(DEV)
        b = torch.randn(shape, generator=g).to(DEV)
        ties = (torch.arange(a.numel()) % 5 == 2).reshape(shape).to(DEV)
        b = torch.where(ties, a, b).contiguous()
        with torch.no_grad():
            val, d_b = slm.l1_mean_and_grad(a, b, scale)
            want = scale * torch.sign(b - a) / a.numel()
            assert val.item() == slm.l1_mean(a, b).item()
        assert ties.any() and (d_b[ties] == 0).all()
        assert torch.equal(d_b, want), (shape, (d_b - want).abs().max().item())


@pytest.mark.parametrize("name", GC.OWN_SIGN_CASES)
def test_loss_and_grad_at_16k_with_the_devices_own_signs(name, tmp_path):
    """min |h0 - h1| exceeds twice the forward gate on these cases (asserted by the generator), so no sign can differ"""
    cname, n16, B, _, _ = SC.CASES[name]
    crit = _loss(tmp_path, 16000)
    x0, x1 = SC.wave(n16, B, 0).to(DEV), SC.wave(n16, B, 1).to(DEV)
    value, d_audio = crit.loss_and_grad(x0, x1)
    with torch.no_grad():
        assert value.item() == crit(x0, x1).item()
    err, gate = report("l1-own-signs", f"{name}.g_l1", d_audio)
    assert err <= gate


def _loss(tmp_path, model_sr):
    from safetensors.torch import save_file
    snap = tmp_path / f"wavlm_{model_sr}"
    if not snap.exists():
        snap.mkdir()
        json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in SC.SMALL.items()}, open(snap / "config.json", "w"))
        save_file(SC.wavlm_weights(SC.SMALL), str(snap / "model.safetensors"))
    return slm.WavLMLoss(str(snap), model_sr, 16000).to(DEV)


@pytest.mark.parametrize("N", SC.RESAMPLE_N)
def test_resampler_adjoint_vs_autograd_of_the_restatement(N):
    x = SC.resample_input(N)
    M = (2 * N + 2) // 3
    gen = torch.Generator().manual_seed(SC.SEED + N)
    y = torch.randn(2, M, generator=gen, dtype=torch.float64).float()
    refs = {}
    for dtype in (torch.float64, torch.float32):
        xi = x.to(dtype).requires_grad_(True)
        refs[dtype] = torch.autograd.grad((SC.resample(xi, dtype=dtype) * y.to(dtype)).sum(), xi)[0]
    ref64, ref32 = refs[torch.float64], refs[torch.float32]
    gate = SC.forward_gate(ref64.abs().max().item(), (ref32.double() - ref64).abs().max().item())
    with torch.no_grad():
        g = slm.resample_backward(y.to(DEV), N, 24000, 16000)
        Rx = slm.resample(x.to(DEV), 24000, 16000)
        base = torch.ones(2, N, device=DEV)
        acc = slm.resample_backward(y.to(DEV), N, 24000, 16000, out=base.clone())
    err = (g.double().cpu() - ref64).abs().max().item()
    print(f"slm_grad resampler adjoint N={N}: max|ref| {ref64.abs().max().item():.4f}  restatement fp32-to-f64 "
          f"{(ref32.double() - ref64).abs().max().item():.3e}  device-to-f64 {err:.3e}  gate {gate:.3e}")
    assert g.shape == (2, N) and err <= gate
    assert torch.equal(acc, base + g)  # accumulate: one fp32 add
    # adjointness, in float64 on the host from the device's outputs: <R x, y> = <x, R^T y>
    lhs = (Rx.double().cpu() * y.double()).sum().item()
    rhs = (x.double() * g.double().cpu()).sum().item()
    scale = (Rx.double().cpu() * y.double()).abs().sum().item()
    print(f"slm_grad resampler adjointness N={N}: <Rx, y> {lhs:.9e}  <x, R^T y> {rhs:.9e}  sum|terms| {scale:.3e}")
    assert abs(lhs - rhs) <= 1e-6 * scale  # fp32 outputs: each term carries 2^-24 of its size, summed in float64


@pytest.mark.parametrize("N", GC.E2E_N)
def test_loss_and_grad_at_24k_end_to_end(N, tmp_path):
    t = golden()
    crit = _loss(tmp_path, 24000)
    gt, pred = (w.to(DEV) for w in GC.e2e_waves(N))
    value, d_audio = crit.loss_and_grad(gt, pred)
    with torch.no_grad():
        assert value.item() == crit(gt, pred).item()
    print(f"slm_grad e2e_{N}: loss {value.item():.6f} ref {t[f'e2e_{N}.loss'].item():.6f} gate {2 * t[f'e2e_{N}.fgate'].item():.2e}")
    assert abs(value.item() - t[f"e2e_{N}.loss"].item()) <= 2 * t[f"e2e_{N}.fgate"].item()
    err, gate = report("end-to-end", f"e2e_{N}.g", d_audio)
    assert d_audio.shape == pred.shape and err <= gate
    # two calls give the same bits
    value2, again = crit.loss_and_grad(gt, pred)
    assert torch.equal(again, d_audio) and value2.item() == value.item()
    # d_pred= accumulation: bit-equal to d_pred + the gradient, into the tensor given
    base = torch.randn(pred.shape, generator=torch.Generator().manual_seed(N)).to(DEV)
    acc = base.clone()
    _, ret = crit.loss_and_grad(gt, pred, d_pred=acc)
    assert ret is acc and torch.equal(acc, base + d_audio)
    # weight = 0.2 is 0.2 x the cotangent route (the weight folded into the L1 cotangent), the value unchanged
    v02, g02 = crit.loss_and_grad(gt, pred, weight=0.2)
    with torch.no_grad():
        ref = crit.hidden_states(gt)
        h = crit.wavlm.forward_keep(slm.resample(pred, 24000, 16000))
        d16 = crit.wavlm.backward(0.2 * torch.sign(h - ref) / h.numel())
        route = slm.resample_backward(d16, N, 24000, 16000)
    assert v02.item() == value.item() and torch.equal(g02, route)
    worst = (g02 - 0.2 * d_audio).abs().max().item()
    print(f"slm_grad e2e_{N} weight 0.2 vs 0.2 x weight 1: {worst:.3e}  gate {0.2 * gate:.3e}")
    assert worst <= 0.2 * gate
    if N == E2E_ROWS_N:
        # row b of a B = 3 call equals its B = 1 call within the gate (the mean's 1 / n differs by the factor 3)
        gt3, pred3 = torch.cat([gt, gt[:1] * 0.5]), torch.cat([pred, pred[:1] * 0.7])
        _, g3 = crit.loss_and_grad(gt3, pred3)
        worst = max((3 * g3[b:b + 1] - crit.loss_and_grad(gt3[b:b + 1], pred3[b:b + 1])[1]).abs().max().item() for b in range(3))
        print(f"slm_grad e2e_{N} batch independence: 3 x B=3 rows vs B=1 {worst:.3e}  gate {2 * gate:.3e}")
        assert worst <= 2 * gate


E2E_ROWS_N = GC.E2E_N[0]


def test_refusals_on_the_host():
    m = model("small")
    x = SC.wave(5200, 2, 1).to(DEV)
    lib = L.load()
    with torch.no_grad():
        m.forward_keep(x)
        m.backward(torch.zeros(GC.stack_shape("small_5200"), device=DEV))
        with pytest.raises(L.StyError, match="no forward_keep"):  # consumed
            m.backward(torch.zeros(GC.stack_shape("small_5200"), device=DEV))
        m.forward_keep(x)
        with pytest.raises(L.StyError, match="another forward_keep"):
            m.backward(torch.zeros(GC.stack_shape("small_7777"), device=DEV))
        with pytest.raises(L.StyError, match="no frame"):
            m.forward_keep(torch.zeros(2, 399, device=DEV))
    # the library's own checks, below the Python layer's
    h = torch.empty(GC.stack_shape("small_5200"), device=DEV)
    d = torch.empty(2, 5200, device=DEV)
    need = m.grad_workspace_bytes(2, 5200, torch.device(DEV))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sty_wavlm_fwd_keep(m._handle, 2, 5200, L.ptr(x), L.ptr(h), L.ptr(ws), need - 4096, st) == -4  # STY_ENOMEM
    assert b"too small" in lib.sty_last_error()
    assert lib.sty_wavlm_bwd(m._handle, 2, 5200, L.ptr(h), L.ptr(d), None, L.ptr(ws), need, st) == -5  # STY_ESTATE: nothing kept
    L.check(lib.sty_wavlm_fwd_keep(m._handle, 2, 5200, L.ptr(x), L.ptr(h), L.ptr(ws), need, st))
    assert lib.sty_wavlm_bwd(m._handle, 3, 5200, L.ptr(h), L.ptr(d), None, L.ptr(ws), need, st) == -2  # STY_ESHAPE
    assert lib.sty_wavlm_bwd(m._handle, 2, 5205, L.ptr(h), L.ptr(d), None, L.ptr(ws), need, st) == -2
    assert lib.sty_wavlm_bwd(m._handle, 2, 5200, L.ptr(h), L.ptr(d), None, L.ptr(ws), need - 4096, st) == -4
    assert lib.sty_wavlm_grad_workspace_bytes(m._handle, 2, 399, C.byref(C.c_size_t())) == -2
    torch.cuda.synchronize()


def _tensors(obj, prefix=""):
    if torch.is_tensor(obj):
        yield prefix, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _tensors(v, f"{prefix}/{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _tensors(v, f"{prefix}/{i}")


def _checkpoint_tensors(path):
    out = {}
    for f in sorted(os.listdir(path)):
        if f.endswith(".bin"):
            out.update(_tensors(torch.load(os.path.join(path, f), map_location="cpu", weights_only=False), f))
    return out


def test_trainer_with_the_slm_term(tmp_path, monkeypatch):
    """two deterministic acoustic steps on the sample dataset: `slm_path` alone changes nothing of the training; with `slm_train`
    the log carries the value, the value is WavLMLoss on the step's waves, the predictor moves, and two runs repeat to the bit"""
    import sys
    from safetensors.torch import save_file
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root_dir, "tools"))
    from make_sample_dataset import make
    from stylish_tts_amd import train as T
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    root = tmp_path / "data"
    make(str(root), 8, 11)
    cfg, mdl = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg.write_text(_default_config_yaml(root, acoustic=dict(epochs=1)))
    mdl.write_text(_default_model_yaml())
    snap = tmp_path / "wavlm"
    snap.mkdir()
    json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in SC.SMALL.items()}, open(snap / "config.json", "w"))
    save_file(SC.wavlm_weights(SC.SMALL), str(snap / "model.safetensors"))
    with pytest.raises(L.StyError, match="--slm-train needs --slm"):
        T.train(str(cfg), str(mdl), str(tmp_path / "refused"), "acoustic", max_steps=2, slm_train=True, log=lambda s: None)
    seen = []
    real = slm.WavLMLoss.loss_and_grad

    def recording(self, wav, y_rec, weight=1.0, d_pred=None):
        seen.append((wav.clone(), y_rec.clone(), weight))
        return real(self, wav, y_rec, weight, d_pred=d_pred)

    monkeypatch.setattr(slm.WavLMLoss, "loss_and_grad", recording)

    def run(name, **kw):
        logs = []
        torch.manual_seed(SC.SEED)  # (train() seeds `random` alone: the models' initialisation is the caller's torch stream)
        ctx = T.train(str(cfg), str(mdl), str(tmp_path / name), "acoustic", max_steps=2, deterministic=True, log=logs.append, **kw)
        torch.cuda.synchronize()
        return ctx, logs, _checkpoint_tensors(os.path.join(str(tmp_path / name), "acoustic", "checkpoint_final"))

    try:
        _, logs_plain, plain = run("plain")
        _, logs_val, val_only = run("val_only", slm_path=str(snap))
        assert not seen and not any(", slm " in ln for ln in logs_plain + logs_val)
        assert plain.keys() == val_only.keys() and not [k for k in plain if not torch.equal(plain[k], val_only[k])]
        ctx, logs_a, with_a = run("with_a", slm_path=str(snap), slm_train=True)
        steps = [ln for ln in logs_a if ln.startswith("acoustic epoch")]
        tr = ctx.stage.trainer
        assert len(seen) == 2 and seen[-1][2] == 0.2  # loss_weight.slm of the default config
        assert steps and steps[-1].endswith(f", slm {float(tr.slm_value):.4f}")
        with torch.no_grad():
            own = slm.WavLMLoss(str(snap), 24000, 16000).to(DEV)
            assert float(own(seen[-1][0], seen[-1][1])) == float(tr.slm_value)
        assert torch.equal(seen[-1][1], tr.audio.squeeze(1))
        from stylish_tts_amd.stage_io import model_file
        moved = [k for k in plain if k.startswith(model_file("speech_predictor") + "/") and not torch.equal(plain[k], with_a[k])]
        assert moved, "the predictor's parameters did not move with the term"
        _, _, with_b = run("with_b", slm_path=str(snap), slm_train=True)
        assert with_a.keys() == with_b.keys() and not [k for k in with_a if not torch.equal(with_a[k], with_b[k])]
    finally:
        L.set_deterministic(False)
