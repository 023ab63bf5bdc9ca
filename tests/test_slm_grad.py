"""The slm gradient fixtures and the Python surface of the gradient path, without a device: tests/golden/slm_grad_* against
tests/slm_grad_cases.py, the sign packing, the inputs of every gate, the condition under which the device may form the L1 signs
itself, and the refusals that need no GPU.  The gradients themselves are held on the device (tests/test_slm_grad_gpu.py)."""
import json
import os
import re

import pytest
import torch

from stylish_tts_amd import lib as L
from stylish_tts_amd import slm
from tests import slm_cases as SC
from tests import slm_grad_cases as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(names):
    from safetensors.torch import load_file
    t = {}
    for f in names:
        path = os.path.join(GOLDEN, f + ".safetensors")
        assert os.path.getsize(path) < (1 << 20), path
        t.update(load_file(path))
    return t


def test_fixture_listing_matches_the_cases():
    meta = json.load(open(os.path.join(GOLDEN, "slm_grad.json")))
    assert meta["seed"] == SC.SEED and tuple(meta["files"]) == GC.FILES
    assert set(meta["cases"]) == set(GC.CASES) == set(SC.CASES)
    t = _load(GC.FILES)
    for name, (fname, want) in GC.CASES.items():
        cname, n16, B, T, _ = SC.CASES[name]
        assert meta["cases"][name] == dict(file=fname, grads=list(want), n16=n16, B=B, T=T)
        for k in want:
            shape = (B, SC.CONFIGS[cname].get("hidden_size", 768), T) if k == "e_cot" else (B, n16)
            assert tuple(t[f"{name}.{k}"].shape) == shape and t[f"{name}.{k}"].dtype == torch.float64
        assert (f"{name}.sign" in t) == ("g_l1" in want)
    assert set(meta["e2e"]) == {str(n) for n in GC.E2E_N}
    for N in GC.E2E_N:
        assert tuple(t[f"e2e_{N}.g"].shape) == (2, N)
        assert meta["e2e"][str(N)]["T"] == SC.frames((2 * N + 2) // 3, SC.CONFIGS[GC.E2E_CONFIG])
    assert GC.cot("small_5200").shape == GC.stack_shape("small_5200") == (3, 2, 16, 64)
    assert torch.equal(GC.cot("small_5200"), GC.cot("small_5200"))


def test_sign_packing_round_trips():
    g = torch.Generator().manual_seed(5)
    for shape in ((1,), (7,), (8,), (3, 2, 24, 64), (13, 1, 81, 768)):
        sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
        packed = GC.pack_signs(sign)
        assert packed.dtype == torch.uint8 and packed.numel() == (sign.numel() + 7) // 8
        assert torch.equal(GC.unpack_signs(packed, shape), sign)
    t = _load(("slm_grad_full2",))
    assert t["full2_8000.sign"].numel() == 3 * 2 * 24 * 768 // 8  # 14 KB
    s = GC.unpack_signs(t["full2_8000.sign"], GC.stack_shape("full2_8000"))
    assert set(s.unique().tolist()) == {-1.0, 1.0}


def test_gate_inputs_are_present_and_positive():
    t = _load(GC.FILES)
    keys = [f"{n}.{k}" for n, (_, want) in GC.CASES.items() for k in want] + [f"e2e_{N}.g" for N in GC.E2E_N]
    for key in keys:
        gmax, gown = t[key + ".gmax"].item(), t[key + ".gown"].item()
        assert gmax > 0 and gown > 0 and gown < 1e-4 * gmax, key
        assert gmax == t[key].abs().max().item()
        assert GC.grad_gate(gmax, gown) == max(1e-5 * gmax, 4 * gown)
    # no frame reads the last two samples of 7777: their gradient is zero in the reference too
    assert (t["small_7777.g_cot"][:, -2:] == 0).all() and (t["small_7777.g_cot"][:, -3] != 0).all()


def test_own_sign_cases_keep_their_distance_from_a_tie():
    """the device may form sign(h1 - h0) itself only where no |h0 - h1| is within twice the forward gate: then no sign can differ
    while both stacks are inside their gates"""
    t, fwd = _load(GC.FILES), _load(("slm_small", "slm_full2", "slm_full12_b"))
    for name in GC.OWN_SIGN_CASES:
        fgate = SC.forward_gate(fwd[name + ".max"].item(), fwd[name + ".own"].item())
        assert t[name + ".mindiff"].item() > 2 * fgate, name
    for N in GC.E2E_N:
        assert t[f"e2e_{N}.mindiff"].item() > 2 * t[f"e2e_{N}.fgate"].item()
    # the others do not qualify, which is why they are held through the fixture's signs alone
    for name in ("small_22800", "full2_8000", "full12_26000"):
        fgate = SC.forward_gate(fwd[name + ".max"].item(), fwd[name + ".own"].item())
        assert t[name + ".mindiff"].item() < 2 * fgate


def test_grad_mode_refusal_of_forward_still_stands(tmp_path):
    from safetensors.torch import save_file
    json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in SC.SMALL.items()}, open(tmp_path / "config.json", "w"))
    save_file(SC.wavlm_weights(SC.SMALL), str(tmp_path / "model.safetensors"))
    crit = slm.WavLMLoss(str(tmp_path), 24000, 16000)
    wav, y = torch.zeros(2, 7800), torch.zeros(2, 7800, requires_grad=True)
    with pytest.raises(L.StyError, match="backward is not built"):
        crit(wav, y)
    with pytest.raises(L.StyError, match="frozen"):
        crit.wavlm.enable_training()
    # the explicit-gradient call refuses on the host what the forward refuses: shapes, the CPU
    with pytest.raises(L.StyError, match="unequal lengths"):
        crit.loss_and_grad(wav, torch.zeros(2, 7801))
    with pytest.raises(L.StyError, match="d_pred must be"):
        crit.loss_and_grad(wav, y.detach(), d_pred=torch.zeros(2, 7799))
    with pytest.raises(L.StyError, match="no forward_keep"):
        crit.wavlm.backward(torch.zeros(3, 2, 16, 64))
    with pytest.raises(L.StyError, match="HIP device"):
        crit.wavlm.forward_keep(torch.zeros(2, 5200))


def test_entry_points_and_options_are_declared():
    header = open(os.path.join(ROOT, "include", "stylish_hip.h")).read()
    for name in ("sty_wavlm_grad_workspace_bytes", "sty_wavlm_fwd_keep", "sty_wavlm_bwd", "sty_slm_loss_fwd_bwd", "sty_slm_resample_bwd"):
        assert re.search(rf"\bint\s+{name}\s*\(", header) and name in L.SYMBOLS, name
    from stylish_tts_amd import train as T
    with pytest.raises(L.StyError, match="--slm-train needs --slm"):
        T.train_model(None, None, "unused", "acoustic", slm_train=True)
