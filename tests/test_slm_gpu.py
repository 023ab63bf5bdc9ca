"""The slm path on the device (stylish_tts_amd/slm.py, csrc/wavlm.hip) against tests/golden/slm_*: transformers' own WavLMModel
run on the CPU in float64 and fp32 on key-filled weights (tools/gen_slm_golden.py).  Reads tests/golden only; imports neither
transformers nor the reference.

Gate of a hidden state: what this project uses for a third-party network (profiles/pitch_parity_table.txt):
device-to-float64 <= max(1e-5 max|ref64|, 4 x max|ref32 - ref64|), both numbers from the fixture.  Gate of the loss: twice that
(a mean of absolute differences of two stacks, each within the gate).  Every parity test prints its line before it asserts;
profiles/slm_parity_table.txt keeps them.
"""
import ctypes as C
import functools
import json
import math
import os

import pytest
import torch

from stylish_tts_amd import lib as L
from stylish_tts_amd import slm
from tests import slm_cases as SC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def golden():
    from safetensors.torch import load_file
    t = {}
    for f in ("slm_small", "slm_full2", "slm_full12_a", "slm_full12_b"):
        t.update(load_file(os.path.join(GOLDEN, f + ".safetensors")))
    return t, json.load(open(os.path.join(GOLDEN, "slm_small.json")))


@functools.lru_cache(maxsize=None)
def model(cname):
    m = slm.WavLM(**SC.CONFIGS[cname])
    m.load_state_dict(SC.wavlm_weights(SC.CONFIGS[cname]), strict=True)
    return m.to(DEV).eval()


def case_gate(name):
    t, _ = golden()
    return SC.forward_gate(t[name + ".max"].item(), t[name + ".own"].item())


@pytest.mark.parametrize("name", list(SC.CASES))
def test_hidden_states_and_loss_vs_the_class(name):
    t, meta = golden()
    cname, n16, B, T, keep = SC.CASES[name]
    assert meta["cases"][name]["T"] == T
    gate = case_gate(name)
    with torch.no_grad():
        h0 = model(cname)(SC.wave(n16, B, 0).to(DEV))
        h1 = model(cname)(SC.wave(n16, B, 1).to(DEV))
        loss = slm.l1_mean(h0, h1).item()
    torch.cuda.synchronize()
    assert h0.shape == (SC.CONFIGS[cname].get("num_hidden_layers", 12) + 1, B, T, model(cname).cfg["hidden_size"])
    errs = {i: (h0[i].double().cpu() - t[f"{name}.h{i}"]).abs().max().item() for i in keep}
    want = t[name + ".loss"].item()
    print(f"slm_parity {name}: T {T}  max|ref| {t[name + '.max'].item():.4f}  reference fp32-to-f64 {t[name + '.own'].item():.3e}  "
          f"device-to-f64 {max(errs.values()):.3e} (states {', '.join(f'{i}: {e:.2e}' for i, e in errs.items())})  gate {gate:.3e}  "
          f"loss {loss:.6f} ref {want:.6f} |diff| {abs(loss - want):.2e} gate {2 * gate:.2e}")
    assert torch.isfinite(h0).all()
    assert max(errs.values()) <= gate, errs
    assert abs(loss - want) <= 2 * gate


def test_a_wave_without_a_frame_is_refused():
    with torch.no_grad():
        with pytest.raises(L.StyError, match="no frame"):
            model("small")(torch.zeros(2, 399, device=DEV))
    T = C.c_int()
    lib = L.load()
    assert lib.sty_wavlm_frames(model("small")._handle, 399, C.byref(T)) == -2  # STY_ESHAPE
    L.check(lib.sty_wavlm_frames(model("small")._handle, 400, C.byref(T)))
    assert T.value == 1


def test_rows_do_not_depend_on_their_neighbours():
    gate = case_gate("small_7777")
    x = SC.wave(7777, 3, 0).to(DEV)
    with torch.no_grad():
        full = model("small")(x)
        worst = max((full[:, b:b + 1] - model("small")(x[b:b + 1])).abs().max().item() for b in range(3))
    print(f"slm_parity batch independence: B=3 rows vs B=1 {worst:.3e}  gate {gate:.3e}")
    assert worst <= gate


def test_the_same_inputs_give_the_same_bits():
    x0, x1 = SC.wave(5200, 2, 0).to(DEV), SC.wave(5200, 2, 1).to(DEV)
    with torch.no_grad():
        a = slm.l1_mean(model("small")(x0), model("small")(x1))
        b = slm.l1_mean(model("small")(x0), model("small")(x1))
    assert a.item() == b.item() and math.isfinite(a.item()) and a.item() > 0


@pytest.mark.parametrize("N", SC.RESAMPLE_N)
def test_resampler_vs_float64_restatement(N):
    x = SC.resample_input(N)
    ref64, ref32 = SC.resample(x), SC.resample(x, dtype=torch.float32)
    gate = SC.forward_gate(ref64.abs().max().item(), (ref32.double() - ref64).abs().max().item())
    with torch.no_grad():
        y = slm.resample(x.to(DEV), 24000, 16000)
    assert y.shape == (2, (2 * N + 2) // 3) == ref64.shape
    err = (y.double().cpu() - ref64).abs().max().item()
    print(f"slm_parity resampler N={N}: max|ref| {ref64.abs().max().item():.4f}  restatement fp32-to-f64 "
          f"{(ref32.double() - ref64).abs().max().item():.3e}  device-to-f64 {err:.3e}  gate {gate:.3e}")
    assert err <= gate


def test_bucket_tables_are_the_class_tables():
    _, meta = golden()
    lib = L.load()
    for T, nb, md in SC.BUCKET_TABLES:
        out = (C.c_int32 * (2 * T - 1))()
        L.check(lib.sty_wavlm_rel_buckets_host(T, nb, md, out))
        assert list(out) == meta["bucket_tables"][f"{T}_{nb}_{md}"], (T, nb, md)


def test_validation_record_gains_slm_and_nothing_else_moves(tmp_path):
    """one acoustic step on the sample dataset, then --validate-only on its checkpoint without and with a small-config snapshot:
    metrics, total and best_loss are bit-identical, "slm" is absent without the option and equals WavLMLoss on the same batches'
    audio_gt and predicted audio with it"""
    import sys
    import yaml
    from safetensors.torch import save_file
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root_dir, "tools"))
    from make_sample_dataset import make
    from stylish_tts_amd import train as T
    from stylish_tts_amd.data import to_step_inputs
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    root = tmp_path / "data"
    make(str(root), 8, 11)
    cfg, mdl, out = tmp_path / "config.yml", tmp_path / "model.yml", tmp_path / "out"
    cfg.write_text(_default_config_yaml(root, acoustic=dict(epochs=1)))
    mdl.write_text(_default_model_yaml())
    snap = tmp_path / "wavlm"
    snap.mkdir()
    json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in SC.SMALL.items()}, open(snap / "config.json", "w"))
    save_file(SC.wavlm_weights(SC.SMALL), str(snap / "model.safetensors"))
    T.train(str(cfg), str(mdl), str(out), "acoustic", max_steps=1, log=lambda s: None)
    final = os.path.join(str(out), "acoustic", "checkpoint_final")
    logs0, logs1 = [], []
    c0 = T.train(str(cfg), str(mdl), str(tmp_path / "v0"), "acoustic", checkpoint=final, validate_only=True, log=logs0.append)
    c1 = T.train(str(cfg), str(mdl), str(tmp_path / "v1"), "acoustic", checkpoint=final, validate_only=True, log=logs1.append,
                 slm_path=str(snap))
    torch.cuda.synchronize()
    r0, r1 = c0.validation, c1.validation
    assert "slm" not in r0 and not any("slm" in ln for ln in logs0 if ln.startswith("Validation step"))
    assert math.isfinite(r1["slm"]) and r1["slm"] > 0
    assert {k: v for k, v in r1.items() if k not in ("slm", "samples")} == {k: v for k, v in r0.items() if k != "samples"}
    assert r0["metrics"] == r1["metrics"] and r0["total"] == r1["total"] and c0.manifest.best_loss == c1.manifest.best_loss
    assert "slm" not in r1["metrics"]
    v0, v1 = ([ln for ln in lg if ln.startswith("Validation step")] for lg in (logs0, logs1))
    assert v1[:-1] == v0 and v1[-1] == f"Validation step {r1['step']}: slm: {r1['slm']:.3f}"
    # the same batches through a WavLMLoss of their own
    own = slm.WavLMLoss(str(snap), 24000, 16000).to(c1.device)
    c1.slm = c1.stage.trainer.slm = None
    vals = []
    for _, batch in T._validation_pass(c1, c1.stage, lambda s: None).batches():
        kw = to_step_inputs(batch, c1.device)
        _, extra = c1.stage.trainer.validate(**kw)
        assert "slm" not in extra
        with torch.no_grad():
            vals.append(float(own(kw["audio_gt"], extra["audio"])))
    assert len(vals) == r1["batches"] and r1["slm"] == sum(vals) / len(vals)
