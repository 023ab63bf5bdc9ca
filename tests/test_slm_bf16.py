"""The bf16 operand mode of the slm term, what runs without a device: the door (sty_wavlm_set_compute, WavLM.set_compute,
WavLMLoss(compute=), train --slm-bf16), the old door that stays shut, and the sanity of the fixtures the device tests read
(tests/golden/slm_bf16.json, tools/gen_slm_bf16_golden.py)."""
import ctypes as C
import json
import os

import pytest
import torch

from stylish_tts_amd import lib as L
from stylish_tts_amd import slm
from tests import slm_bf16_cases as BC
from tests import slm_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load()


def test_set_compute_accepts_the_kind_and_two_values():
    lib = _lib()
    h = C.c_void_p()
    assert lib.sty_model_create(b"wavlm", C.byref(h)) == 0
    assert lib.sty_wavlm_set_compute(h, 0) == 0 and lib.sty_wavlm_set_compute(h, 1) == 0  # before finalize
    assert lib.sty_wavlm_set_compute(h, 2) == -1 and b"0 = fp32" in lib.sty_last_error()
    assert lib.sty_wavlm_set_compute(h, -1) == -1
    assert lib.sty_wavlm_set_compute(h, 0) == 0
    # the old door still refuses, with the calls tests/test_slm.py makes, in either mode of the new one
    for mode in (0, 1):
        assert lib.sty_wavlm_set_compute(h, mode) == 0
        assert lib.sty_model_set_train_opts(h, C.byref(L.TrainOpts(0, 0, 0, 0, 0.1, 0, 0.2, 1, 0, 0.2))) == -1
        assert b"wavlm" in lib.sty_last_error() and b"sty_wavlm_set_compute" in lib.sty_last_error()
        assert lib.sty_model_set_train_opts(h, C.byref(L.TrainOpts(0, 0, 0, 0, 0.1, 0, 0.2, 0, 0, 0.2))) == 0
    lib.sty_model_destroy(h)
    assert lib.sty_model_create(b"rmvpe", C.byref(h)) == 0
    assert lib.sty_wavlm_set_compute(h, 1) == -1 and b"rmvpe" in lib.sty_last_error()
    lib.sty_model_destroy(h)
    assert lib.sty_wavlm_set_compute(None, 1) == -1
    for sym in ("sty_wavlm_set_compute", "sty_attention_rel_fwd_bwd", "sty_wavlm_strided_conv_fwd_bwd",
                "sty_wavlm_strided_conv_workspace_bytes"):
        assert sym in L.SYMBOLS


def test_unit_entries_refuse_bad_arguments_on_the_host():
    lib = _lib()
    need = C.c_size_t()
    assert lib.sty_wavlm_strided_conv_workspace_bytes(2, 64, 64, 3, 2, 130, C.byref(need)) == 0 and need.value > 0
    assert lib.sty_wavlm_strided_conv_workspace_bytes(2, 64, 64, 3, 2, 2, C.byref(need)) == -1   # Nin < k
    assert lib.sty_wavlm_strided_conv_workspace_bytes(2, 64, 64, 3, 17, 130, C.byref(need)) == -1  # stride past 16
    buf = (C.c_float * 4)()
    assert lib.sty_attention_rel_fwd_bwd(2, 3, 64, 24, buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, 2, buf, 1 << 30, None) == -1
    assert lib.sty_attention_rel_fwd_bwd(2, 3, 32, 24, buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, 0, buf, 1 << 30, None) == -1


def test_python_door_round_trips_and_the_old_one_stays_shut(tmp_path):
    from safetensors.torch import save_file
    m = slm.WavLM(**SC.SMALL)
    assert m.compute == "fp32"
    assert m.set_compute("bf16") is m and m.compute == "bf16"
    assert m.set_compute("fp32").compute == "fp32"
    with pytest.raises(L.StyError, match="'fp32' or 'bf16'"):
        m.set_compute("fp16")
    with pytest.raises(L.StyError, match="compute_bf16"):
        m.set_train_opts(compute_bf16=True)
    d = tmp_path / "snap"
    d.mkdir()
    json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in SC.SMALL.items()}, open(d / "config.json", "w"))
    save_file(SC.wavlm_weights(SC.SMALL), str(d / "model.safetensors"))
    assert slm.WavLMLoss(str(d), 24000).compute == "fp32"
    loss = slm.WavLMLoss(str(d), 24000, 16000, compute="bf16")
    assert loss.compute == "bf16" and loss.wavlm.compute == "fp32"  # (the network's mode is set per call)
    with pytest.raises(L.StyError, match="'fp32' or 'bf16'"):
        slm.WavLMLoss(str(d), 24000, compute="half")
    wav = torch.zeros(1, 2400)
    with torch.no_grad():
        with pytest.raises(L.StyError, match="'fp32' or 'bf16'"):
            loss(wav, wav, compute="half")
        with pytest.raises(L.StyError, match="HIP device"):  # the mode is set, then the device check refuses the CPU tensor
            loss(wav, wav, compute="fp32")
    assert loss.wavlm.compute == "fp32"
    with pytest.raises(L.StyError, match="compute_bf16"):
        loss.wavlm.set_train_opts(compute_bf16=True)
    from stylish_tts_amd.acoustic import AcousticTrainer
    import inspect
    assert inspect.signature(AcousticTrainer.__init__).parameters["slm_compute"].default == "fp32"


def test_slm_bf16_without_slm_train_is_refused_before_anything_loads(tmp_path):
    from stylish_tts_amd import train as T
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    cfg, mdl = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg.write_text(_default_config_yaml(tmp_path / "no_such_dataset"))
    mdl.write_text(_default_model_yaml())
    snap = tmp_path / "wavlm"
    snap.mkdir()
    with pytest.raises(L.StyError, match="--slm-bf16 needs --slm-train"):
        T.train(str(cfg), str(mdl), str(tmp_path / "out"), "acoustic", slm_path=str(snap), slm_bf16=True)
    with pytest.raises(L.StyError, match="--slm-bf16 needs --slm-train"):
        T.train(str(cfg), str(mdl), str(tmp_path / "out"), "acoustic", slm_bf16=True)
    with pytest.raises(L.StyError, match="--slm-train needs --slm"):
        T.train(str(cfg), str(mdl), str(tmp_path / "out"), "acoustic", slm_train=True, slm_bf16=True)
    assert not (tmp_path / "out").exists()


def test_fixtures_are_sane():
    listing = json.load(open(os.path.join(GOLDEN, BC.LISTING)))["cases"]
    assert set(listing) == set(BC.CASES)
    for name, (cname, n16, B, T, keep, fstride, sstride) in BC.CASES.items():
        rec = listing[name]
        assert T == SC.frames(n16, SC.CONFIGS[cname]) == rec["T"], name
        assert (rec["n16"], rec["B"], rec["frame_stride"], rec["sample_stride"]) == (n16, B, fstride, sstride)
        autos = [rec[f"r_auto.h{i}"] for i in keep] + [rec["r_auto.stack"], rec["r_auto.g_cot"]]
        assert all(0.0 < v < 0.1 for v in autos), (name, autos)
        assert all(0.0 < rec[f"r_emul.h{i}"] < 0.1 for i in keep) and 0.0 < rec["r_emul.stack"] < 0.1
        assert rec["rms.stack"] > 0 and rec["loss"] > 0
        # the autocast value sits within the bound the device is held to
        assert abs(rec["loss_auto"] - rec["loss"]) <= 2 * rec["r_auto.stack"] * rec["rms.stack"]
        states, g = BC.load_reference(name, GOLDEN)
        H = SC.CONFIGS[cname].get("hidden_size", 768)
        for i in keep:
            assert tuple(states[i].shape) == (B, len(range(0, T, fstride)), H), (name, i)
            assert torch.isfinite(states[i]).all()
        assert tuple(g.shape) == (B, len(range(0, n16, sstride))) and torch.isfinite(g).all()
        assert tuple(BC.cot(name).shape) == BC.stack_shape(name)
    for name in SC.CASES:  # the draw of the cotangent is tests/slm_grad_cases.py's
        if name in BC.CASES:
            from tests import slm_grad_cases as GC
            assert torch.equal(BC.cot(name), GC.cot(name))
    for fs in BC.NEW_FILES.values():
        for f in fs:
            assert os.path.getsize(os.path.join(GOLDEN, f + ".safetensors")) < (1 << 20)


def test_kernel_level_references_are_what_they_say():
    """the float64 attention reference against a direct loop on one small problem, and the bf16-representability of its inputs"""
    q, k, v, gate, tab, d_o = BC.attn_inputs(5, 16)
    for t in (q, k, v, d_o):
        assert torch.equal(t.bfloat16().float(), t)
    o = BC.attn_reference(q, k, v, gate, tab, d_o)[0]
    B, H, T, DH = BC.ATTN_B, BC.ATTN_H, 5, 16
    for b in range(B):
        for h in range(H):
            qs, ks, vs = (x[b, h * DH:(h + 1) * DH].double() for x in (q, k, v))
            for i in range(T):
                logit = torch.stack([(qs[:, i] * ks[:, j]).sum() / DH ** 0.5 + gate[b, h, i].double() * tab[h, j - i + T - 1].double()
                                     for j in range(T)])
                want = (torch.softmax(logit, 0)[None, :] * vs).sum(1)
                assert torch.allclose(o[b, h * DH:(h + 1) * DH, i], want, rtol=0, atol=1e-12)
    x, w, gy = BC.conv_inputs(64, 64, 3, 2, 9)
    assert gy.shape == (2, 64, 4) and torch.equal(w.bfloat16().float(), w) and torch.equal(gy.bfloat16().float(), gy)
