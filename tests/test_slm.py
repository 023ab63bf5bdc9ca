"""CPU-side checks of the slm path (stylish_tts_amd/slm.py): the manifest against the class's own key list, the key spellings a
hub file may carry, the config and path refusals, the frame count.  No device, no network, no transformers import."""
import json
import os

import pytest
import torch

from stylish_tts_amd import lib as L
from stylish_tts_amd import slm
from stylish_tts_amd.manifest import wavlm_manifest
from tests import slm_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_manifest_is_the_class_key_list():
    ref = json.load(open(os.path.join(GOLDEN, "manifest_wavlm.json")))
    assert wavlm_manifest() == ref
    assert "masked_spec_embed" not in ref and len(ref) == 247


def test_every_key_has_a_fill_rule_and_the_shell_its_keys():
    state = SC.wavlm_weights(SC.SMALL)
    assert set(state) == set(wavlm_manifest(**SC.SMALL))
    c = state["encoder.layers.1.attention.gru_rel_pos_const"]
    assert c.shape == (1, 4, 1, 1) and 0.0 < (c - 1).abs().max() < 2.0
    assert state["encoder.layers.0.attention.rel_attn_embed.weight"].shape == (32, 4)
    m = slm.WavLM(**SC.SMALL)
    assert set(m.state_dict()) == set(state)
    m.load_state_dict(state, strict=True)


def test_both_weight_norm_spellings_and_the_prefix_load():
    state = SC.wavlm_weights(SC.SMALL)
    g, v = "encoder.pos_conv_embed.conv.parametrizations.weight.original0", "encoder.pos_conv_embed.conv.parametrizations.weight.original1"
    old = {("wavlm." + k): t for k, t in state.items() if k not in (g, v)}
    old["wavlm.encoder.pos_conv_embed.conv.weight_g"] = state[g]
    old["wavlm.encoder.pos_conv_embed.conv.weight_v"] = state[v]
    old["wavlm.masked_spec_embed"] = torch.zeros(64)
    got = slm.normalize_state_dict(old)
    assert set(got) == set(state)
    assert all(got[k] is state[k] for k in state)
    assert set(slm.normalize_state_dict(state)) == set(state)
    with pytest.raises(RuntimeError):  # strict otherwise
        slm.WavLM(**SC.SMALL).load_state_dict({**state, "encoder.extra.weight": torch.zeros(1)}, strict=True)


@pytest.mark.parametrize("field,value", [("feat_extract_norm", "layer"), ("do_stable_layer_norm", True), ("conv_bias", True),
                                          ("hidden_act", "relu"), ("feat_extract_activation", "relu")])
def test_unsupported_config_value_is_refused_by_name(field, value):
    with pytest.raises(L.StyError, match=field):
        slm.check_wavlm_config({**SC.SMALL, field: value})
    assert slm.check_wavlm_config({})["conv_stride"] == (5, 2, 2, 2, 2, 2, 2)


def test_hub_id_or_missing_directory_raises_without_a_download(tmp_path):
    for model in ("microsoft/wavlm-base-plus", str(tmp_path / "absent"), str(tmp_path / "file.bin")):
        (tmp_path / "file.bin").write_bytes(b"x")
        with pytest.raises(L.StyError, match="--slm") as e:
            slm.WavLMLoss(model, 24000)
        assert "downloaded" in str(e.value)
    (tmp_path / "snap").mkdir()
    with pytest.raises(L.StyError, match="config.json"):
        slm.WavLMLoss(str(tmp_path / "snap"), 24000)


def test_train_refuses_a_missing_slm_directory_before_anything_else(tmp_path):
    from stylish_tts_amd import train as T
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    cfg, mdl = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg.write_text(_default_config_yaml(tmp_path / "nowhere"))
    mdl.write_text(_default_model_yaml())
    with pytest.raises(L.StyError, match="--slm") as e:
        T.train(str(cfg), str(mdl), str(tmp_path / "out"), "acoustic", slm_path="microsoft/wavlm-base-plus")
    assert "downloaded" in str(e.value)


def test_snapshot_directory_loads_both_file_formats(tmp_path):
    from safetensors.torch import save_file
    state = SC.wavlm_weights(SC.SMALL)
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in SC.SMALL.items()}
    for fmt in ("safetensors", "bin"):
        d = tmp_path / fmt
        d.mkdir()
        json.dump({**cfg, "model_type": "wavlm"}, open(d / "config.json", "w"))
        if fmt == "bin":
            torch.save({("wavlm." + k): v for k, v in state.items()}, d / "pytorch_model.bin")
        else:
            save_file(state, str(d / "model.safetensors"))
        loss = slm.WavLMLoss(str(d), 24000)
        assert loss.wavlm.cfg["hidden_size"] == 64 and (loss.model_sr, loss.slm_sr) == (24000, 16000)
        assert torch.equal(loss.wavlm.state_dict()["encoder.layer_norm.bias"], state["encoder.layer_norm.bias"])
        assert not any(p.requires_grad for p in loss.parameters())
    bad = tmp_path / "bad"
    bad.mkdir()
    json.dump({**cfg, "conv_bias": True}, open(bad / "config.json", "w"))
    save_file(state, str(bad / "model.safetensors"))
    with pytest.raises(L.StyError, match="conv_bias"):
        slm.WavLMLoss(str(bad), 24000)


def test_frame_counts_are_the_recorded_ones():
    cases = json.load(open(os.path.join(GOLDEN, "slm_small.json")))["cases"]
    assert set(cases) == set(SC.CASES)
    for name, c in cases.items():
        assert slm.wavlm_frames(c["n16"], slm.check_wavlm_config(SC.CONFIGS[c["config"]])) == c["T"], name
    assert slm.wavlm_frames(399) == 0 and slm.wavlm_frames(400) == 1
    # the c3 wave: 156 000 samples at 24 kHz -> 104 000 -> ... -> 324
    n, chain = 104000, []
    for k, s in zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)):
        n = (n - k) // s + 1
        chain.append(n)
    assert chain == [20799, 10399, 5199, 2599, 1299, 649, 324] and slm.wavlm_frames(104000) == 324


def test_forward_refuses_grad_mode_unequal_lengths_and_the_cpu(tmp_path):
    from safetensors.torch import save_file
    d = tmp_path / "snap"
    d.mkdir()
    json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in SC.SMALL.items()}, open(d / "config.json", "w"))
    save_file(SC.wavlm_weights(SC.SMALL), str(d / "model.safetensors"))
    loss = slm.WavLMLoss(str(d), 24000)
    wav = torch.zeros(1, 2400)
    with pytest.raises(L.StyError, match="backward is not built"):
        loss(wav, wav.clone().requires_grad_(True))
    with torch.no_grad():
        with pytest.raises(L.StyError, match="unequal lengths"):
            loss(wav, torch.zeros(1, 1, 2399))
        with pytest.raises(L.StyError, match="HIP device"):
            loss(wav, wav[:, None])
    with pytest.raises(L.StyError):
        loss.wavlm.enable_training()
    with pytest.raises(L.StyError, match="compute_bf16"):
        loss.wavlm.set_train_opts(compute_bf16=True)


def test_library_refuses_training_and_bf16_for_the_kind():
    """the C side itself (the shell raises before it gets there): enable_training, bind_grad and compute_bf16 on kind "wavlm"
    return STY_EINVAL and name the kind; sty_wavlm_set_config refuses another kind and a bad stride; forward before finalize is
    STY_ESTATE"""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    lib = L.load()
    h = C.c_void_p()
    assert lib.sty_model_create(b"wavlm", C.byref(h)) == 0
    assert lib.sty_model_enable_training(h) == -1 and b"wavlm" in lib.sty_last_error()
    buf = (C.c_float * 4)()
    assert lib.sty_model_bind_grad(h, b"encoder.layer_norm.weight", buf) == -1 and b"inference-only" in lib.sty_last_error()
    assert lib.sty_model_set_train_opts(h, C.byref(L.TrainOpts(0, 0, 0, 0, 0.1, 0, 0.2, 1, 0, 0.2))) == -1
    assert b"wavlm" in lib.sty_last_error()
    assert lib.sty_model_set_train_opts(h, C.byref(L.TrainOpts(0, 0, 0, 0, 0.1, 0, 0.2, 0, 0, 0.2))) == 0
    stride = (C.c_int * 7)(5, 2, 2, 2, 2, 2, 2)
    assert lib.sty_wavlm_set_config(h, 7, stride, 800, 1e-5) == 0
    assert lib.sty_wavlm_set_config(h, 7, (C.c_int * 7)(5, 2, 0, 2, 2, 2, 2), 800, 1e-5) == -1
    assert lib.sty_wavlm_set_config(h, 1, stride, 800, 1e-5) == -1
    T = C.c_int()
    assert lib.sty_wavlm_frames(h, 16000, C.byref(T)) == -5  # STY_ESTATE: not finalized
    lib.sty_model_destroy(h)
    assert lib.sty_model_create(b"rmvpe", C.byref(h)) == 0
    assert lib.sty_wavlm_set_config(h, 7, stride, 800, 1e-5) == -1
    lib.sty_model_destroy(h)


def test_host_tables_without_a_device():
    """the bucket function against the class's recorded tables, the resampler table against the float64 restatement"""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    lib = L.load()
    tables = json.load(open(os.path.join(GOLDEN, "slm_small.json")))["bucket_tables"]
    for T, nb, md in SC.BUCKET_TABLES:
        out = (C.c_int32 * (2 * T - 1))()
        L.check(lib.sty_wavlm_rel_buckets_host(T, nb, md, out))
        assert list(out) == tables[f"{T}_{nb}_{md}"], (T, nb, md)
    for orig, new, shape in ((24000, 16000, (2, 23)), (22050, 16000, None), (16000, 16000, (1, 15))):
        want = SC.resample_kernel(orig, new, torch.float32)
        if shape:
            assert tuple(want.shape) == shape
        assert lib.sty_slm_resample_kernel_host(orig, new, None) == want.numel()
        got = torch.empty(want.numel(), dtype=torch.float32)
        lib.sty_slm_resample_kernel_host(orig, new, C.c_void_p(got.data_ptr()))
        assert (got.view_as(want).double() - SC.resample_kernel(orig, new)).abs().max().item() <= 1.2e-7  # one fp32 rounding of values <= 1
    assert lib.sty_slm_resample_len(156000, 24000, 16000) == 104000 and lib.sty_slm_resample_len(7, 3, 2) == 5
