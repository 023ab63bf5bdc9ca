"""The pitch command on the device: the RMVPE network against the reference's recorded salience (tools/gen_pitch_golden.py) at a
small and at the full width, batch independence, the front end against the float64 restatement of tests/pitch_cases.py, the
decode kernel, the chain salience -> f0 against the reference's float64 f0, and `python -m stylish_tts_amd.pitch` end to end.

Every parity gate is tests/test_align_gpu.py::forward_gate: max(1e-5 max|ref64|, 4 x max|ref32 - ref64|), both reference runs
in the fixture (or, for the front end, both runs of the restatement); the three numbers are printed per case."""
import json
import math
import os
import sys

import pytest
import torch
from safetensors.torch import load_file, save_file

from tests import pitch_cases as PC

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
_MODELS = {}


def device_model(name):
    import stylish_tts_amd as S
    if name not in _MODELS:
        cfg = PC.SMALL if name == "small" else PC.FULL
        m = S.RMVPE(**cfg)
        m.load_state_dict(PC.rmvpe_weights(cfg), strict=True)
        _MODELS[name] = m.to(DEV).eval()
    return _MODELS[name]


def net_fixture(name, n):
    return load_file(os.path.join(G, f"pitch_{name}_n{n}.safetensors"))


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(G, "pitch_small.safetensors")), json.load(open(os.path.join(G, "pitch_small.json")))


def run_net(m, x):
    with torch.no_grad():
        out = m.mel2hidden(x.to(DEV))
    torch.cuda.synchronize()
    return out.cpu()


# ---- the network ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PC.NET_FRAMES)
def test_network_vs_reference_fixture_small(n):
    """n_blocks = 2, inter_layers = 2, en_out_channels = 4; B = 2; the frame axis is reflected by 15 / 0 / 31 / 3 / 0 frames.
    Negative control at n = 33: the input zero-padded to 64 frames instead (no reflection left to do) must turn the gate red."""
    fx = net_fixture("small", n)
    ref64, ref32 = fx["salience_f64"], fx["salience_f32"]
    gate, scale, own = PC.forward_gate(ref64, ref32)
    m = device_model("small")
    got = run_net(m, fx["input"])
    err = (got.double() - ref64).abs().max().item()
    print(f"\n  pitch_parity small n={n}: max|ref| {scale:.4f}  reference fp32-to-f64 {own:.3e}  device-to-f64 {err:.3e}  gate {gate:.3e}")
    assert got.shape == (2, n, PC.N_CLASS) and bool(torch.isfinite(got).all())
    assert err <= gate
    if n == 33:
        zero = run_net(m, torch.nn.functional.pad(fx["input"], (0, 31)))[:, :n]
        err_zero = (zero.double() - ref64).abs().max().item()
        print(f"  pitch_parity small n={n}: zero padding instead of reflection {err_zero:.3e}")
        assert err_zero > gate, "a wrong frame padding must turn the gate red"


def test_network_vs_reference_fixture_full_size():
    """E2E0(4, 1, (2, 2)): 90 M parameters, B = 2, n = 61"""
    fx = net_fixture("full", 61)
    ref64, ref32 = fx["salience_f64"], fx["salience_f32"]
    gate, scale, own = PC.forward_gate(ref64, ref32)
    got = run_net(device_model("full"), fx["input"])
    err = (got.double() - ref64).abs().max().item()
    print(f"\n  pitch_parity full n=61: max|ref| {scale:.4f}  reference fp32-to-f64 {own:.3e}  device-to-f64 {err:.3e}  gate {gate:.3e}")
    assert got.shape == (2, 61, PC.N_CLASS) and bool(torch.isfinite(got).all())
    assert err <= gate


def test_a_row_does_not_depend_on_its_batch():
    """row 0 of a B = 3 call against its own B = 1 call (and B = 6: two groups of the recurrent kernel, the second one ragged)"""
    fx = net_fixture("small", 61)
    gate, scale, own = PC.forward_gate(fx["salience_f64"][:1], fx["salience_f32"][:1])
    m = device_model("small")
    x = fx["input"]
    alone = run_net(m, x[:1])
    three = run_net(m, torch.cat([x, 0.5 * x[:1] - 1.0]))
    six = run_net(m, torch.cat([x[1:], 0.5 * x - 1.0, x[1:], x[:1], x[1:]]))
    d3 = (three[0].double() - alone[0].double()).abs().max().item()
    d6 = (six[4].double() - alone[0].double()).abs().max().item()
    print(f"\n  pitch_parity batch independence: B=3 row 0 vs B=1 {d3:.3e}  B=6 row 4 vs B=1 {d6:.3e}  gate {gate:.3e}")
    assert d3 <= gate and d6 <= gate
    assert (alone[0].double() - fx["salience_f64"][0]).abs().max().item() <= gate


# ---- the front end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [18000, 24000])
def test_front_end_vs_float64_restatement(N):
    """a harmonic signal with leading and trailing zero padding, as audio_list produces, B = 2; compared in the linear domain
    exp(logmel) so that no entry is excluded; the gate's second term is the restatement's own fp32 run.  Frames that see only
    zeros must be log(1e-5) exactly (one bit pattern)."""
    import stylish_tts_amd as S
    audio = PC.harmonic_audio(N)
    ref64 = PC.mel_linear(audio, torch.float64).clamp(min=1e-5)
    ref32 = PC.mel_linear(audio, torch.float32).clamp(min=1e-5)
    gate, scale, own = PC.forward_gate(ref64, ref32)
    with torch.no_grad():
        got = S.RMVPE.mel(audio.to(DEV))
    torch.cuda.synchronize()
    got = got.cpu()
    n = (2 * N // 3) // 200 + 1
    assert got.shape == (2, PC.N_MELS, n) and bool(torch.isfinite(got).all())
    err = (got.double().exp() - ref64).abs().max().item()
    print(f"\n  pitch_parity front end N={N}: max|ref| {scale:.4f}  restatement fp32-to-f64 {own:.3e}  device-to-f64 {err:.3e}  gate {gate:.3e}")
    assert err <= gate
    silent = PC.mel_linear(audio, torch.float64).abs().amax(dim=1) == 0  # [B, n]
    assert int(silent[0].sum()) >= 3 and int(silent[1].sum()) >= 3
    floor = torch.tensor(math.log(1e-5), dtype=torch.float32)
    assert bool((got.transpose(1, 2)[silent] == floor).all())


# ---- decode --------------------------------------------------------------------------------------------------------------
def device_decode(hidden, thred=0.03):
    import stylish_tts_amd as S
    f0 = S.RMVPE.decode(hidden.to(DEV), thred)
    torch.cuda.synchronize()
    return f0.cpu()


def test_decode_kernel_on_the_cases(gold):
    """the rows of tests/test_pitch.py on the device, against the reference function's float64 run under the same gate"""
    fx, meta = gold
    names = meta["decode_cases"]
    rows, ref32, ref64 = fx["decode.rows"], fx["decode.f0_f32"].double(), fx["decode.f0_f64"]
    got = device_decode(rows[None])[0].double()
    gated = [i for i, k in enumerate(names) if k != "at_threshold"]
    gate, scale, own = PC.forward_gate(ref64[gated], ref32[gated])
    err = (got[gated] - ref64[gated]).abs().max().item()
    print(f"\n  pitch_parity decode: max|ref| {scale:.3f}  reference fp32-to-f64 {own:.3e}  device-to-f64 {err:.3e}  gate {gate:.3e}")
    assert err <= gate
    want = PC.decode(rows)  # the kernel sums in double: the fp32 rounding of the exact expression
    assert torch.equal(got.float(), want.float())
    assert got[names.index("quiet")].item() == 0.0
    assert got[names.index("at_threshold")].item() > 0  # `< thred` in fp32, as the reference's fp32 run
    # a batch of frames through one launch: [B, n, 360] in, [B, n] out, rows in order
    many = device_decode(rows.repeat(3, 1).reshape(3, len(names), PC.N_CLASS))
    assert many.shape == (3, len(names)) and torch.equal(many[2].double(), got)
    assert device_decode(rows[None], thred=0.95)[0].count_nonzero().item() == sum(float(r.max()) >= 0.95 for r in rows)


@pytest.mark.parametrize("name", ["small", "full"])
def test_f0_chain_vs_reference_float64(gold, name):
    """device salience -> device decode against the reference's float64 f0 at n = 64 (seed 11, input 2 randn - 5).  Frames whose
    float64 top-2 margin is <= 2 x the salience gate are left out (the arg-max may legitimately move there), at most 10 % of
    them.  The bound per frame: a salience error of at most g (the gate) on each of the window's nine bins moves
    cents = sum s c / sum s by at most 9 g 80 / sum s (the window spans +-80 cents around its centre), i.e. f0 by the factor
    ln 2 / 1200 of that; on top, 1e-5 f0 for the fp32 arithmetic of the reference's own decode (the gate's first term)."""
    fx, meta = gold
    g = meta["chain"][name]["salience_gate"]
    f64, margin = fx[f"chain.{name}.f0_f64"], fx[f"chain.{name}.margin_f64"]
    m = device_model(name)
    sal = run_net(m, PC.net_input(64))
    f0 = device_decode(sal).double()
    keep = margin > 2 * g
    left_out = 1.0 - keep.double().mean().item()
    c = sal.argmax(dim=2, keepdim=True)
    idx = torch.arange(PC.N_CLASS)
    ws = (sal * ((idx >= c - 4) & (idx < c + 5))).sum(2).double()
    bound = f64 * (math.log(2) / 1200.0) * (9 * 80 * g / ws) + 1e-5 * f64
    excess = ((f0 - f64).abs() - bound)[keep].max().item()
    print(f"\n  pitch_parity f0 chain {name} n=64: salience gate {g:.3e}  minimum margin {margin.min().item():.3e}  left out "
          f"{100 * left_out:.1f} %  max|f0 - ref| {(f0 - f64).abs()[keep].max().item():.3e}  largest bound {bound[keep].max().item():.3e}")
    assert left_out <= 0.10
    assert bool((f64[keep] > 0).all()) and excess <= 0


# ---- the command ---------------------------------------------------------------------------------------------------------
def test_pitch_command_end_to_end(tmp_path):
    """config.yml + model.yml + a small-width key-filled rmvpe.safetensors + a synthetic dataset without a pitch file ->
    `python -m stylish_tts_amd.pitch` -> pitch.safetensors: the keys are both lists' names, every entry is float32
    [1, frame_count] and equals the module chain run one wave at a time; SampleDataset loads the file."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_sample_dataset as M
    from stylish_tts_amd import data as D
    from stylish_tts_amd import pitch as P
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    root = tmp_path / "data"
    lines = M.make(str(root), n=10, seed=21, n_val=2)
    os.remove(root / "pitch.safetensors")
    ckpt = tmp_path / "rmvpe.safetensors"
    save_file({k: v.contiguous() for k, v in PC.rmvpe_weights(PC.SMALL).items()}, str(ckpt))
    cfg, mdl = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg.write_text(_default_config_yaml(root))
    mdl.write_text(_default_model_yaml())
    logged = []
    result = P.pitch(str(cfg), str(mdl), 8, "rmvpe", rmvpe_path=str(ckpt), batch_size=8, log=logged.append)
    line = [ln for ln in logged if "audio-seconds per second" in ln]
    assert line, logged
    print("\n  " + line[0])
    stored = load_file(str(root / "pitch.safetensors"))
    names = [ln.split("|")[0] for ln in lines]
    assert sorted(stored) == sorted(names) and sorted(result) == sorted(names)
    ds = D.SampleDataset(data_list=lines, root_path=str(root / "wav-dir"), pitch_path=str(root / "pitch.safetensors"),
                         alignment_path=str(root / "alignment.safetensors"))
    m = device_model("small")
    worst = 0.0
    for i, name in enumerate(names):
        _, _, path, wave, pitch, _ = ds[i]
        frames = wave.shape[0] // 300
        got = stored[name]
        assert got.dtype == torch.float32 and got.shape == (1, frames), (name, got.shape, frames)
        assert not bool(torch.isnan(got).any()) and torch.equal(pitch, got)
        with torch.no_grad():
            f0 = m.infer_from_audio(wave[None].to(DEV))
        assert f0.shape == (1, frames + 1)
        want = P.to_pitch_entry(f0[0])
        gate = 1e-5 * want.abs().max().item()  # the gate's first term: there is one arithmetic on both sides
        worst = max(worst, (got - want).abs().max().item() / max(gate, 1e-30))
        assert (got - want).abs().max().item() <= gate, name
    print(f"  batched command vs one wave at a time: worst distance {worst:.3f} gates")
    # the command-line form runs the same pass, at another batch size, and replaces the file
    P.main([str(cfg), "--model-config", str(mdl), "--rmvpe", str(ckpt), "-bs", "3", "-k", "2"])
    again = load_file(str(root / "pitch.safetensors"))
    assert sorted(again) == sorted(names)
    assert all((again[k] - stored[k]).abs().max().item() <= 1e-5 * stored[k].abs().max().item() for k in stored)
