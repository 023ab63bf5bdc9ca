"""The fp32 split mode (bf16x3) of the persistent 32-channel conv on the device: the unit conv against float64 on the unrounded
operands and against the fp32 kernel's own error, the AdaptiveGeneratorBlock (Snake prologue, residual, output statistics), the
vocoder end to end at the fp32 parity gates, and `speak --compute bf16x3` against `--compute fp32`."""
import ctypes as C
import os

import pytest
import torch
from safetensors.torch import load_file, save_file

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
SPLIT, FP32 = "conv32p_kernel<split>", "conv32p_kernel<false>"
TILE = 256  # columns of the split kernel's tile (conv32p.hip: the fp32 mode's, so the min-tiles threshold counts the same)


def dev(t):
    return t.to(DEV)


def _profiled(fn):
    """fn() with the profiler on -> (its result, {kernel name: launches})"""
    from stylish_tts_amd import lib as L
    lib = L.load()
    L.prof_report(512)
    lib.sty_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.sty_prof_enable(0)
    rows = {}
    for r in L.prof_report(512):
        rows[r["name"]] = rows.get(r["name"], 0) + r["launches"]
    return out, rows


def _unit_conv(shape, mode, x, w, b):
    from stylish_tts_amd import lib as L
    lib = L.load()
    B, Ci, Co, K, d, T = shape
    y = torch.empty(B, Co, T, device=DEV)
    need = C.c_size_t()
    L.check(lib.sty_conv1d_workspace_bytes(Co, Ci, K, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.sty_conv1d_fwd(B, Ci, Co, K, d, T, L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(ws), ws.numel(), mode, st))
    torch.cuda.synchronize()
    return y.cpu()


UNIT_SHAPES = [(2, 32, 32, 11, 5, 700), (3, 32, 32, 21, 1, 1333), (2, 22, 32, 7, 1, 513), (1, 32, 30, 11, 3, 100),
               (5, 32, 32, 11, 3, 2049),
               (2, 32, 32, 11, 1, TILE - 1), (2, 32, 32, 11, 3, TILE + 1), (1, 32, 32, 11, 5, 2 * TILE + 1),
               (2, 32, 32, 11, 1, 6),
               (96, 32, 32, 11, 1, 1100),    # 480 tiles of 256 columns: one or two per workgroup
               (160, 32, 32, 11, 1, 1100)]   # 800 tiles: three or four per workgroup, both output stages and the plane buffer reused


@pytest.mark.parametrize("shape", UNIT_SHAPES)
def test_unit_conv_split_vs_float64_and_the_fp32_kernel(shape, monkeypatch):
    """sty_conv1d_fwd in compute mode 4 (split) and 0 (the fp32 kernel) on the same operands; float64 reference on the UNROUNDED
    operands.  Gates: the project's conv gate 2e-5, and 3 x the fp32 kernel's own error + 1e-6 (another summation order and six
    times as many partial products per output; a two-piece split sits 5-10 x above fp32 accumulation error and fails this one).
    The bf16 kernel, which compute mode 4 meant before the split existed, misses both by ~500 x."""
    monkeypatch.setenv("STY_CONV32P_MIN_TILES", "1")
    B, Ci, Co, K, d, T = shape
    if shape[0] == 160:
        assert B * -(-T // TILE) > 3 * 256
    g = torch.Generator().manual_seed(sum(shape))
    x, w, b = torch.randn(B, Ci, T, generator=g), torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5, torch.randn(Co, generator=g)
    ref = torch.nn.functional.conv1d(x.double(), w.double(), b.double(), padding=(K - 1) * d // 2, dilation=d)
    xd, wd, bd = dev(x), dev(w), dev(b)
    y4, rows4 = _profiled(lambda: _unit_conv(shape, 4, xd, wd, bd))
    y0, rows0 = _profiled(lambda: _unit_conv(shape, 0, xd, wd, bd))
    err_split = (y4.double() - ref).abs().max().item()
    err_fp32 = (y0.double() - ref).abs().max().item()
    print(f"\n  conv1d {shape}: max|err| vs float64  split {err_split:.3e}  fp32 kernel {err_fp32:.3e}  kernels {sorted(rows4)}")
    assert rows4.get(SPLIT, 0) == 1 and FP32 not in rows4, rows4
    assert rows0.get(FP32, 0) == 1 and SPLIT not in rows0, rows0
    assert bool(torch.isfinite(y4).all())
    assert err_split <= 2e-5
    assert err_split <= 3 * err_fp32 + 1e-6


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from oracle import frontend, speech_predictor as osp
    from oracle.manifest import speech_predictor_manifest
    from oracle.weights import fill_state_dict
    from tests.cases import make_case
    P = fill_state_dict(speech_predictor_manifest(), 0)
    cs = make_case("sp_small")
    ali = frontend.duration_to_alignment(cs["durations"])
    voiced = (cs["pitch"] > 20).float()
    want = {}
    with torch.no_grad():
        ref_audio = osp.speech_predictor(P, cs["texts"], cs["text_lengths"], ali, cs["pitch"], cs["energy"], voiced,
                                         cs["style"], cs["pitch"], cs["noise"], want)
    return dict(P=P, cs=cs, voiced=voiced, want=want, ref_audio=ref_audio)


def _predictor(P, split):
    import stylish_tts_amd as S
    m = S.SpeechPredictor()
    m.load_state_dict({k: v.clone() for k, v in P.items()}, strict=False)
    m = m.to(DEV)
    if split:
        m.set_fp32_split(True)
    m._ensure(torch.device(DEV))
    return m


def _rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def test_resblock_split_vs_reference_golden(env, monkeypatch):
    """AdaptiveGeneratorBlock (AdaIN + Snake prologue, residual, output statistics for the next AdaIN) through sty_resblock_fwd on
    a model with the split on, against the reference's block output in tests/golden/blocks.safetensors at test_adain_resblock's
    tolerance (1e-5 of the tensor's scale); the same call with the split off is reported beside it."""
    from oracle.weights import fill_tensor
    from oracle import manifest as M
    from stylish_tts_amd import lib as L
    from tests.cases import make_case
    monkeypatch.setenv("STY_CONV32P_MIN_TILES", "1")
    lib = L.load()
    prefix = "generator.basegen.amp_prior_block"
    shapes = {}
    M._gen_block(shapes, "res", 32, 64)
    P = dict(env["P"])
    for k, s in shapes.items():
        key = prefix + k[len("res"):]
        assert key in P and tuple(P[key].shape) == tuple(s), key
        P[key] = fill_tensor(k, s, 0)
    cb = make_case("blocks")
    ref = load_file(os.path.join(G, "blocks.safetensors"))["resblock32"]
    x, style = dev(cb["x32"]), dev(cb["style"])
    B, _, T = cb["x32"].shape
    out = {}
    for split in (True, False):
        m = _predictor(P, split)
        y = torch.empty(B, 32, T, device=DEV)
        ws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _, rows = _profiled(lambda: L.check(lib.sty_resblock_fwd(m._handle, prefix.encode(), B, T, L.ptr(x), L.ptr(style), L.ptr(y),
                                                                 L.ptr(ws), ws.numel(), st)))
        out[split] = (y.cpu(), rows)
    e_split, e_fp32 = _rel_err(out[True][0], ref), _rel_err(out[False][0], ref)
    print(f"\n  resblock32 vs the reference: split {e_split:.3e}  fp32 {e_fp32:.3e}  split vs fp32 {_rel_err(out[True][0], out[False][0]):.3e}"
          f"  split launches {out[True][1].get(SPLIT, 0)}")
    assert out[True][1].get(SPLIT, 0) >= 1 and FP32 not in out[True][1], out[True][1]
    assert SPLIT not in out[False][1] and out[False][1].get(FP32, 0) >= 1, out[False][1]
    assert bool(torch.isfinite(out[True][0]).all()) and e_split <= 1e-5


def _mel_l1(a, b):
    from oracle.frontend import calculate_mel
    return (calculate_mel(a.squeeze(1), 512, 512, 300) - calculate_mel(b.squeeze(1), 512, 512, 300)).abs().mean().item()


def test_vocoder_end_to_end_split(env, monkeypatch):
    """test_vocoder_end_to_end's case (B = 2, T = 80, explicit source through prior_override) and gates -- the taps at their
    tolerances, waveform MSE <= 1e-8, mel-L1 <= 1e-3 -- with the split on and the 32-channel convs forced onto the persistent
    kernel: split launches, no fp32 launch of that kernel.  Switched off again, the model's audio is bit for bit that of a model
    that never had the split on."""
    monkeypatch.setenv("STY_CONV32P_MIN_TILES", "1")
    cs, want, ref = env["cs"], env["want"], env["ref_audio"]
    B, T = cs["pitch"].shape
    Tu = 75 * T
    taps = {k: torch.zeros(*shape, device=DEV) for k, shape in dict(
        tap_conformer_out=(B, 256, T), tap_prior=(B, 300 * T), tap_har_spec=(B, 32, Tu), tap_har_phase=(B, 32, Tu),
        tap_logamp_prior=(B, 32, Tu), tap_phase_prior=(B, 32, Tu), tap_trunk=(B, 32, Tu), tap_logamp=(B, 32, Tu)).items()}
    args = dict(mel=dev(want["decoder_out"]), style=dev(cs["style"]), pitch=dev(cs["pitch"]), voiced=dev(env["voiced"]),
                noise=dev(cs["noise"]), prior_override=dev(want["prior"]))
    m = _predictor(env["P"], True)
    with torch.no_grad():
        a1, rows = _profiled(lambda: m.vocoder_forward(taps=taps, **args).audio.cpu())
    bad = []
    for name, got, exp, tol in (("conformer_out", taps["tap_conformer_out"], want["conformer_out"], 1e-5),
                                ("har_spec", taps["tap_har_spec"], want["har_spec"], 1e-5),
                                ("cos(har_phase)", torch.cos(taps["tap_har_phase"]), torch.cos(want["har_phase"]), 1e-3),
                                ("logamp_prior", taps["tap_logamp_prior"], want["logamp_prior"], 1e-4),
                                ("phase_prior", taps["tap_phase_prior"], want["phase_prior"], 5e-3),
                                ("trunk", taps["tap_trunk"], want["trunk"], 1e-5),
                                ("logamp", taps["tap_logamp"], want["logamp"], 1e-5)):
        e = _rel_err(got, exp)
        print(f"\n  {name:16s} rel_err {e:9.3e}  tol {tol:.1e}", end="")
        if not (e <= tol and bool(torch.isfinite(got).all())):
            bad.append(name)
    mse, l1 = ((a1 - ref) ** 2).mean().item(), _mel_l1(a1, ref)
    print(f"\n  audio, split on: max|err| {(a1 - ref).abs().max().item():.3e} mse {mse:.3e} mel-L1 {l1:.3e}  "
          f"split launches {rows.get(SPLIT, 0)}")
    assert not bad, bad
    assert mse <= 1e-8 and l1 <= 1e-3
    assert rows.get(SPLIT, 0) >= 1 and FP32 not in rows, rows
    m.set_fp32_split(False)
    never = _predictor(env["P"], False)
    with torch.no_grad():
        a_off, rows_off = _profiled(lambda: m.vocoder_forward(**args).audio.cpu())
        a_never = never.vocoder_forward(**args).audio.cpu()
    assert SPLIT not in rows_off and rows_off.get(FP32, 0) >= 1, rows_off
    assert torch.equal(a_off, a_never)
    assert not torch.equal(a_off, a1)  # (the split kernels really computed the first audio)
    # switched on for a model that has run already (a live handle: the shell binds and finalizes again for the fragment triples)
    never.set_fp32_split(True)
    with torch.no_grad():
        a_late, rows_late = _profiled(lambda: never.vocoder_forward(**args).audio.cpu())
    assert rows_late.get(SPLIT, 0) >= 1 and FP32 not in rows_late, rows_late
    assert (a_late - a1).abs().max().item() <= 1e-6  # the audio of the model that had the split on from the start


def test_speak_bf16x3_vs_fp32(tmp_path, monkeypatch):
    """Speaker(compute="bf16x3") and Speaker(compute="fp32") on the checkpoint fixture of the speak end-to-end test, the same
    line and seed: audio of equal length, waveform MSE <= 1e-8 (the fp32 waveform gate; the harmonic source sees bit-identical
    pitch in both modes, only the speech predictor's 32-channel convs change), and the split kernels ran in the one mode alone."""
    from stylish_tts_amd import speak as SP
    from tests.test_boundary import _default_model_yaml
    from tests.test_voicepack_gpu import _write_checkpoint
    monkeypatch.setenv("STY_CONV32P_MIN_TILES", "1")
    mdl = tmp_path / "model.yml"
    mdl.write_text(_default_model_yaml())
    ckpt = str(tmp_path / "ckpt")
    _write_checkpoint(ckpt)
    pack = str(tmp_path / "voice.safetensors")
    save_file({"voicepack_static": torch.randn(512, 192, generator=torch.Generator().manual_seed(3)) * 0.5}, pack)
    line = "ɑbɐ ɒdæ ɓfʙ, ɑβɔ ɕçɗ ɖðʤ əɘɚ ɛɜɝ."
    audio, rows = {}, {}
    for mode in ("fp32", "bf16x3"):
        sp = SP.Speaker(ckpt, str(mdl), pack, compute=mode)
        assert sp.compute == mode
        audio[mode], rows[mode] = _profiled(lambda: sp.speak(line, seed=4))
    assert audio["fp32"].shape == audio["bf16x3"].shape and audio["fp32"].shape[0] > 0
    mse = float(((audio["fp32"].astype("float64") - audio["bf16x3"].astype("float64")) ** 2).mean())
    print(f"\n  speak, {audio['fp32'].shape[0] / 24000:.2f} s: bf16x3 vs fp32 waveform mse {mse:.3e}  "
          f"split launches {rows['bf16x3'].get(SPLIT, 0)}")
    assert rows["bf16x3"].get(SPLIT, 0) >= 1 and FP32 not in rows["bf16x3"], rows["bf16x3"]
    assert SPLIT not in rows["fp32"] and rows["fp32"].get(FP32, 0) >= 1, rows["fp32"]
    assert mse <= 1e-8
