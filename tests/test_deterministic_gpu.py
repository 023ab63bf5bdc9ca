"""The deterministic mode on the device: training steps of all four stages repeat to the bit, the mode passes the default mode's
parity gates with their own tolerances, its gradients equal the default mode's up to summation order, it is latched by the
forward, and a workspace sized for the other mode is refused on the host.

Shapes: B = 5 (a float sum of TWO terms onto zero is the same in either order, so at the B = 2 of the other small cases every
per-(b, c) atomic is order-independent already and a repeat test there shows nothing), T = 80 frames (6000 columns at the 75T
rate), 24 tokens drawn with repeats, full-width synthetic weights.  Every test leaves the switch at 0.
"""
import ctypes as C
import importlib.util
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
B, T, LT = 5, 80, 24

from tests.test_hip_parity import env  # noqa: E402,F401  (the parity gates' module fixture)


def _tool():
    """tools/repeat_step.py: the trainers, the batch and the state walk are the tool's own (it is what a user runs)"""
    spec = importlib.util.spec_from_file_location("repeat_step", os.path.join(ROOT, "tools", "repeat_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def L():
    from stylish_tts_amd import lib
    lib.load()
    try:
        yield lib
    finally:
        lib.set_deterministic(False)


def _assert_equal(a, b, what):
    bad = [n for (n, x), (_, y) in zip(a, b) if not (torch.equal(x, y) if torch.is_tensor(x) else x == y)]
    assert [n for n, _ in a] == [n for n, _ in b]
    assert not bad, f"{what}: {len(bad)} of {len(a)} items differ, first (in backward order): {bad[:6]}"


def _repeat(stage, steps, compute="fp32"):
    RS = _tool()
    batch = RS.batch_of(B, T, LT, torch.device(DEV), ragged=stage == "alignment")
    pair = [RS.build(stage, torch.device(DEV), compute=compute, deterministic=True, train_mode=True, lr=1e-3) for _ in range(2)]
    for i in range(steps):
        losses = [RS.step(stage, tr, batch, i) for tr in pair]
        torch.cuda.synchronize()
        # after every step: the returned losses and every .grad (state_items lists them first, in backward order)
        a, b = RS.state_items(stage, pair[0], losses[0]), RS.state_items(stage, pair[1], losses[1])
        keep = lambda items: [(n, t) for n, t in items if n.startswith(("loss.", "grad "))]
        assert sum(n.startswith("grad ") for n, _ in a) > 10
        _assert_equal(keep(a), keep(b), f"{stage} step {i}")
    # at the end: every state_dict entry of every model, both AdamW moments of every optimizer, every tracked loss
    _assert_equal(a, b, f"{stage} after {steps} steps")
    return pair


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_acoustic_steps_repeat_to_the_bit(L, compute):
    """two fresh AcousticTrainers (train_mode, three SpecDiscriminators, the waveform discriminator, lr 1e-3, deterministic=True)
    from identical seeds, three steps with seed = i and disc_index (0, 2, 2)"""
    pair = _repeat("acoustic", 3, compute)
    assert L.get_deterministic() and pair[0].mrd is not None and pair[0].disc is not None and pair[0].train_mode


def test_textual_steps_repeat_to_the_bit(L):
    _repeat("textual", 2)


def test_duration_steps_repeat_to_the_bit(L):
    _repeat("duration", 2)


def test_alignment_steps_repeat_to_the_bit(L):
    _repeat("alignment", 2)


def _gate_cases():
    """(id, gate name, arguments behind `env`) for every case of the default mode's parity gates"""
    from tests import test_hip_parity as P
    out = []
    for name, takes_env in (("test_acoustic_train_step_gradients", True),
                            ("test_acoustic_train_step_with_spectrogram_discriminators", True),
                            ("test_textual_train_step_vs_oracle", True), ("test_duration_train_step_vs_oracle", True),
                            ("test_block_backward_vs_float64_oracle", True),
                            ("test_layernorm32_backward_one_thread_per_column_equals_the_general_kernel", True),
                            ("test_mel_style_encoder_backward", False), ("test_acoustic_losses_forward_backward", False)):
        fn = getattr(P, name)
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        if not marks:
            out.append(pytest.param(name, takes_env, (), id=name))
            continue
        for vals in marks[0].args[1]:
            vals = vals if isinstance(vals, (tuple, list)) else (vals,)
            out.append(pytest.param(name, takes_env, tuple(vals), id=f"{name}[{'-'.join(str(v) for v in vals)}]"))
    return out


@pytest.mark.parametrize("name,takes_env,args", _gate_cases())
def test_deterministic_mode_passes_the_default_mode_parity_gates(L, env, monkeypatch, name, takes_env, args):  # noqa: F811
    """the existing gate functions, unchanged, with the switch on: a fixed-order sum is no further from float64 than an atomic one,
    so the project's own tolerances hold verbatim"""
    from tests import test_hip_parity as P
    fn = getattr(P, name)
    L.set_deterministic(True)
    kw = {}
    if "monkeypatch" in fn.__code__.co_varnames[:fn.__code__.co_argcount]:
        kw["monkeypatch"] = monkeypatch
    if name.startswith("test_layernorm32"):
        monkeypatch.setenv("STY_NO_LN32_BWD", "1")  # (the gate deletes the variable for its second half)
    fn(*(((env,) if takes_env else ()) + args), **kw)
    assert L.get_deterministic()


# rows of the table: what the mode converts
TABLE_ROWS = (("LayerNorm weight / bias", lambda k: re.search(r"(_norm\.(weight|bias)|norm_layers.*\.(gamma|beta))$", k) is not None),
              ("Snake alpha", lambda k: "alpha" in k),
              ("GRN gamma", lambda k: k.endswith("grn.gamma")),
              ("text_encoder.emb.weight", lambda k: k == "speech_predictor.text_encoder.emb.weight"),
              ("unshared.weight", lambda k: k == "speech_style_encoder.unshared.weight"))


def test_deterministic_gradients_equal_the_default_mode_up_to_summation_order(L):
    """fp32, train_mode=False, lr = 0, no discriminators, B = 5: one step in each mode from identical state.  The gates are those
    of test_multi_stream_step_equals_single_stream_step for the same kind of difference (one summation order against another,
    d_style among the reordered sums): relative L2 of the concatenated predictor + style-encoder gradient <= 1e-6, losses to
    rtol 1e-6.  The table (profiles/deterministic_table.txt) has one row per converted tensor class."""
    RS = _tool()
    batch = RS.batch_of(B, T, LT, torch.device(DEV))
    res = {}
    for mode in (False, True):
        L.set_deterministic(mode)
        tr = RS.build("acoustic", torch.device(DEV), deterministic=mode, train_mode=False, lr=0.0, adversarial=False)
        seen, sp_backward = {}, tr.sp.backward

        def spy(*a, **kw):  # d loss / d style, as the predictor's backward hands it to the style encoder's
            out = sp_backward(*a, **kw)
            seen["d_style"] = out[0]
            return out

        tr.sp.backward = spy
        losses = tr.train_batch(seed=0, **batch)
        torch.cuda.synchronize()
        g = {f"{key}.{n}": p.grad.detach().cpu().clone() for key, m in RS.models_of("acoustic", tr).items()
             for n, p in m.named_parameters() if p.grad is not None}
        res[mode] = (losses.cpu(), g, seen["d_style"].detach().cpu().clone())
    L.set_deterministic(False)
    (l0, g0, s0), (l1, g1, s1) = res[False], res[True]
    assert g0.keys() == g1.keys()
    rows = []
    for title, pick in TABLE_ROWS:
        ks = [k for k in g0 if pick(k)]
        assert ks, title
        worst = max(((g1[k] - g0[k]).abs().max().item() / max(g0[k].abs().max().item(), 1e-30), k) for k in ks)
        rows.append((title, len(ks), worst[0], worst[1]))
    rows.append(("d_style", 1, (s1 - s0).abs().max().item() / s0.abs().max().item(), "d_style"))
    print("\n  deterministic mode vs default mode, one acoustic step (fp32, eval graph, B 5, T 80, 24 tokens):")
    print("  tensors                      count  max|diff| / max|default|  worst tensor")
    for title, n, e, k in rows:
        print(f"  {title:28s} {n:5d}  {e:10.3e}               {k}")
    a, b = torch.cat([v.flatten() for v in g1.values()]), torch.cat([v.flatten() for v in g0.values()])
    rel = ((a - b).norm() / b.norm()).item()
    print(f"  all gradients ({a.numel()} elements): relative L2 {rel:.3e}; losses {l1.tolist()} / {l0.tolist()}")
    assert rel <= 1e-6
    assert torch.allclose(l1, l0, rtol=1e-6, atol=0)


@pytest.mark.parametrize("Tf", [255, 256, 257, 513, 413, 512, 355])
def test_ln32_parameter_sums_repeat_at_workgroup_edges(L, env, monkeypatch, Tf):  # noqa: F811
    """The vocoder backward that test_layernorm32_backward_one_thread_per_column_equals_the_general_kernel drives, B = 3, in
    mode 1: two calls give equal bits, and the three LayerNorms' dw / db pass that test's gate (2e-5 of the tensor's scale)
    against the general kernel.  The long-row kernel takes a LayerNorm(32) at B x 75T >= 65536 columns: T = 513 (three
    workgroups of frames, 151 of columns per utterance) runs it; at 255 / 256 / 257 frames B x 75T is below that and the general
    pair runs with the mode's [B][C] slots -- both paths must repeat.  413 / 512 / 355 frames put the long-row kernel itself at a
    workgroup edge: 75 T = 30975 = 121 x 256 - 1, 38400 = 150 x 256 and 26625 = 104 x 256 + 1 columns per utterance, B x 75T above
    the threshold in all three."""
    import stylish_tts_amd as S
    from tests.test_hip_parity import rel_err
    L.set_deterministic(True)
    P = {k: v.clone() for k, v in env["P"].items()}
    g = torch.Generator().manual_seed(3)
    mel, style = torch.randn(3, 256, Tf, generator=g), torch.randn(3, 64, generator=g)
    pitch, voiced = torch.rand(3, Tf, generator=g) * 200 + 80, torch.ones(3, Tf)
    noise = torch.randn(3, 300 * Tf, 9, generator=g)

    def run(general):
        if general:
            monkeypatch.setenv("STY_NO_LN32_BWD", "1")
        else:
            monkeypatch.delenv("STY_NO_LN32_BWD", raising=False)
        m = S.SpeechPredictor()
        m.load_state_dict(P, strict=False)
        m = m.to(DEV).enable_training()
        audio = m.vocoder_forward_train(mel=mel.to(DEV), style=style.to(DEV), pitch=pitch.to(DEV), voiced=voiced.to(DEV),
                                        noise=noise.to(DEV))
        m.vocoder_backward(torch.sign(audio) / audio.numel())
        torch.cuda.synchronize()
        return {k: p.grad.cpu().clone() for k, p in m.named_parameters() if p.grad is not None and k.startswith("generator.")}

    a, b, ref = run(False), run(False), run(True)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad[:6]
    ln = [k for k in a if "layer_norm" in k or k.endswith(("phase_norm.weight", "phase_norm.bias"))]
    assert len(ln) >= 6
    for k in ln:
        e = rel_err(a[k], ref[k])
        print(f"\n  T {Tf}: d {k[-44:]:44s} vs the general kernel {e:.2e}", end="")
        assert e <= 2e-5, (k, e)


def _speech_case(RS):
    import stylish_tts_amd as S
    from stylish_tts_amd import manifest as M
    from stylish_tts_amd.acoustic import duration_to_alignment
    from stylish_tts_amd.synthetic_weights import fill_state_dict
    batch = RS.batch_of(B, T, LT, torch.device(DEV))
    g = torch.Generator().manual_seed(9)
    m = S.SpeechPredictor()
    m.load_state_dict(fill_state_dict(M.speech_predictor_manifest(), 0), strict=False)
    m = m.to(DEV).enable_training()
    pitch = batch["pitch"]
    args = (batch["texts"], batch["text_lengths"], duration_to_alignment(batch["durations"], T), pitch,
            torch.randn(B, T, generator=g).to(DEV), (pitch > 20).float(), torch.randn(B, 64, generator=g).to(DEV), pitch)
    return m, args, torch.randn(B, 300 * T, 9, generator=g).to(DEV)


def test_mode_is_latched_by_the_forward(L):
    """sty_speech_fwd_train in mode 1, the switch flipped to 0, sty_speech_bwd: the gradients are those of a run that never
    flipped (the backward runs in the mode its forward ran in)"""
    RS = _tool()
    out = []
    for flip in (False, True):
        L.set_deterministic(True)
        m, args, noise = _speech_case(RS)
        audio = m.forward_train(*args, noise=noise)
        if flip:
            L.set_deterministic(False)
        d_style, d_energy = m.backward(torch.sign(audio) / audio.numel())
        torch.cuda.synchronize()
        out.append(dict({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, d_style=d_style,
                        d_energy=d_energy))
    L.set_deterministic(False)
    assert out[0].keys() == out[1].keys() and len(out[0]) > 100
    bad = [k for k in out[0] if not torch.equal(out[0][k], out[1][k])]
    assert not bad, bad[:6]


def test_small_workspace_is_refused_not_overrun(L):
    """a workspace sized in mode 0 and handed to a mode-1 sty_speech_fwd_train: STY_ENOMEM from the host-side check (mode 1 needs
    the partial slots on top), nothing launched -- the output buffer keeps its fill and no device error is pending; the figures
    of the training entry points follow the mode, and mode 0's is the same after the visit"""
    RS = _tool()
    lib = L.load()
    m, args, noise = _speech_case(RS)
    L.set_deterministic(False)
    audio = m.forward_train(*args, noise=noise)  # (builds the handle; sizes m._train_ws for mode 0)
    m.backward(torch.sign(audio) / audio.numel())
    need0, need1, again = C.c_size_t(), C.c_size_t(), C.c_size_t()
    L.check(lib.sty_speech_train_workspace_bytes(m._handle, B, LT, T, C.byref(need0)))
    L.set_deterministic(True)
    L.check(lib.sty_speech_train_workspace_bytes(m._handle, B, LT, T, C.byref(need1)))
    print(f"\n  sty_speech_train_workspace_bytes(B {B}, L {LT}, T {T}): {need0.value} bytes, deterministic mode {need1.value} "
          f"(+{need1.value - need0.value})")
    assert need1.value > need0.value
    ws = torch.empty(need0.value, dtype=torch.uint8, device=DEV)
    io = L.SpeechIO()
    io.B, io.L, io.T = B, LT, T
    keep = [args[0].to(torch.int64).contiguous(), args[1].to(torch.int64).contiguous()]
    io.texts, io.text_lengths = keep[0].data_ptr(), keep[1].data_ptr()
    for name, t in zip(("alignment", "pitch", "energy", "voiced", "style", "denormal_pitch"), args[2:]):
        t = t.to(torch.float32).contiguous()
        keep.append(t)
        setattr(io, name, t.data_ptr())
    io.noise = noise.data_ptr()
    out = torch.full((B, 1, 300 * T), 7.0, device=DEV)
    io.audio = out.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.sty_speech_fwd_train(m._handle, C.byref(io), C.c_void_p(ws.data_ptr()), ws.numel(), st)
    assert rc == -4, (rc, lib.sty_last_error())  # STY_ENOMEM
    assert b"deterministic" in lib.sty_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    L.set_deterministic(False)
    L.check(lib.sty_speech_train_workspace_bytes(m._handle, B, LT, T, C.byref(again)))
    assert again.value == need0.value
    rc = lib.sty_speech_fwd_train(m._handle, C.byref(io), C.c_void_p(ws.data_ptr()), ws.numel(), st)  # mode 0: it fits
    assert rc == 0, lib.sty_last_error()
    torch.cuda.synchronize()
    assert not bool((out == 7.0).all())


def test_unit_entries_repeat_in_the_deterministic_mode(L):
    """sty_act_bwd (Snake d alpha) and sty_grn_bwd (d gamma) have no room for slots: in mode 1 they run one launch per utterance,
    so the rows' atomic adds meet in stream order.  B = 5, two calls each: equal bits; against the default mode 1e-5 of the tensor's
    largest value (another order of B fp32 additions moves a sum by at most (B - 1) 2^-23 sum_b |term|, and the terms of these
    random inputs add up to no more than a few times the largest result)."""
    lib = L.load()
    g = torch.Generator().manual_seed(2)
    Bn, Cc, Tn = 5, 96, 520
    x, dy = torch.randn(Bn, Cc, Tn, generator=g).to(DEV), torch.randn(Bn, Cc, Tn, generator=g).to(DEV)
    alpha = (torch.rand(Cc, generator=g) + 0.5).to(DEV)
    ds = torch.randn(Bn, Cc, generator=g).to(DEV)
    gamma = torch.randn(Cc, generator=g).to(DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = C.c_size_t()
    L.check(lib.sty_grn_bwd_workspace_bytes(Bn, Cc, Tn, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)

    def run():
        dx, dal = torch.empty_like(x), torch.zeros(Cc, device=DEV)
        L.check(lib.sty_act_bwd(3, Bn, Cc, Tn, L.ptr(x), L.ptr(dy), L.ptr(alpha), None, None, 0, L.ptr(dx), 0, L.ptr(dal), st))
        coef, dg = torch.empty(Bn, Cc, device=DEV), torch.zeros(Cc, device=DEV)
        L.check(lib.sty_grn_bwd(Bn, Cc, Tn, L.ptr(x), L.ptr(ds), L.ptr(gamma), 1, L.ptr(coef), L.ptr(dg), L.ptr(ws), ws.numel(), st))
        torch.cuda.synchronize()
        return dx, dal, coef, dg

    L.set_deterministic(False)
    ref = run()
    L.set_deterministic(True)
    a, b = run(), run()
    for u, v, r in zip(a, b, ref):
        assert torch.equal(u, v)
        assert (u - r).abs().max().item() <= 1e-5 * r.abs().max().item()
