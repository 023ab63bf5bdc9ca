"""The bf16 operand mode of the slm term on the device (sty_wavlm_set_compute; csrc/wavlm.hip, csrc/attn16.hip, the plan in
csrc/plan_wavlm.hip; stylish_tts_amd/slm.py).  Reads tests/golden only; imports neither transformers nor the reference.

Two levels.

Kernel level, sharp.  The attention with the gated relative bias (sty_attention_rel_fwd_bwd) against float64 softmax attention and
its autograd on bf16-representable q, k, v, d_o: the bf16 kernels within 1e-2 of each tensor's scale, the fp32 kernels on the same
inputs within 1e-4, the two outputs not bit-equal (the bounds of test_attention_bf16_mode_vs_float64_on_rounded_operands).  One
strided feature conv (sty_wavlm_strided_conv_fwd_bwd), forward and input gradient, against float64 on the same bf16-rounded
operands at 2e-5 of the output scale (the bound of the block-level bf16 tests, tests/test_small_column_convs.py), the staged twin
bit-equal to torch's .bfloat16() of the fp32 view.

Network level, against the reference alone (tests/golden/slm_bf16.json, tools/gen_slm_bf16_golden.py): the device in bf16 mode is
no further from the class's float64 run than the class's own bf16 mode (torch.autocast) is -- relative L2 of every stored hidden
state and of the g_cot gradient <= r_auto, no margin: the device rounds operands only, autocast also rounds every output.
The network gate catches gross wiring errors only: on the float64 reference alone, removing the position bias moves the last state
by 0.23-0.36 (seen), gru_rel_pos_const = 1 by 1.5-1.8e-2 (borderline), one conv weight x (1 + 2^-6) by 7e-3 to 1e-2 (not seen).
The kernel-level tests above carry the precision.

Every parity test prints its line before it asserts; profiles/slm_bf16_parity_table.txt keeps them.
"""
import ctypes as C
import functools
import json
import os

import pytest
import torch

from stylish_tts_amd import lib as L
from stylish_tts_amd import slm
from tests import slm_bf16_cases as BC
from tests import slm_cases as SC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
SWITCHES = ("STY_NO_CONVSC", "STY_CONVSC_MAX_COLS", "STY_CONVK1_MIN_TILES", "STY_CONVP16_MIN_TILES", "STY_NO_CONVK1", "STY_NO_CONVP16",
            "STY_CONVQ_MIN_TILES")
K_K1, K_Q, K_P16, K_TILED = 3, 4, 5, 6  # STY_CONV_* of include/stylish_hip.h
F_X16 = 128                             # STY_ROUTE_X16


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def listing():
    return json.load(open(os.path.join(GOLDEN, BC.LISTING)))["cases"]


@functools.lru_cache(maxsize=None)
def reference(name):
    return BC.load_reference(name, GOLDEN)


@functools.lru_cache(maxsize=None)
def model(cname):
    m = slm.WavLM(**SC.CONFIGS[cname])
    m.load_state_dict(SC.wavlm_weights(SC.CONFIGS[cname]), strict=True)
    return m.to(DEV).eval()


def _scale_err(got, ref):
    ref = ref.double()
    return (got.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------
def _attention(lib, T, DH, bf16, t):
    B, H = BC.ATTN_B, BC.ATTN_H
    need = C.c_size_t()
    L.check(lib.sty_attention_workspace_bytes(B, H, T, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    d = [x.to(DEV).contiguous() for x in t]
    o, dq, dk, dv = (torch.empty(B, H * DH, T, device=DEV) for _ in range(4))
    dg = torch.full((B, H, T), float("nan"), device=DEV)  # written, not accumulated: no NaN may survive
    L.check(lib.sty_attention_rel_fwd_bwd(B, H, DH, T, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]), L.ptr(d[5]),
                                          L.ptr(o), L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(dg), int(bf16), L.ptr(ws), ws.numel(),
                                          _stream()))
    torch.cuda.synchronize()
    return dict(o=o.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu(), d_gate=dg.cpu())


@pytest.mark.parametrize("T", BC.ATTN_T)
def test_attention_with_the_gated_bias_vs_float64_on_rounded_operands(T):
    lib = L.load()
    t = BC.attn_inputs(T, 64)
    ref = dict(zip(("o", "dq", "dk", "dv", "d_gate"), BC.attn_reference(*t)))
    res = {mode: _attention(lib, T, 64, mode == "bf16", t) for mode in ("fp32", "bf16")}
    bad = []
    for k in ref:
        e32, e16 = _scale_err(res["fp32"][k], ref[k]), _scale_err(res["bf16"][k], ref[k])
        print(f"slm_bf16 attention T={T} {k}: scale {ref[k].abs().max().item():.3e}  fp32 kernels {e32:.3e} (1e-4)  "
              f"bf16 kernels {e16:.3e} (1e-2)")
        if not (e32 <= 1e-4 and e16 <= 1e-2 and torch.isfinite(res["bf16"][k]).all() and torch.isfinite(res["fp32"][k]).all()):
            bad.append(k)
    assert not bad, bad
    assert not torch.equal(res["fp32"]["o"], res["bf16"]["o"])  # the bf16 kernels really ran
    again = _attention(lib, T, 64, True, t)
    assert all(torch.equal(again[k], res["bf16"][k]) for k in ref)  # no atomic: two calls, the same bits


def test_attention_with_the_gated_bias_head_dim_16_reaches_the_fp32_kernels():
    lib = L.load()
    T = 33
    t = BC.attn_inputs(T, 16)
    ref = dict(zip(("o", "dq", "dk", "dv", "d_gate"), BC.attn_reference(*t)))
    res = _attention(lib, T, 16, False, t)
    for k in ref:
        e = _scale_err(res[k], ref[k])
        print(f"slm_bf16 attention DH=16 T={T} {k}: fp32 kernels {e:.3e} (1e-4)")
        assert e <= 1e-4, k
    d = [x.to(DEV) for x in t]
    o = torch.empty(BC.ATTN_B, BC.ATTN_H * 16, T, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    rc = lib.sty_attention_rel_fwd_bwd(BC.ATTN_B, BC.ATTN_H, 16, T, *(L.ptr(x) for x in d), L.ptr(o), L.ptr(o), L.ptr(o), L.ptr(o), L.ptr(o), 1,
                                       L.ptr(ws), ws.numel(), _stream())
    assert rc == -1 and b"head dim 16" in lib.sty_last_error()  # bf16 mode: head dim 64 alone; refused on the host


def _unview(view, Cin, s, Nin):
    """[B, s Cin, Tp] phase-major -> [B, Cin, s Tp][:Nin]: x[c][s t + p] = view[p Cin + c][t]"""
    B, _, Tp = view.shape
    x = view.reshape(B, s, Cin, Tp).permute(0, 2, 3, 1).reshape(B, Cin, Tp * s)[:, :, :Nin]
    return torch.nn.functional.pad(x, (0, Nin - x.shape[-1]))  # (a dropped remainder may lie past the view: no frame reads it)


@pytest.mark.parametrize("Nin", BC.CONV_NIN)
@pytest.mark.parametrize("ch", BC.CONV_CH, ids=lambda c: "ci%d-co%d" % c)
@pytest.mark.parametrize("ks", BC.CONV_KS, ids=lambda c: "k%d-s%d" % c)
def test_strided_feature_conv_on_the_bf16_twin_vs_float64(ks, ch, Nin, monkeypatch):
    lib = L.load()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("STY_CONVP16_MIN_TILES", "1")  # (the block parity tests' way to run a family on a small shape)
    (k, s), (Cin, Cout), B = ks, ch, BC.CONV_B
    x, w, gy = BC.conv_inputs(Cin, Cout, k, s, Nin)
    T = (Nin - k) // s + 1
    Tp = T + (k + s - 1) // s - 1
    need = C.c_size_t()
    L.check(lib.sty_wavlm_strided_conv_workspace_bytes(B, Cin, Cout, k, s, Nin, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    dx_, dw_, dg_ = x.to(DEV), w.to(DEV), gy.to(DEV)
    y = torch.empty(B, Cout, T, device=DEV)
    dx = torch.full((B, Cin, Nin), float("nan"), device=DEV)
    view = torch.empty(B, s * Cin, Tp, device=DEV)
    view16 = torch.empty(B, s * Cin, Tp, dtype=torch.bfloat16, device=DEV)
    routes = (C.c_int * 4)()
    L.check(lib.sty_wavlm_strided_conv_fwd_bwd(B, Cin, Cout, k, s, Nin, L.ptr(dx_), L.ptr(dw_), 1, L.ptr(y), L.ptr(dg_), L.ptr(dx),
                                               L.ptr(view), L.ptr(view16), routes, L.ptr(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert routes[0] in (K_P16, K_Q) and routes[2] == 1, list(routes)       # the conv read the twin on a twin family
    assert routes[1] in (K_P16, K_Q, K_K1) and (routes[3] == 1 or k == s), list(routes)
    # the twin the stage writes is torch's rounding of the fp32 view, bit for bit; the fp32 view is GELU(x), phase-major
    assert torch.equal(view16.view(torch.int16), view.bfloat16().view(torch.int16))
    gelu64 = torch.nn.functional.gelu(x.double())
    got_x = _unview(view.cpu(), Cin, s, Nin)
    ev = (got_x.double() - gelu64)[:, :, :min(Nin, Tp * s)].abs().max().item()
    # fp32 GELU = 0.5 x (1 + erf(x / sqrt 2)): erf's few ulp and three roundings -- eight half-ulps of the largest value
    vgate = 8 * 2.0 ** -24 * gelu64.abs().max().item()
    print(f"slm_bf16 strided conv k{k} s{s} {Cin}->{Cout} Nin={Nin}: fp32 view vs float64 GELU {ev:.3e} (gate {vgate:.3e})")
    assert ev <= vgate and (view.cpu().reshape(B, s, Cin, Tp).permute(0, 2, 3, 1).reshape(B, Cin, -1)[:, :, Nin:] == 0).all()
    # forward: float64 conv on the operands the device multiplied (the twin, the bf16-representable weight)
    op = _unview(view16.float().cpu(), Cin, s, Nin).double()
    ref = torch.nn.functional.conv1d(op, w.double(), stride=s)
    ey = (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    # input gradient: the transposed conv of the bf16-representable gy in float64, times GELU'(x)
    xg = x.double().requires_grad_(True)
    lin = torch.nn.functional.conv_transpose1d(gy.double(), w.double(), stride=s)
    lin = torch.nn.functional.pad(lin, (0, Nin - lin.shape[-1]))
    torch.nn.functional.gelu(xg).backward(lin)
    refg = xg.grad
    eg = (dx.double().cpu() - refg).abs().max().item() / refg.abs().max().item()
    print(f"slm_bf16 strided conv k{k} s{s} {Cin}->{Cout} Nin={Nin}: routes {list(routes)}  forward {ey:.3e}  input gradient {eg:.3e}  "
          f"(2e-5 of scale {ref.abs().max().item():.2f} / {refg.abs().max().item():.2f})")
    assert ey <= 2e-5 and eg <= 2e-5
    tail = Nin - ((T - 1) * s + k)  # samples no frame reads
    assert tail >= 0 and (tail == 0 or (dx[:, :, Nin - tail:] == 0).all()) and torch.isfinite(dx).all()


# ---------------------------------------------------------------------------------------------------------------------------
# network level
# ---------------------------------------------------------------------------------------------------------------------------
def _dense_convs(cfg_name, n16):
    """(Cin, Cout, K, T, flags) of every dense conv of the plan at n16 samples in bf16 mode, the strided ones in the form the
    plan offers them to the twin families (a same-length conv over the padded view of the bf16 twin)"""
    from stylish_tts_amd.manifest import WAVLM_DEFAULT_CFG
    c = {**WAVLM_DEFAULT_CFG, **SC.CONFIGS[cfg_name]}
    out, n, cin = [], n16, 1
    for i, (dim, k, s) in enumerate(zip(c["conv_dim"], c["conv_kernel"], c["conv_stride"])):
        n = (n - k) // s + 1
        if i:
            K = (k + s - 1) // s
            out.append((s * cin, dim, K, n + K - 1, F_X16))
            out.append((dim, s * cin, K, n + K - 1, F_X16 if i < len(c["conv_dim"]) - 1 else 0))  # its transposed conv
        cin = dim
    H, FF = c["hidden_size"], c["intermediate_size"]
    out += [(cin, H, 1, n, 0), (H, cin, 1, n, 0), (H, H, 1, n, 0), (H, FF, 1, n, 0), (FF, H, 1, n, 0)]
    Cg = H // c["num_conv_pos_embedding_groups"]
    out.append((Cg, Cg, c["num_conv_pos_embeddings"], n, 0))
    return out


def _route(lib, B, Ci, Co, K, T, flags):
    k = C.c_int(-2)
    L.check(lib.sty_conv1d_route(B, Ci, Co, K, 1, T, 1, flags, C.byref(k)))
    return k.value


@pytest.mark.parametrize("name", list(BC.CASES))
def test_network_in_bf16_mode_is_no_further_from_float64_than_autocast(name, monkeypatch):
    cname, n16, B, T, keep, fstride, sstride = BC.CASES[name]
    rec = listing()[name]
    states, g64 = reference(name)
    lib = L.load()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if name == "full2_104000":
        # the c3 row: B = 2 here, B = 32 in the step.  With the families' thresholds lowered every dense conv takes the family it
        # takes at B 32 without them (the routes are asked for both)
        convs = _dense_convs(cname, n16)
        at32 = [_route(lib, 32, *c) for c in convs]
        monkeypatch.setenv("STY_CONVP16_MIN_TILES", "1")
        monkeypatch.setenv("STY_CONVK1_MIN_TILES", "1")
        here = [_route(lib, B, *c) for c in convs]
        print(f"slm_bf16 routes {name}: " + " ".join(f"{c[0]}>{c[1]}k{c[2]}T{c[3]}:{r}" for c, r in zip(convs, here)))
        assert here == at32, list(zip(convs, at32, here))
        strided = [r for c, r in zip(convs, here) if c[4] == F_X16 and c[2] > 1]
        assert strided and all(r == K_P16 for r in strided)  # the dominant family reads twins on the persistent bf16 kernel
    m = model(cname)
    x0, x1 = SC.wave(n16, B, 0).to(DEV), SC.wave(n16, B, 1).to(DEV)
    cot = BC.cot(name, torch.float32).to(DEV)
    m.set_compute("bf16")
    try:
        L.prof_report(64)
        lib.sty_prof_enable(1)
        try:
            with torch.no_grad():
                h0 = m(x0)
                h1 = m.forward_keep(x1)
                g = m.backward(cot / h1.numel())
        finally:
            lib.sty_prof_enable(0)
        fams = sorted(r["name"] for r in L.prof_report(64))
        with torch.no_grad():
            value = slm.l1_mean(h0, h1).item()
    finally:
        m.set_compute("fp32")
    torch.cuda.synchronize()
    assert h0.shape == BC.stack_shape(name) and torch.isfinite(h0).all() and torch.isfinite(g).all()
    bad = []
    for i in keep:
        r = BC.rel_l2(h0[i, :, ::fstride].cpu(), states[i])
        print(f"slm_bf16 network {name} state {i}: device-to-f64 {r:.3e}  autocast-to-f64 (gate) {rec[f'r_auto.h{i}']:.3e}  "
              f"operand-rounding emulation {rec[f'r_emul.h{i}']:.3e}")
        if not r <= rec[f"r_auto.h{i}"]:
            bad.append(f"h{i}")
    r = BC.rel_l2(g[:, ::sstride].cpu(), g64)
    print(f"slm_bf16 network {name} g_cot: device-to-f64 {r:.3e}  autocast-to-f64 (gate) {rec['r_auto.g_cot']:.3e}")
    if not r <= rec["r_auto.g_cot"]:
        bad.append("g_cot")
    bound = 2 * rec["r_auto.stack"] * rec["rms.stack"]
    print(f"slm_bf16 network {name} loss: device {value:.6f}  float64 {rec['loss']:.6f}  |diff| {abs(value - rec['loss']):.3e} "
          f"(rel {abs(value - rec['loss']) / rec['loss']:.1e}; autocast rel {abs(rec['loss_auto'] - rec['loss']) / rec['loss']:.1e})  "
          f"bound {bound:.3e}")
    if not abs(value - rec["loss"]) <= bound:
        bad.append("loss")
    print(f"slm_bf16 families {name}: " + " ".join(fams))
    assert not bad, bad
    if n16 == 7777:  # remainders dropped at several strides: no frame reads the last two samples
        assert (g[:, -2:] == 0).all() and (g[:, -3] != 0).all()
    if cname != "small":  # (widths from 512 up: no dense conv is left on fp32 operands)
        assert not [f for f in fams if f.startswith("conv1d_mfma_kernel") and f.endswith("false>")], fams
        assert any(f.startswith("attn16_") for f in fams), fams
    if name == "full2_104000":
        assert any(f.startswith("convp16_kernel") for f in fams) and any(f.startswith("wavlm_stage_rs_kernel<16>") for f in fams)


def test_the_mode_really_ran_and_fp32_mode_keeps_its_bits():
    cfg = SC.CONFIGS["full2"]
    m = slm.WavLM(**cfg)
    m.load_state_dict(SC.wavlm_weights(cfg), strict=True)
    m = m.to(DEV).eval()
    x = SC.wave(8000, 2, 1).to(DEV)
    with torch.no_grad():
        before = m(x)                      # the mode was never switched on this object
        kept = m.forward_keep(x)
        assert m.set_compute("bf16").compute == "bf16"
        b16 = m(x)
        b16k = m.forward_keep(x)
        m.set_compute("fp32")
        after = m(x)
    assert torch.equal(before, kept) and torch.equal(before, after)
    assert not torch.equal(before, b16)
    # keep mode in bf16: the same operands through the same kernels on the dense side
    r = BC.rel_l2(b16k.cpu(), b16.cpu())
    print(f"slm_bf16 mode: bf16 stack vs fp32 stack {BC.rel_l2(b16.cpu(), before.cpu()):.3e}; bf16 forward_keep vs forward {r:.3e}")
    assert r <= listing()["full2_8000"]["r_auto.stack"]


def test_backward_in_another_mode_than_its_forward_is_refused():
    m = model("small")
    lib = L.load()
    x = SC.wave(5200, 2, 1).to(DEV)
    with torch.no_grad():
        h = m.forward_keep(x)
        m.set_compute("bf16")
        try:
            with pytest.raises(L.StyError, match="kept in fp32 mode"):
                m.backward(torch.zeros_like(h))
        finally:
            m.set_compute("fp32")
    assert lib.sty_wavlm_set_compute(m._handle, 2) == -1 and lib.sty_wavlm_set_compute(m._handle, 0) == 0
    # the workspace queries answer for the current mode
    a, b = C.c_size_t(), C.c_size_t()
    L.check(lib.sty_wavlm_grad_workspace_bytes(m._handle, 2, 22800, C.byref(a)))
    L.check(lib.sty_wavlm_set_compute(m._handle, 1))
    L.check(lib.sty_wavlm_grad_workspace_bytes(m._handle, 2, 22800, C.byref(b)))
    L.check(lib.sty_wavlm_set_compute(m._handle, 0))
    assert b.value >= a.value
    torch.cuda.synchronize()


def _snapshot(tmp_path, cfg=None):
    from safetensors.torch import save_file
    cfg = SC.SMALL if cfg is None else cfg
    snap = tmp_path / "wavlm"
    snap.mkdir()
    json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, open(snap / "config.json", "w"))
    save_file(SC.wavlm_weights(cfg), str(snap / "model.safetensors"))
    return snap


def test_loss_and_grad_repeats_to_the_bit_and_rows_are_independent(tmp_path):
    crit = slm.WavLMLoss(str(_snapshot(tmp_path, SC.FULL2)), 16000, 16000, compute="bf16").to(DEV)
    r_auto = listing()["full2_8000"]
    gt, pred = SC.wave(8000, 3, 0).to(DEV), SC.wave(8000, 3, 1).to(DEV)
    v1, g1 = crit.loss_and_grad(gt, pred)
    v2, g2 = crit.loss_and_grad(gt, pred)
    assert torch.equal(g1, g2) and v1.item() == v2.item()
    assert crit.wavlm.compute == "bf16"
    with torch.no_grad():
        assert crit(gt, pred).item() == v1.item()                       # forward(): the bits of loss_and_grad's value
        v32, g32 = crit.loss_and_grad(gt, pred, compute="fp32")         # per-call override
        assert crit(gt, pred, compute="fp32").item() == v32.item() and v32.item() != v1.item()
        h3 = crit.hidden_states(pred)
        cot = torch.randn(h3.shape, generator=torch.Generator().manual_seed(SC.SEED)).to(DEV)
        n1 = h3[:, :1].numel()
        crit.wavlm.forward_keep(pred)
        gc3 = crit.wavlm.backward(cot / n1)
    # Rows of a B = 3 call against their B = 1 calls.  The two take other kernels (tile shapes, split reductions), so their fp32
    # sums differ in the last bits, and every later rounding to bf16 turns some of those into whole bf16 steps: the rows are two
    # evaluations of the mode, not one.  Held: the stack and the gradient of a smooth cotangent, each within the autocast figure
    # of its kind.  The L1 gradient with the device's own signs is printed only: a sign that flips between the two evaluations
    # moves an element of the cotangent by 2 / n, which no figure taken on a smooth cotangent bounds.
    worst_h = worst_g = worst_l1 = 0.0
    for b in range(3):
        with torch.no_grad():
            hb = crit.hidden_states(pred[b:b + 1])
            crit.wavlm.forward_keep(pred[b:b + 1])
            gcb = crit.wavlm.backward(cot[:, b:b + 1].contiguous() / n1)
        _, gb = crit.loss_and_grad(gt[b:b + 1], pred[b:b + 1])
        worst_h = max(worst_h, BC.rel_l2(h3[:, b:b + 1].cpu(), hb.cpu()))
        worst_g = max(worst_g, BC.rel_l2(gc3[b:b + 1].cpu(), gcb.cpu()))
        worst_l1 = max(worst_l1, BC.rel_l2(3 * g1[b:b + 1].cpu(), gb.cpu()))  # (the mean's 1 / n differs by the factor 3)
    print(f"slm_bf16 batch independence: B=3 rows vs B=1, stack {worst_h:.3e} (gate {r_auto['r_auto.stack']:.3e})  "
          f"cotangent gradient {worst_g:.3e} (gate {r_auto['r_auto.g_cot']:.3e})  L1 gradient, own signs {worst_l1:.3e} (no gate)")
    assert worst_h <= r_auto["r_auto.stack"] and worst_g <= r_auto["r_auto.g_cot"]


# ---------------------------------------------------------------------------------------------------------------------------
# trainer and command
# ---------------------------------------------------------------------------------------------------------------------------
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


def test_trainer_and_command_with_the_term_on_bf16_operands(tmp_path):
    """one deterministic acoustic step on the sample dataset with the term on fp32 and on bf16 operands, from the same weights
    and seed; then --validate-only on one checkpoint with and without slm_bf16"""
    import sys
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
    snap = _snapshot(tmp_path)

    def run(name, **kw):
        logs = []
        torch.manual_seed(SC.SEED)
        ctx = T.train(str(cfg), str(mdl), str(tmp_path / name), "acoustic", max_steps=1, deterministic=True, log=logs.append,
                      slm_path=str(snap), slm_train=True, **kw)
        torch.cuda.synchronize()
        return ctx, logs, _checkpoint_tensors(os.path.join(str(tmp_path / name), "acoustic", "checkpoint_final"))

    try:
        c32, logs32, p32 = run("fp32")
        c16, logs16, p16a = run("bf16_a", slm_bf16=True)
        assert any("on bf16 operands" in ln for ln in logs16) and any("on fp32 operands" in ln for ln in logs32)
        t32, t16 = c32.stage.trainer, c16.stage.trainer
        assert (t32.slm_compute, t16.slm_compute) == ("fp32", "bf16")
        v32, v16 = float(t32.slm_value), float(t16.slm_value)
        # the loss bound of the network test with the small cases' figures: 2 x r_auto(stack) x rms(stack), the largest of them
        small = [r for n, r in listing().items() if r["config"] == "small"]
        bound = max(2 * r["r_auto.stack"] * r["rms.stack"] for r in small)
        print(f"slm_bf16 trainer: slm value fp32 {v32:.6f}  bf16 {v16:.6f}  |diff| {abs(v32 - v16):.3e}  bound {bound:.3e}")
        assert torch.isfinite(torch.tensor(v16)) and abs(v16 - v32) <= bound and v16 != v32
        step = lambda logs: [ln for ln in logs if ln.startswith("acoustic epoch")][-1]
        assert step(logs16).endswith(f", slm {v16:.4f}") and step(logs32).endswith(f", slm {v32:.4f}")
        assert step(logs16).rsplit(", slm ", 1)[0] == step(logs32).rsplit(", slm ", 1)[0]  # every other logged term: the same bits
        assert torch.equal(t16.audio, t32.audio)
        moved = [k for k in p32 if not torch.equal(p32[k], p16a[k])]
        assert moved, "the operand mode of the term did not reach the step"
        _, _, p16b = run("bf16_b", slm_bf16=True)
        assert p16a.keys() == p16b.keys() and not [k for k in p16a if not torch.equal(p16a[k], p16b[k])]
        # the object that trained on bf16 operands gives the fp32 validation value: the bits of a fresh fp32 object
        gt, pred = SC.wave(7777, 2, 0).to(DEV).repeat(1, 2)[:, :12000], SC.wave(7777, 2, 1).to(DEV).repeat(1, 2)[:, :12000]
        with torch.no_grad():
            own = slm.WavLMLoss(str(snap), 24000, 16000).to(DEV)
            assert c16.slm.wavlm.compute == "bf16"
            assert float(c16.slm(gt, pred)) == float(own(gt, pred))
    finally:
        L.set_deterministic(False)
    final = os.path.join(str(tmp_path / "fp32"), "acoustic", "checkpoint_final")
    va = T.train(str(cfg), str(mdl), str(tmp_path / "va"), "acoustic", checkpoint=final, validate_only=True, log=lambda s: None,
                 slm_path=str(snap), slm_train=True)
    vb = T.train(str(cfg), str(mdl), str(tmp_path / "vb"), "acoustic", checkpoint=final, validate_only=True, log=lambda s: None,
                 slm_path=str(snap), slm_train=True, slm_bf16=True)
    torch.cuda.synchronize()
    assert va.validation["slm"] == vb.validation["slm"] and va.validation["metrics"] == vb.validation["metrics"]
