"""Shared cases of the bf16 operand mode of the slm term (tests/test_slm_bf16.py on the CPU, tests/test_slm_bf16_gpu.py on the
device) and of tools/gen_slm_bf16_golden.py.  Waves, weights and configurations are those of tests/slm_cases.py; the cotangent is
tests/slm_grad_cases.py's.  This file adds the case list of the mode (two of its cases are new: the frame counts 130 and 324 at
full width), where each case's float64 reference lives, and the kernel-level shapes.

The network-level reference is the class itself, twice: in float64 (the truth) and under torch.autocast("cpu", bfloat16) (the
reference's own bf16 mode).  The fixture holds how far the second is from the first (`r_auto`, a relative L2); the device in bf16
mode has to be no further from float64 than that.
"""
import torch

from tests import slm_cases as SC

# name -> (config, N16, B, T, hidden states stored, frame stride of the stored states, sample stride of the stored gradient)
# existing cases keep the float64 tensors of tests/golden/slm_*.safetensors and slm_grad_*.safetensors (strides 1);
# the two new ones store float32 copies of the float64 runs in tests/golden/slm_bf16_*.safetensors, thinned to fit a file
CASES = {
    "small_400": ("small", 400, 2, 1, (0, 1, 2), 1, 1),        # T 1
    "small_7777": ("small", 7777, 2, 24, (0, 1, 2), 1, 1),     # dropped remainders
    "small_22800": ("small", 22800, 2, 71, (0, 1, 2), 1, 1),   # T % 4 != 0
    "full2_8000": ("full2", 8000, 2, 24, (0, 1, 2), 1, 1),     # head dim 64
    "full12_26000": ("full12", 26000, 1, 81, (0, 6, 12), 1, 1),  # depth 12
    "full2_41700": ("full2", 41700, 1, 130, (0, 1, 2), 2, 1),  # two queries past a 128-query workgroup
    "full2_104000": ("full2", 104000, 2, 324, (0, 1, 2), 8, 2),  # the c3 row
}
NEW_CASES = ("full2_41700", "full2_104000")
# where the float64 states / the float64 g_cot of a case live
STATE_FILES = {"small": ("slm_small",), "full2": ("slm_full2",), "full12": ("slm_full12_a", "slm_full12_b")}
GRAD_FILES = {"small_400": "slm_grad_small_a", "small_7777": "slm_grad_small_a", "small_22800": "slm_grad_small_b",
              "full2_8000": "slm_grad_full2", "full12_26000": "slm_grad_full12"}
NEW_FILES = {"full2_41700": ("slm_bf16_full2_41700",), "full2_104000": ("slm_bf16_full2_104000_h", "slm_bf16_full2_104000_g")}
LISTING = "slm_bf16.json"

# ---- kernel level ----
ATTN_T = (24, 33, 130, 324)   # < one 32-key tile; one key past a tile; two queries past a 128-query workgroup; the c3 frame count
ATTN_B, ATTN_H = 2, 3
CONV_KS = ((3, 2), (2, 2))
CONV_CH = ((64, 64), (512, 512))
CONV_NIN = (9, 130, 1039)     # a dropped remainder; one column past a 128-column tile; many tiles with an odd tail
CONV_B = 2


def stack_shape(name):
    cname, _, B, T, _, _, _ = CASES[name]
    cfg = SC.CONFIGS[cname]
    return (cfg.get("num_hidden_layers", 12) + 1, B, T, cfg.get("hidden_size", 768))


def cot(name, dtype=torch.float64):
    """the seeded normal cotangent of the case's hidden-state stack (tests/slm_grad_cases.py's draw)"""
    g = torch.Generator().manual_seed(7001 * SC.SEED + CASES[name][1])
    return torch.randn(stack_shape(name), generator=g, dtype=torch.float64).to(dtype)


def rel_l2(a, ref):
    """|| a - ref || / || ref || in float64"""
    a, ref = a.double(), ref.double()
    return ((a - ref).norm() / ref.norm()).item()


def load_reference(name, golden):
    """(states {i: float64 [B, T', H] on the case's frame stride}, g_cot float64 [B, N'] on its sample stride)"""
    import os

    from safetensors.torch import load_file
    cname = CASES[name][0]
    files = NEW_FILES[name] if name in NEW_CASES else STATE_FILES[cname] + (GRAD_FILES[name],)
    t = {}
    for f in files:
        t.update(load_file(os.path.join(golden, f + ".safetensors")))
    return {i: t[f"{name}.h{i}"].double() for i in CASES[name][4]}, t[f"{name}.g_cot"].double()


def attn_inputs(T, DH, seed=SC.SEED):
    """q, k, v, d_o [B, H DH, T] bf16-representable; gate [B, H, T] and table [H, 2T - 1] plain fp32 (the sizes WavLM's have:
    the gate in (1, 3) around 2, table entries of order 1)"""
    g = torch.Generator().manual_seed(9173 * seed + 131 * T + DH)
    B, H = ATTN_B, ATTN_H
    r = lambda *s: torch.randn(*s, generator=g)
    q, k, v, d_o = (r(B, H * DH, T).bfloat16().float() for _ in range(4))
    gate = 2.0 + 0.5 * torch.tanh(r(B, H, T))
    tab = 0.7 * r(H, 2 * T - 1)
    return q, k, v, gate, tab, d_o


def attn_reference(q, k, v, gate, tab, d_o):
    """float64 softmax attention with the gated relative bias and its autograd: o, dq, dk, dv [B, H DH, T], d_gate [B, H, T]"""
    B, H, T = gate.shape
    DH = q.shape[1] // H
    q, k, v, gate = (x.double().requires_grad_(True) for x in (q, k, v, gate))
    qh, kh, vh = (x.reshape(B, H, DH, T) for x in (q, k, v))
    idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1            # [i, j] -> j - i + T - 1
    bias = gate[..., None] * tab.double()[:, idx][None]                            # [B, H, i, j]
    p = torch.softmax(torch.einsum("bhdi,bhdj->bhij", qh, kh) / DH ** 0.5 + bias, dim=-1)
    o = torch.einsum("bhij,bhdj->bhdi", p, vh).reshape(B, H * DH, T)
    grads = torch.autograd.grad((o * d_o.double()).sum(), (q, k, v, gate))
    return (o.detach(),) + tuple(grads)


def conv_inputs(Cin, Cout, k, s, Nin, seed=SC.SEED):
    """x [B, Cin, Nin] (a pre-activation), w [Cout, Cin, k] bf16-representable, gy [B, Cout, T] bf16-representable"""
    g = torch.Generator().manual_seed(6113 * seed + 17 * Nin + 3 * Cin + k)
    T = (Nin - k) // s + 1
    x = torch.randn(CONV_B, Cin, Nin, generator=g)
    w = (torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5).bfloat16().float()
    gy = torch.randn(CONV_B, Cout, T, generator=g).bfloat16().float()
    return x, w, gy
