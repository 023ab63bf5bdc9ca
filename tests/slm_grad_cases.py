"""Shared cases of the slm gradient tests (tests/test_slm_grad.py on the CPU, tests/test_slm_grad_gpu.py on the device) and of
tools/gen_slm_grad_golden.py.  The waves, weights and configurations are those of tests/slm_cases.py; this file adds what a
gradient needs: the seeded cotangent of a hidden-state stack (regenerated on both sides, never stored), the bit-packing of the
float64 run's L1 signs, the 24 kHz end-to-end waves, and the fixture layout.
"""
import torch

from tests import slm_cases as SC

# case -> (fixture file, gradients stored).  g_cot: d/d wave1 of sum(h(wave1) * cot) / numel -- the smooth pin; e_cot: the same
# gradient at the encoder's input (the tap); g_l1: d/d wave1 of mean |h(wave0) - h(wave1)|, with the float64 run's signs beside it
CASES = {
    "small_400": ("slm_grad_small_a", ("g_cot", "e_cot", "g_l1")),
    "small_5200": ("slm_grad_small_a", ("g_cot", "e_cot", "g_l1")),
    "small_7777": ("slm_grad_small_a", ("g_cot", "e_cot", "g_l1")),
    "small_22800": ("slm_grad_small_b", ("g_cot", "e_cot", "g_l1")),
    "small_104000": ("slm_grad_small_c", ("g_cot",)),   # 832 KB: a file of its own
    "full2_8000": ("slm_grad_full2", ("g_cot", "g_l1")),
    "full12_26000": ("slm_grad_full12", ("g_cot", "g_l1")),
}
FILES = ("slm_grad_small_a", "slm_grad_small_b", "slm_grad_small_c", "slm_grad_full2", "slm_grad_full12", "slm_grad_e2e")
# the cases whose L1 signs the device may form itself: min |h0 - h1| > 2 x the forward gate (asserted by the generator), so no
# sign can flip while both stacks are inside their gates
OWN_SIGN_CASES = ("small_400", "small_5200", "small_7777")
# end to end at 24 kHz: SC.resample in float64 composed with the float64 small model, autograd through both; B = 2
E2E_N = (7800, 11666)
# The end-to-end test lets the device form the L1 signs, so its waves must keep every |h0 - h1| above twice the forward gate, as
# OWN_SIGN_CASES do.  The smallest of 6 144 (9 216) differences is a matter of chance: of eight draws of the prediction's noise,
# scanned on the float64 reference alone, these are the ones with the widest margin (1.1e-4 against 7.8e-5, 2.0e-4 against 8.0e-5);
# the generator asserts the condition.
E2E_DRAW = {7800: 7, 11666: 0}
E2E_CONFIG = "small"


def stack_shape(name):
    cname, _, B, T, _ = SC.CASES[name]
    cfg = SC.CONFIGS[cname]
    return (cfg.get("num_hidden_layers", 12) + 1, B, T, cfg.get("hidden_size", 768))


def cot(name, dtype=torch.float64):
    """the seeded normal cotangent of the case's hidden-state stack"""
    g = torch.Generator().manual_seed(7001 * SC.SEED + SC.CASES[name][1])
    return torch.randn(stack_shape(name), generator=g, dtype=torch.float64).to(dtype)


def pack_signs(sign):
    """a tensor of +-1 (no zero) -> uint8, eight per byte, little bit first, zero-padded"""
    bits = (sign.reshape(-1) > 0).to(torch.uint8)
    pad = (-bits.numel()) % 8
    bits = torch.cat([bits, bits.new_zeros(pad)]).reshape(-1, 8)
    return (bits << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8)


def unpack_signs(packed, shape, dtype=torch.float32):
    n = 1
    for s in shape:
        n *= s
    bits = (packed[:, None] >> torch.arange(8, dtype=torch.uint8)) & 1
    return (bits.reshape(-1)[:n].to(dtype) * 2 - 1).reshape(shape)


def e2e_waves(N, B=2):
    """(ground truth, prediction) [B, N] at 24 kHz: the resampler tests' wave, and the same plus a third of another draw"""
    gt = SC.resample_input(N, B)
    g = torch.Generator().manual_seed(4111 * SC.SEED + N + 1000003 * E2E_DRAW[N])
    return gt, (gt.double() + 0.1 * torch.randn(B, N, generator=g, dtype=torch.float64)).float()


def grad_gate(gmax, gown):
    """SC.forward_gate on a gradient: max(1e-5 max|g64|, 4 x max|g32 - g64|)"""
    return SC.forward_gate(gmax, gown)
