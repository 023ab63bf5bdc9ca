"""What tests/test_optim_edges.py (GPU) assumes about the reference arithmetic of the optimizer side, pinned on the CPU on exactly
the inputs of the GPU module (tests/optim_cases.py):

  * the AdamW reference is torch.optim.AdamW in float64; the gates of the GPU module are derived from ONE thing, the distance of
    the same torch.optim.AdamW in float32 from it, per case family: twice the worst value measured here, rounded up to one digit,
    and the fp32 run is held inside half of each gate.  The factor of two: adamw_kernel has torch's operation order but contracts
    m + w1 (g - m) and v b2 + w2 g g into FMAs, which can only move a last bit.  No gate comes from a HIP run.  The scaled entry
    point's p gate is derived by the same rule at the scaled rate (GATE_SCALED_P says why the family's cannot hold below 1);
  * fp32(1 - lr wd) rounded apart and fused is one float at regime (b) and two at b-contract: what the bit-equality test can see;
  * the gates can see a wrong kernel: every float64 restatement with one mistake (optim_cases.WRONG_VARIANTS) lands at least 10 x
    outside the gate of the case named here, while the restatement without a mistake IS the oracle;
  * the rate multiplier: the plain-Python restatement of train/losses.py:238-249 and the package's host
    DiscriminatorLossHelper.get_disc_lr_multiplier both reproduce tests/golden/disc_lr_small.json (recorded from the reference's
    helper) with `==` on doubles;
  * the optimizer's C entry points refuse bad arguments on the host, before anything could be launched.
"""
import ctypes as C
import math

import pytest

from tests.optim_cases import (ADAMW_REGIME_CASES, ADAMW_SCALED_CASES, ADAMW_SCALED_MULTS, ADAMW_SIZE_NAMES, DISC_LR_POINTS, DISC_LR_SEQUENCE, DISC_LR_SUB_COUNTS, FAMILIES,
                               WRONG_VARIANTS, adamw_cases, contract_case, decay_roundings, disc_lr_fixture, distances, helper_constants, oracle64,
                               restated_multiplier, restated_sequence, torch_adamw, wrong_adamw)

import torch

ALL_CASES = ADAMW_SIZE_NAMES + ADAMW_REGIME_CASES
# family -> (GATE_P, GATE_M, GATE_V): 2 x FP32_WORST, rounded up to one digit.  FP32_WORST: torch.optim.AdamW in float32 against
# float64, the metric of optim_cases.distances, worst case of the family, as test_fp32_anchor_sits_inside_half_of_every_gate measures
# and prints it (profiles/optim_edges_table.txt has every case)
FP32_WORST = {
    "size": (1.084e-4, 1.046e-7, 1.481e-7),
    "a": (4.787e-5, 7.397e-8, 1.392e-7),
    "b": (5.589e-7, 7.122e-8, 7.916e-8),
    "c": (4.695e-5, 6.822e-8, 1.277e-7),
    "d": (4.501e-5, 4.382e-8, 9.283e-8),
    "e": (5.344e-7, 1.015e-7, 1.160e-7),
    "f": (3.645e-7, 8.915e-8, 5.989e-8),
}
GATES = {
    "size": (3e-4, 3e-7, 3e-7),
    "a": (1e-4, 2e-7, 3e-7),
    "b": (2e-6, 2e-7, 2e-7),
    "c": (1e-4, 2e-7, 3e-7),
    "d": (1e-4, 9e-8, 2e-7),
    "e": (2e-6, 3e-7, 3e-7),
    "f": (8e-7, 2e-7, 2e-7),
}
# The scaled entry point at lr_d x multiplier.  m and v do not depend on the rate: their gates are the family's.  p does: its
# metric divides by the movement, which shrinks with the rate while the fp32 rounding of p (0.05 randn) stays, so at multiplier
# 0.01 torch.optim.AdamW in float32 itself sits at 2.7e-3 (regime a) and 1.2e-4 (regime b), 27 and 58 times the family's GATE_P.  The
# p gate of a scaled case is therefore derived by the same rule at the same rate -- twice torch's own float32 distance at
# lr_d x multiplier, rounded up to one digit -- which at multiplier 1 IS the family's gate and above 1 is tighter than it.
FP32_SCALED_P = {
    "a-reference": (2.651e-3, 2.650e-4, 4.787e-5, 2.606e-5, 3.330e-5),
    "b-decay": (1.157e-4, 3.469e-6, 5.589e-7, 3.699e-7, 1.933e-7),
}
GATE_SCALED_P = {
    "a-reference": (6e-3, 6e-4, 1e-4, 6e-5, 7e-5),
    "b-decay": (3e-4, 7e-6, 2e-6, 8e-7, 4e-7),
}
# the case (and tensor) at which each wrong variant is required to land >= 10 x outside the gate
WRONG_SEEN_AT = {
    "l2_weight_decay": ("b-decay", "m"),
    "eps_inside_bias_correction": ("c-eps", "p"),
    "betas_swapped": ("a-reference", "m"),
    "grad_scale_not_squared": ("e-gscale1/3", "v"),
    "bias_correction_t_minus_1": ("f-step2", "p"),
}
SENS = 10


def round_up_one_digit(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


def gate_of(name):
    return GATES[adamw_cases()[name]["family"]]


def scaled_gates(name, mult):
    """(GATE_P at lr_d x mult, the family's GATE_M, the family's GATE_V)"""
    return (GATE_SCALED_P[name][ADAMW_SCALED_MULTS.index(mult)],) + gate_of(name)[1:]


def test_gates_are_twice_the_fp32_anchor_rounded_up():
    assert set(GATES) == set(FP32_WORST) == set(FAMILIES)
    for fam in FAMILIES:
        for worst, gate in zip(FP32_WORST[fam], GATES[fam]):
            assert gate == pytest.approx(round_up_one_digit(2 * worst), rel=1e-9), (fam, worst, gate)
    for name in ADAMW_SCALED_CASES:
        for worst, gate in zip(FP32_SCALED_P[name], GATE_SCALED_P[name]):
            assert gate == pytest.approx(round_up_one_digit(2 * worst), rel=1e-9), (name, worst, gate)
        assert scaled_gates(name, 1.0) == gate_of(name)


@pytest.mark.parametrize("fam", FAMILIES)
def test_fp32_anchor_sits_inside_half_of_every_gate(fam):
    """torch.optim.AdamW in float32 against itself in float64, per case; the family's worst is FP32_WORST (to the digits written
    there) and sits inside half of the gate."""
    names = [n for n in ALL_CASES if adamw_cases()[n]["family"] == fam]
    assert names
    worst = [0.0, 0.0, 0.0]
    print()
    for name in names:
        case = adamw_cases()[name]
        e = distances(case, torch_adamw(case, torch.float32), oracle64(name))
        print(f"  {name:16s} fp32 torch vs float64 torch: p {e[0]:.2e}  m {e[1]:.2e}  v {e[2]:.2e}")
        worst = [max(a, b) for a, b in zip(worst, e)]
    print(f"  family {fam}: worst p {worst[0]:.3e}  m {worst[1]:.3e}  v {worst[2]:.3e}   gates {GATES[fam]}")
    for w, rec, gate in zip(worst, FP32_WORST[fam], GATES[fam]):
        assert w <= gate / 2
        assert rec / 2 <= w <= gate / 2, (w, rec)  # the recorded figure is what is measured, up to how a CPU's torch rounds lerp / addcdiv


@pytest.mark.parametrize("name", ADAMW_SCALED_CASES)
def test_fp32_anchor_at_the_scaled_rates(name):
    """torch.optim.AdamW in float32 against float64, both at lr_d x multiplier: m and v as at multiplier 1 (they never see the
    rate), p inside half of GATE_SCALED_P -- and, at the multipliers below 1, OUTSIDE the family's own GATE_P, which is why the
    scaled cases carry a p gate of their own."""
    case = adamw_cases()[name]
    print()
    for i, mult in enumerate(ADAMW_SCALED_MULTS):
        lr = case["hp"]["lr"] * mult
        e = distances(case, torch_adamw(case, torch.float32, lr), oracle64(name, lr))
        gates = scaled_gates(name, mult)
        print(f"  {name} x {mult!r:20}: fp32 torch vs float64 torch p {e[0]:.3e}  m {e[1]:.2e}  v {e[2]:.2e}   gate p {gates[0]:.0e}")
        assert all(a <= g / 2 for a, g in zip(e, gates)) and e[0] >= FP32_SCALED_P[name][i] / 2
        if mult < 1:
            assert e[0] > gate_of(name)[0]


def test_decay_rounded_apart_and_fused_differ_only_at_the_contract_case():
    """What the bit-equality test of the GPU module can and cannot see: at regime (b) fp32(1 - lr wd) is one value however it is
    rounded, at all five multipliers; at b-contract, multiplier 4, a fused multiply-subtract gives the neighbouring float."""
    f32 = lambda x: torch.tensor(x, dtype=torch.float64).float().item()
    hp = adamw_cases()["b-decay"]["hp"]
    for mult in ADAMW_SCALED_MULTS:
        apart, fused = decay_roundings(f32(hp["lr"] * mult), f32(hp["wd"]))
        assert apart == fused and 1 - apart > 1000 * 2.0 ** -24 * mult
    name, mult = contract_case()
    hp = adamw_cases()[name]["hp"]
    assert f32(hp["wd"]) == hp["wd"] and abs(hp["wd"] - 0.1) < 1e-5 and hp["lr"] == 1e-2
    apart, fused = decay_roundings(f32(hp["lr"] * mult), hp["wd"])
    assert abs(apart - fused) == 2.0 ** -24


def test_restatement_without_a_mistake_is_the_oracle():
    for name in ADAMW_REGIME_CASES + ADAMW_SIZE_NAMES[:8]:
        e = distances(adamw_cases()[name], wrong_adamw(name, None), oracle64(name))
        assert max(e) <= 1e-12, (name, e)


@pytest.mark.parametrize("variant", sorted(WRONG_VARIANTS))
def test_every_wrong_variant_lands_outside_a_gate(variant):
    name, tensor = WRONG_SEEN_AT[variant]
    e = dict(zip("pmv", distances(adamw_cases()[name], wrong_adamw(name, variant), oracle64(name))))
    gate = dict(zip("pmv", gate_of(name)))
    print(f"\n  {variant} ({WRONG_VARIANTS[variant]}) at {name}: " +
          "  ".join(f"{k} {e[k]:.2e} ({e[k] / gate[k]:.0f} x gate)" for k in "pmv"))
    assert e[tensor] >= SENS * gate[tensor], (variant, name, tensor, e[tensor], gate[tensor])


@pytest.mark.parametrize("sub_count", DISC_LR_SUB_COUNTS)
def test_multiplier_restatements_reproduce_the_fixture_exactly(sub_count):
    """`==` on doubles: the restatement of optim_cases and the package's host helper against what the reference's helper returned"""
    from stylish_tts_amd.discriminators import DiscriminatorLossHelper
    fx = disc_lr_fixture()
    assert fx["constants"][str(sub_count)] == helper_constants(sub_count)
    helper = DiscriminatorLossHelper(None, sub_count)
    assert {k: getattr(helper, k) for k in helper_constants(sub_count)} == helper_constants(sub_count)
    assert helper.last_loss == helper.ideal_loss
    rows = fx["points"][str(sub_count)]
    assert [r[0] for r in rows] == DISC_LR_POINTS[sub_count]
    branches = set()
    for last, want in rows:
        got, branch = restated_multiplier(last, sub_count)
        helper.last_loss = last
        assert got == want and helper.get_disc_lr_multiplier() == want, (last, got, helper.get_disc_lr_multiplier(), want)
        branches.add(branch)
    assert branches == {"f_max", "h_min", "above", "below"}
    c = helper_constants(sub_count)
    assert restated_multiplier(c["ideal_loss"], sub_count) == (1.0, "below")


@pytest.mark.parametrize("sub_count", DISC_LR_SUB_COUNTS)
def test_host_helper_follows_the_restated_sequence(sub_count):
    """get_disc_lr_multiplier() then track(), the order of train/stage.py, on DISC_LR_SEQUENCE: the same doubles as the restatement"""
    from stylish_tts_amd.discriminators import DiscriminatorLossHelper
    seq = DISC_LR_SEQUENCE[sub_count]
    assert seq.dtype == torch.float32 and seq.shape == (200,)
    mults, branches, means = restated_sequence(seq, sub_count)
    assert set(branches) == {"f_max", "h_min", "above", "below"}
    helper = DiscriminatorLossHelper(None, sub_count)
    for i in range(200):
        assert helper.get_disc_lr_multiplier() == mults[i]
        helper.track((None, seq[i]))
        assert helper.last_loss == means[i]


def test_optimizer_entries_refuse_bad_arguments_on_the_host():
    """sty_adamw_step / sty_adamw_step_scaled: a null buffer, a buffer off the 16-byte grid, step < 1 and (scaled) no multiplier;
    sty_disc_lr_track: no state, an empty band.  All refused with sty_last_error set before anything could be launched (no device
    here; the pointers are never dereferenced); n == 0 is nothing to do and returns OK."""
    import __graft_entry__ as ge
    ge.build()
    from stylish_tts_amd import lib as L
    lib = L.load()
    fake, odd = C.c_void_p(4096), C.c_void_p(4096 + 4)
    hp = (0.85, 0.99, 1e-9, 1e-4)

    def plain(n, p, g, m, v, step):
        return lib.sty_adamw_step(n, p, g, m, v, 1e-4, *hp, step, 1.0, None)

    def scaled(n, p, g, m, v, mult, step):
        return lib.sty_adamw_step_scaled(n, p, g, m, v, 1e-4, mult, *hp, step, 1.0, None)

    for step in (0, -1):
        assert plain(8, fake, fake, fake, fake, step) != 0 and b"sty_adamw_step:" in lib.sty_last_error()
        assert scaled(8, fake, fake, fake, fake, fake, step) != 0 and b"sty_adamw_step_scaled" in lib.sty_last_error()
    assert scaled(8, fake, fake, fake, fake, None, 1) != 0 and b"no multiplier" in lib.sty_last_error()
    for k in range(4):
        null = [None if i == k else fake for i in range(4)]
        bent = [odd if i == k else fake for i in range(4)]
        assert plain(8, *null, 1) != 0 and plain(8, *bent, 1) != 0 and b"unaligned" in lib.sty_last_error()
        assert scaled(8, *null, fake, 1) != 0 and scaled(8, *bent, fake, 1) != 0
        assert plain(0, *bent, 1) != 0  # the arguments are checked before n
    assert plain(0, fake, fake, fake, fake, 1) == 0
    assert scaled(0, fake, fake, fake, fake, fake, 1) == 0
    assert lib.sty_disc_lr_track(None, None, 2.5, 4.0, 0.01, 0.25, 0.25, None) != 0 and b"null state" in lib.sty_last_error()
    assert lib.sty_disc_lr_track(fake, None, 2.5, 4.0, 0.01, 0.0, 0.25, None) != 0 and b"empty band" in lib.sty_last_error()
    assert lib.sty_disc_lr_track(fake, None, 2.5, 4.0, 0.01, 0.25, 0.0, None) != 0
    assert lib.sty_disc_lr_track(fake, None, 2.5, 4.0, 0.01, -0.25, 0.25, None) != 0
