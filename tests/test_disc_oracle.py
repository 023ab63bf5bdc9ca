"""What the discriminator gates rest on, on the CPU (tests/cases.py DISC_*_CASES; the device side is tests/test_disc_edges.py).

  * the fp32 oracle (oracle/discriminator.py as the other tests run it) against the SAME code in float64, on every case and under
    the score cotangents the loss helpers produce: it has to sit inside HALF of every gate of tests/test_discriminators.py, so that
    at least half of each gate is left for the device;
  * the fp32 oracle's loss values against the float64-sum reference the device losses are held to (disc_checks.loss_reference64);
  * ties at the median: torch.median's backward divides the gradient evenly among the tied elements; a batch in which two of
    three pred rows equal their target rows has 2n/3 ties at every level, and putting the whole d rel / d m on the first tied
    element instead moves d_pred by thousands of gates (the weight gradients provably not at all: see the test);
  * the lower median is part of the definition: the upper one moves the loss values by many gates.
The measured figures are in profiles/disc_edges_table.txt (run with -s to print them).
"""
import functools

import pytest
import torch

from tests import disc_checks as dc
from tests.cases import (DISC_SEQ_CASES, DISC_SEQ_TIED, DISC_SPEC_BF16_CASES, DISC_SPEC_CASES, DISC_SPEC_TIED, DISC_WAVE_CASES,
                         disc_seq_inputs, disc_spec_inputs, disc_wave_inputs)
from oracle import discriminator as od

CASES = ([("spec", c) for c in DISC_SPEC_CASES + [c for c in DISC_SPEC_BF16_CASES if c not in DISC_SPEC_CASES]]
         + [("wave", c) for c in DISC_WAVE_CASES] + [("seq", c) for c in DISC_SEQ_CASES])
IDS = [f"{f}-" + "-".join(str(x) for x in c) for f, c in CASES]


def case_inputs(family, case, tied=False):
    if family == "spec":
        return dc.spec_fixture()[1], *disc_spec_inputs(*case, tied=tied)
    if family == "wave":
        return dc.cf_fixture()[1], *disc_wave_inputs(*case)
    name, dim_in, K, B, T = case
    return dc.seq_params(name, dim_in, K), *disc_seq_inputs(dim_in, B, T, tied=tied)


@functools.lru_cache(maxsize=None)
def _fp32(family, case):
    """fp32 oracle score maps of a case and the loss oracle's values and cotangents on them (shared, never modified)"""
    params, t, q = case_inputs(family, case)
    with torch.no_grad():
        rs, gs = dc.family_scores(family, params, t), dc.family_scores(family, params, q)
    return params, t, q, rs, gs, dc.loss_cotangents(rs, gs)


@pytest.mark.parametrize("family,case", CASES, ids=IDS)
def test_fp32_oracle_within_half_of_every_gate(family, case):
    """score maps, input gradient and every weight gradient of the fp32 oracle against the float64 oracle, the same injected score
    cotangents on both sides (those of the loss helpers on the fp32 score maps, median term included), the norms and floors of
    the device checks.  Measured over all cases (profiles/disc_edges_table.txt): scores <= 2.6e-6 (half gate 1e-5), d_pred <= 3.5e-6
    and weight gradients <= 6.0e-5 (half gates 1e-4 / 2.5e-4), original0 <= 4.8e-6 (half gate 5e-4)."""
    params, t, q, _, _, (_, _, g_gen, g_dr, g_dg) = _fp32(family, case)
    got = dc.oracle_pass(family, params, t, q, (g_gen, g_dr, g_dg), torch.float32)
    ref = dc.oracle_pass(family, params, t, q, (g_gen, g_dr, g_dg), torch.float64)
    errs = dc.rel_errors(family, got, ref)
    print(f"\nfp32-oracle {family} {case}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 0.5 * dc.gate_of(family, k), (k, v)


@pytest.mark.parametrize("family,case", CASES, ids=IDS)
def test_fp32_loss_values_within_half_of_the_gate(family, case):
    """the fp32 oracle's two loss values against the float64 sums over the fp32 membership (loss_reference64)"""
    _, _, _, rs, gs, (gl, dl, *_) = _fp32(family, case)
    if family == "spec":  # the relativistic term is live at every level (tests/cases.py disc_spec_inputs)
        assert all(rg < od.TAU and rd < od.TAU for _, rg, _, rd in dc.rel_terms(rs, gs))
    g64, d64 = dc.loss_reference64(rs, gs)
    eg, ed = abs(gl.item() - g64) / g64, abs(dl.item() - d64) / d64
    print(f"\nfp32-loss {family} {case}: gen {eg:.2e}  disc {ed:.2e}")
    assert eg <= 0.5 * dc.gate_of(family, "loss") and ed <= 0.5 * dc.gate_of(family, "loss"), (eg, ed)


@pytest.mark.parametrize("B,N", DISC_WAVE_CASES)
def test_wave_cases_stay_clear_of_the_relu_kink(B, N, monkeypatch):
    """The waveform discriminator ends in Conv1d(256, 512, 1) + ReLU + Conv1d(512, 1, 1).  A ReLU unit whose pre-activation lies
    within fp32 rounding of zero passes its gradient or not depending on the rounding, and through the median's spike one such
    unit moves every upstream weight gradient by several 1e-3 of its size (seen on the device with a pre-activation of 3e-7).
    The fp32 oracle's pre-activations differ from the float64 ones by at most 2.2e-6 on these cases; every case keeps all of its
    units at least 5e-6 away from zero in float64."""
    import torch.nn.functional as F
    params, t, q = case_inputs("wave", (B, N))
    p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    seen, relu = [], F.relu
    monkeypatch.setattr(F, "relu", lambda z: (seen.append(z.detach()), relu(z))[1])
    for x in (t, q):
        od.context_free_discriminator(p64, x.double())
    assert len(seen) == 2 and all(h.shape[1] == 512 for h in seen)
    assert min(h.abs().min().item() for h in seen) >= 5e-6


def test_torch_median_backward_splits_evenly_among_ties():
    x = torch.tensor([3., 1., 2., 2., 2., 0., 5., 2.], requires_grad=True)
    torch.median(x).backward()
    assert x.grad.tolist() == [0, 0, 0.25, 0.25, 0.25, 0, 0, 0.25]  # (not 1 on the first 2)
    y = torch.tensor([0.0, -0.0, 1.0, -1.0, 0.0], requires_grad=True)  # -0.0 == +0.0 ties
    torch.median(y).backward()
    assert torch.equal(y.grad, torch.tensor([1., 1., 0., 0., 1.]) / 3)


def _end_to_end(family, params, t, q0, median):
    """(d gen / d pred, {key: d disc / d parameter}) of the fp32 oracle with the given median rule"""
    keys = dc.grad_keys(family, params)
    q = q0.clone().requires_grad_(True)
    pp = {k: (v.clone().requires_grad_(True) if k in keys else v) for k, v in params.items()}
    rs, gs = dc.family_scores(family, pp, t), dc.family_scores(family, pp, q)
    gen, disc = dc.loss_helpers(rs, gs, median)
    dq, = torch.autograd.grad(gen, q, retain_graph=True)
    return dq, dict(zip(keys, torch.autograd.grad(disc, [pp[k] for k in keys])))


@pytest.mark.parametrize("family,case", [("spec", DISC_SPEC_TIED), ("spec", (3, 5, 33)), ("seq", DISC_SEQ_TIED)],
                         ids=["spec-3-9-25", "spec-3-5-33", "seq-dur-64"])
def test_tied_median_batch_separates_the_even_split_from_the_first_element_rule(family, case):
    """Two of three pred rows equal their target rows: ties = 2n/3 at every level, the relativistic term live at every level for
    both helpers, and the first-element rule moves d_pred by >= 100 gates (measured 3000 .. 4800).
    The WEIGHT gradients cannot tell the two rules apart on such a batch, and on no batch whose ties come from equal inputs: a tied
    element is r_i - g_i with r_i and g_i the same function of the parameters (same weights, same input row), so d (r_i - g_i) /
    d theta = 0 and whatever share of d rel / d m the element receives is multiplied by zero.  Asserted here as what it is: the
    two rules' weight gradients agree to rounding (measured 2e-3 of a gate).  The rule reaches the weights only through ties of
    unequal inputs, which no entry point can construct."""
    params, t, q = case_inputs(family, case, tied=True)
    with torch.no_grad():
        rs, gs = dc.family_scores(family, params, t), dc.family_scores(family, params, q)
    for lvl, (r, g, (tg, relg, td, reld)) in enumerate(zip(rs, gs, dc.rel_terms(rs, gs))):
        assert 3 * tg == 2 * r.numel() and 3 * td == 2 * r.numel(), (lvl, tg, td, r.numel())
        assert relg < od.TAU and reld < od.TAU, (lvl, relg, reld)  # the gradient of the relativistic term is live
    # the variant helpers with torch.median are the oracle's helpers
    gen, disc = dc.loss_helpers(rs, gs)
    assert gen.item() == od.generator_loss_helper(rs, gs).item() and disc.item() == od.discriminator_loss_helper(rs, gs).item()
    dq_e, dw_e = _end_to_end(family, params, t, q, dc.median_even)
    dq_f, dw_f = _end_to_end(family, params, t, q, dc.median_first)
    move_x = (dq_f - dq_e).abs().max().item() / dq_e.abs().max().item() / dc.gate_of(family, "d_pred")
    move_w = max((dw_f[k] - v).abs().max().item() / max(v.abs().max().item(), 1e-3)
                 / dc.gate_of(family, "grad.original0" if k.endswith("original0") else "grad") for k, v in dw_e.items())
    print(f"\ntied {family} {case}: first-element rule moves d_pred by {move_x:.0f} gates, the worst weight gradient by {move_w:.0f} gates")
    assert move_x >= 100, move_x
    assert move_w <= 0.1, move_w


@pytest.mark.parametrize("family", ["spec", "wave", "seq"])
def test_upper_median_moves_the_losses_by_many_gates(family):
    """torch.median is the LOWER median; at an even element count the upper one is another number.  Per case: the relative move
    of both loss values; at least one case per family moves one of them by >= 10 gates."""
    worst = 0.0
    for f, case in CASES:
        if f != family:
            continue
        _, _, _, rs, gs, _ = _fp32(f, case)
        if all(r.numel() % 2 for r in rs):
            continue
        lo, up = dc.loss_helpers(rs, gs), dc.loss_helpers(rs, gs, dc.median_upper)
        mg, md = abs(up[0].item() - lo[0].item()) / lo[0].item(), abs(up[1].item() - lo[1].item()) / lo[1].item()
        print(f"\nupper-median {f} {case}: gen {mg:.2e}  disc {md:.2e}  ({mg / dc.gate_of(f, 'loss'):.0f} / {md / dc.gate_of(f, 'loss'):.0f} gates)")
        worst = max(worst, mg / dc.gate_of(f, "loss"), md / dc.gate_of(f, "loss"))
    assert worst >= 10, worst


def test_case_tables_reach_the_kernels_their_comments_name():
    """fp32 mode: every conv and input-gradient conv of every case runs the tiled kernel (flat-image mode for the spectrogram
    discriminator); bf16 mode: only (4, 45, 25) reaches convp16_kernel's flat-image mode, at level 1."""
    for family, case in CASES:
        for name, fwd, bwd in dc.conv_routes(family, case):
            assert fwd in (None, "tiled") and bwd == "tiled", (family, case, name, fwd, bwd)
    for case in DISC_SPEC_BF16_CASES:
        routes = dc.conv_routes("spec", case, bf16=True)
        want = {"level 1"} if case == (4, 45, 25) else set()
        assert {n for n, fwd, bwd in routes if fwd == "convp16"} == want, (case, routes)
        assert {n for n, fwd, bwd in routes if bwd == "convp16"} == want, (case, routes)
        assert all(fwd in (None, "tiled", "convp16") for _, fwd, _ in routes), (case, routes)
