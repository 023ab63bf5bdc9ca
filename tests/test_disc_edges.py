"""The discriminators on the device at the layout edges of tests/cases.py (DISC_SPEC_CASES, DISC_WAVE_CASES, DISC_SEQ_CASES),
held to the float64 oracle.

The two-part scheme of tests/disc_checks.py with the network half compared to the oracle in float64 (score maps, d_pred, every
parameter gradient, under the score gradients the fp32 loss oracle computes on the device's own score maps) and the loss half
compared to the float64 sums over the fp32 membership (loss_reference64), at the gates of tests/test_discriminators.py;
tests/test_disc_oracle.py shows that the fp32 oracle itself uses less than half of each.  Exact properties on top: the combined
call equals the two separate calls on the generator side, a batch's score maps equal its rows run alone, the dropped tail of a
waveform gets an exactly zero gradient.  The measured errors are in profiles/disc_edges_table.txt (run with -s to print them).
"""
import pytest
import torch

from tests import disc_checks as dc
from tests.cases import (DISC_SEQ_CASES, DISC_SEQ_TIED, DISC_SPEC_BF16_CASES, DISC_SPEC_CASES, DISC_SPEC_TIED, DISC_WAVE_CASES,
                         disc_seq_inputs, disc_spec_inputs, disc_wave_inputs)

pytestmark = pytest.mark.gpu
F64 = dict(dtype=torch.float64, loss64=True)


def _show(tag, case, rec):
    print(f"\ndevice {tag} {case}: " + "  ".join(f"{k} {v:.2e}" for k, v in rec.items()))


def _ties(m, t, q, dev):
    """per level: (elements of real - gen equal to its median, element count) on the device's score maps"""
    rs, gs = m(t.to(dev))[0], m(q.to(dev))[0]
    return [(int((r - g == torch.median(r - g)).sum()), r.numel()) for r, g in zip(rs, gs)]


@pytest.mark.parametrize("B,H,W", DISC_SPEC_CASES)
def test_spec_discriminator_edges_vs_float64(B, H, W):
    dev = torch.device("cuda:0")
    _, params = dc.spec_fixture()
    m = dc.hip_spec_model(params, dev)
    t, q0 = disc_spec_inputs(B, H, W)
    rec = {}
    gen, disc, d_pred = dc.check_against_oracle(m, params, t, q0, dev, 2e-5, 2e-4, rec=rec, **F64)
    _show("spec", (B, H, W), rec)
    # the combined call equals the two separate calls
    for p in m.parameters():
        p.grad = None
    d2 = torch.zeros(B, H, W, device=dev)
    gen2, _ = m.losses(t.to(dev), q0.to(dev), gen_scale=2.0, d_pred=d2)
    _, disc2 = m.losses(t.to(dev), q0.to(dev), disc_scale=3.0)
    assert torch.equal(gen2, gen) and torch.equal(d2, d_pred)
    assert abs(disc2[0].item() - disc[0].item()) <= 1e-6 * abs(disc[0].item())
    # a batch's score maps equal its rows run alone, bit for bit
    whole = m(q0.to(dev))[0]
    for b in range(B):
        alone = m(q0[b:b + 1].to(dev))[0]
        for i in range(5):
            assert torch.equal(alone[i][0], whole[i][b]), (b, i)


@pytest.mark.parametrize("B,H,W", DISC_SPEC_BF16_CASES)
def test_spec_discriminator_edges_bf16_mode(B, H, W):
    """the gates of test_spec_discriminator_bf16_mode; a misplaced column is an O(1) error and these gates see it"""
    dev = torch.device("cuda:0")
    _, params = dc.spec_fixture()
    m = dc.hip_spec_model(params, dev)
    m.compute_bf16 = True
    t, q0 = disc_spec_inputs(B, H, W)
    rec = {}
    dc.check_against_oracle(m, params, t, q0, dev, 2e-2, 5e-2, rec=rec, **F64)
    _show("spec-bf16", (B, H, W), rec)


@pytest.mark.parametrize("B,N", DISC_WAVE_CASES)
def test_context_free_discriminator_edges_vs_float64(B, N):
    dev = torch.device("cuda:0")
    _, params = dc.cf_fixture()
    t, q0 = disc_wave_inputs(B, N)
    rec = {}
    _, _, d_pred = dc.cf_check(dc.hip_cf_model(params, dev), params, t, q0, dev, 2e-5, 5e-4, rec=rec, **F64)
    _show("wave", (B, N), rec)
    kept = ((N - 1024) // 512) * 512 + 1024
    assert d_pred[:, :kept].abs().max().item() > 0
    assert torch.equal(d_pred[:, kept:], torch.zeros(B, N - kept, device=dev))  # the dropped tail: exactly zero


@pytest.mark.parametrize("name,dim_in,K,B,T", DISC_SEQ_CASES)
def test_pitch_discriminator_edges_vs_float64(name, dim_in, K, B, T):
    dev = torch.device("cuda:0")
    params = dc.seq_params(name, dim_in, K)
    m = dc.hip_seq_model(params, dim_in, K, dev)
    t, q0 = disc_seq_inputs(dim_in, B, T)
    rec = {}
    dc.pd_check(m, params, t, q0, dev, rec=rec, **F64)
    _show("seq", (name, dim_in, K, B, T), rec)


def test_spec_discriminator_tied_median_batch():
    """rows 0 and 1 of pred equal target: exactly 2n/3 ties at the median of every level on the device's own score maps; the loss
    kernels have to divide d rel / d m evenly among them (torch.median's backward).  With the whole of it on the first tied element
    d_pred is off by thousands of gates (tests/test_disc_oracle.py)."""
    dev = torch.device("cuda:0")
    _, params = dc.spec_fixture()
    m = dc.hip_spec_model(params, dev)
    t, q0 = disc_spec_inputs(*DISC_SPEC_TIED, tied=True)
    for ties, n in _ties(m, t, q0, dev):
        assert 3 * ties == 2 * n, (ties, n)
    rec = {}
    dc.check_against_oracle(m, params, t, q0, dev, 2e-5, 2e-4, rec=rec, **F64)
    _show("spec-tied", DISC_SPEC_TIED, rec)


def test_pitch_discriminator_tied_median_batch():
    dev = torch.device("cuda:0")
    name, dim_in, K, B, T = DISC_SEQ_TIED
    params = dc.seq_params(name, dim_in, K)
    m = dc.hip_seq_model(params, dim_in, K, dev)
    t, q0 = disc_seq_inputs(dim_in, B, T, tied=True)
    for ties, n in _ties(m, t, q0, dev):
        assert 3 * ties == 2 * n, (ties, n)
    rec = {}
    dc.pd_check(m, params, t, q0, dev, rec=rec, **F64)
    _show("seq-tied", DISC_SEQ_TIED, rec)
