"""What tests/test_ragged_lengths.py (GPU) assumes about the reference arithmetic on ragged text batches, pinned on the CPU
with the oracle alone, so that a later change of the oracle cannot silently void the GPU gates:

  * the fp32 oracle of duration_predictor sits inside HALF of each GPU gate against the float64 oracle (2.5e-5 on `out`,
    2.5e-4 on d_style and on every parameter gradient, of the tensor's maximum);
  * token ids on the padded positions do not matter: variants A (id 0) and B (ids 170..177) give bit-identical outputs and
    gradients; the output on padded positions and the embedding-gradient rows of ids that occur on padding only are exactly 0;
  * one row with a length one too large moves the output, d_style and EVERY parameter gradient by more than 10 x the GPU gate
    (float64 on both sides), so the gates can see an off-by-one in a mask.
"""
import functools

import pytest
import torch

from tests.cases import RAGGED_CASES, RAGGED_PAD_IDS, make_ragged

GATE_OUT, GATE_GRAD = 5e-5, 5e-4  # the gates of the duration predictor's training graph (test_hip_parity.py)
N_GRADS = 195                      # parameters of the duration predictor that receive a gradient
COT_SEED = 6


def rel(a, b):
    """max |a - b| relative to the maximum of the reference tensor b"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


@functools.lru_cache(maxsize=None)
def duration_params(seed=3):
    from oracle.manifest import duration_predictor_manifest
    from oracle.weights import fill_state_dict
    return fill_state_dict(duration_predictor_manifest(), seed)


def duration_cotangent(B, L, NC):
    return torch.randn(B, L, NC, generator=torch.Generator().manual_seed(COT_SEED))


def oracle_duration(P, texts, text_lengths, style, dtype):
    """duration_predictor forward + autograd under the cotangent randn(out.shape) (seed 6) in `dtype`, every floating-point
    parameter a leaf -> (out, d_style, {key: gradient}) as `dtype` tensors; parameters the graph does not reach are left out"""
    from oracle import predictors as OP
    Q = {k: (v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in P.items()}
    st = style.detach().to(dtype).clone().requires_grad_(True)
    out = OP.duration_predictor(Q, texts, text_lengths, st)
    (out * duration_cotangent(*out.shape).to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in Q.items() if v.is_floating_point() and v.grad is not None}
    return out.detach(), st.grad, grads


def off_by_one(text_lengths):
    """the longest row that is shorter than L with a length one too large (row 1: 65 -> 66 in the first case, the negative
    control of the GPU module; a row of length 1 growing to 2 would be the smallest change a batch can see, not a typical one)"""
    t = text_lengths.clone()
    short = torch.where(t < t.max(), t, torch.zeros_like(t))
    t[int(short.argmax())] += 1
    return t


@pytest.mark.parametrize("L,lengths", RAGGED_CASES)
def test_duration_predictor_oracle_on_ragged_batches(L, lengths):
    cs = make_ragged(L, lengths)
    P = duration_params()
    tl, valid = cs["text_lengths"], cs["valid"]
    out_a, ds_a, g_a = oracle_duration(P, cs["texts_a"], tl, cs["style"], torch.float32)
    out_b, ds_b, g_b = oracle_duration(P, cs["texts_b"], tl, cs["style"], torch.float32)
    out64, ds64, g64 = oracle_duration(P, cs["texts_a"], tl, cs["style"], torch.float64)
    assert len(g64) == N_GRADS and g_a.keys() == g64.keys() == g_b.keys()
    # the fp32 reference arithmetic inside half of each GPU gate
    worst = max(g64, key=lambda k: rel(g_a[k], g64[k]))
    print(f"\n  L={L} lengths={lengths}: fp32 vs float64 oracle: out {rel(out_a, out64):.2e}  d_style {rel(ds_a, ds64):.2e}  "
          f"worst gradient {rel(g_a[worst], g64[worst]):.2e} ({worst})")
    assert rel(out_a, out64) <= GATE_OUT / 2
    assert rel(ds_a, ds64) <= GATE_GRAD / 2
    for k in g64:
        assert g64[k].abs().max().item() > 1e-9, f"{k}: structurally zero gradient"
        assert rel(g_a[k], g64[k]) <= GATE_GRAD / 2, (k, rel(g_a[k], g64[k]))
    # padded token ids do not matter, bit for bit
    assert torch.equal(out_a, out_b) and torch.equal(ds_a, ds_b)
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), k
    # exact zeros
    assert (out_a[~valid] == 0).all() and (out64[~valid] == 0).all()
    emb = "text_encoder.emb.weight"
    lo, hi = RAGGED_PAD_IDS
    assert (g_a[emb][lo:hi] == 0).all() and (g_b[emb][lo:hi] == 0).all() and (g_a[emb][0] == 0).all()
    assert g_b[emb][0].abs().max() == 0  # variant B has no id 0 at all
    # sensitivity: one row one token too long, float64 on both sides
    out_o, ds_o, g_o = oracle_duration(P, cs["texts_a"], off_by_one(tl), cs["style"], torch.float64)
    v3 = valid[:, :, None].double()
    moved = {k: rel(g_o[k], g64[k]) for k in g64}
    least = min(moved, key=moved.get)
    print(f"  off by one on the longest padded row: out (valid positions) {rel(out_o * v3, out64):.2e}  d_style {rel(ds_o, ds64):.2e}  "
          f"least moved gradient {moved[least]:.2e} ({least})")
    assert rel(out_o * v3, out64) > 10 * GATE_OUT
    assert rel(ds_o, ds64) > 10 * GATE_GRAD
    for k, e in moved.items():
        assert e > 10 * GATE_GRAD, (k, e)
