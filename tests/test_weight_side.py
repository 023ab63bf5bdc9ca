"""The weight side's device tables across a second finalize of the same handle (csrc/weights.hip, WeightTables).

A model that is bound, finalized and run for inference, and then has training enabled on the SAME handle, is finalized
again: its tables are freed and rebuilt, now with the gradient un-pack jobs.  One forward_train + backward of such a model
must give what a model gives that went straight to training.  The model that went straight to training runs twice (two
fresh handles): that repeat is the control for the float-atomic sums of the training graph.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _duration():
    """plain, weight-norm, w2a and input-gradient tables"""
    import stylish_tts_amd as S
    from oracle.manifest import duration_predictor_manifest
    from oracle.weights import fill_state_dict
    P = fill_state_dict(duration_predictor_manifest(), 0)
    g = torch.Generator().manual_seed(11)
    probe = S.DurationPredictor()
    texts = torch.randint(1, probe.cfg["tokens"], (2, 7), generator=g)
    lengths = torch.tensor([7, 4])
    style = torch.randn(2, probe.cfg["style_dim"], generator=g)
    cot = torch.randn(2, 7, probe.cfg["dp_classes"], generator=g)
    args = (texts.to(DEV), lengths.to(DEV), style.to(DEV))

    def make():
        m = S.DurationPredictor()
        m.load_state_dict(P)
        return m.to(DEV)

    def train(m):
        out = m.forward_train(*args)
        m.backward(cot.to(DEV))  # (its return value, d loss / d style, is an input gradient: it never passes the weight side)
        return {"out": out}

    return make, (lambda m: m(*args)), train


def _style():
    """both spectral-norm tables and the 2-D input-gradient pack"""
    import stylish_tts_amd as S
    from oracle.manifest import style_encoder_manifest
    from oracle.weights import fill_state_dict
    P = fill_state_dict(style_encoder_manifest(), 0)
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(2, 1, 80, 62, generator=g) * 0.8 - 0.3).to(DEV)
    cot = torch.randn(2, 64, generator=g).to(DEV)

    def make():
        m = S.MelStyleEncoder()
        m.load_state_dict(P, strict=False)
        return m.to(DEV)

    def train(m):
        out = m.forward_train(x)
        m.backward(cot)
        return {"out": out}

    return make, (lambda m: m(x)), train


def _train_leg(m, train):
    """one forward_train + backward at default train options -> (outputs, parameter gradients), on the host"""
    m.enable_training()
    outs = train(m)
    torch.cuda.synchronize()
    outs = {k: v.detach().cpu().clone() for k, v in outs.items()}
    grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
    return outs, grads


@pytest.mark.parametrize("case", ["duration_predictor", "mel_style_encoder"])
def test_tables_rebuilt_by_a_second_finalize(case):
    make, infer, train = {"duration_predictor": _duration, "mel_style_encoder": _style}[case]()
    fresh = [_train_leg(make(), train) for _ in range(2)]

    m = make()
    m._ensure(torch.device(DEV))  # bind + finalize: an inference model
    handle = m._handle.value
    m.prepare()
    with torch.no_grad():
        y = infer(m)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    staged = _train_leg(m, train)  # bind_grad on the same handle: the second finalize frees and rebuilds the tables
    assert m._handle.value == handle, "the module made a new handle instead of finalizing the old one again"

    # the control first: the two fresh runs agree to the bit on at least three quarters of the gradient tensors
    names = sorted(fresh[0][1])
    exact = [k for k in names if torch.equal(fresh[0][1][k], fresh[1][1][k])]
    print(f"\n{case}: {len(exact)} of {len(names)} gradient tensors are bit-identical between two fresh runs")
    assert 4 * len(exact) >= 3 * len(names), "control: the fresh runs themselves differ on more than a quarter of the gradients"

    bad = []
    for part in (0, 1):  # outputs, gradients
        for k in sorted(fresh[0][part]):
            a, b, t = fresh[0][part][k], fresh[1][part][k], staged[part][k]
            if torch.equal(a, b):
                ok = torch.equal(t, a)
                spread = 0.0
            else:  # a float-atomic sum: no further from the fresh runs than they are from each other
                spread = (a - b).abs().max().item()
                ok = max((t - a).abs().max().item(), (t - b).abs().max().item()) <= spread
                print(f"  {k}: fresh runs differ by {spread:.3e}; re-finalized model: {(t - a).abs().max().item():.3e}, "
                      f"{(t - b).abs().max().item():.3e}")
            if not ok or not bool(torch.isfinite(t).all()):
                bad.append((k, spread, (t - a).abs().max().item()))
    assert not bad, f"re-finalized model differs from the fresh one (name, control spread, difference): {bad[:8]}"
