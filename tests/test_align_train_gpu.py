"""The alignment stage's training path on the device: the CTC loss kernel against torch's CPU ctc_loss in float64, the
TextAligner's training graph against the float64 restatement with autograd (tests/align_train_cases.py), the trainer, and the
`train_align` command end to end into `align`.  Every parity gate is measured on its case -- max(1e-5 max|ref64|, 4 x the fp32
CPU run's own distance from float64) -- every parity test prints scale, own distance, device distance and gate
(profiles/align_train_parity_table.txt) and carries a negative control that must exceed the gate."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
from safetensors.torch import load_file

from tests import align_cases as AC
from tests import align_train_cases as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def line(what, scale, own, err, gate, extra=""):
    print(f"\n  align_train_parity {what}: max|ref| {scale:.4e}  cpu fp32-to-f64 {own:.3e}  device-to-f64 {err:.3e}  "
          f"gate {gate:.3e}{extra}")


def device_ctc(lp32, targets, il, tl, blank=TC.BLANK, **kw):
    from stylish_tts_amd.alignment import ctc_loss
    out = ctc_loss(lp32.to(DEV), targets, il, tl, blank, **kw)
    torch.cuda.synchronize()
    return out


# ---- the CTC kernel ------------------------------------------------------------------------------------------------
_CTC_REF = {}


def ctc_refs(i):
    """the case and its float64 / fp32 CPU references, computed once"""
    if i not in _CTC_REF:
        logits, targets, il, tl, priors = TC.ctc_case(i)
        ref = {}
        for name, pri in (("plain", None), ("priors", priors)):
            ref[name] = (TC.ctc_from_logits(logits, targets, il, tl, torch.float64, log_priors=pri),
                         TC.ctc_from_logits(logits, targets, il, tl, torch.float32, log_priors=pri))
        _CTC_REF[i] = (logits, targets, il, tl, priors, ref)
    return _CTC_REF[i]


@pytest.mark.parametrize("priors", [False, True], ids=["plain", "priors"])
@pytest.mark.parametrize("case", range(len(TC.CTC_CASES)), ids=[f"T{c[0]}" for c in TC.CTC_CASES])
def test_ctc_loss_vs_torch_float64(case, priors):
    """nll to 1e-9 relative against torch's float64 ctc_loss on the very log-probs the device reads; loss and d loss / d logits
    against autograd of ctc(log_softmax(logits)) in float64 under the measured gate; exact zeros at and beyond a row's
    length.  Controls: target lengths one short, and blank = 0.
    With priors the scores log_probs - 0.3 priors are not normalised, and torch's ctc_loss backward assumes they are; the
    loss and nll references stay torch's, the gradient's reference is autograd through the written-out float64 recurrence
    (align_train_cases.ctc_nll_recurrence, which tests/test_align_train.py holds to torch on the normalised cases and to a
    finite difference with priors)."""
    logits, targets, il, tl, pri, ref = ctc_refs(case)
    (loss64, _, g64), (loss32, _, g32) = ref["priors" if priors else "plain"]
    assert bool(torch.isfinite(g64).all()) and math.isfinite(float(loss64))
    lp32 = torch.log_softmax(logits, dim=-1)
    kw = dict(log_priors=pri.to(DEV)) if priors else {}
    loss, nll, d = device_ctc(lp32, targets, il, tl, **kw)
    T = logits.shape[1]
    assert d.shape == (3, TC.V1, T) and nll.dtype == torch.float64
    # the same double recurrence on the same fp32 inputs: only the order of the sums differs
    lp_in = lp32.double() - (TC.PRIOR_SCALE * pri.double() if priors else 0.0)
    _, nll64 = TC.ctc_reference(lp_in, targets, il, tl)
    rel = ((nll.cpu() - nll64).abs() / nll64.abs().clamp(min=1.0)).max().item()
    got = d.cpu().transpose(1, 2)
    g_gate, g_scale, g_own = TC.gate(g64, g32)
    l_gate, l_scale, l_own = TC.gate(loss64.reshape(1), loss32.reshape(1))
    g_err, l_err = TC.dist(got, g64), TC.dist(loss, loss64.reshape(1))
    # controls
    _, _, d_short = device_ctc(lp32, targets, il, (tl - 1).clamp(min=0), **kw)
    _, _, d_blank = device_ctc(lp32, targets, il, tl, blank=0, **kw)
    c_short, c_blank = TC.dist(d_short.cpu().transpose(1, 2), g64), TC.dist(d_blank.cpu().transpose(1, 2), g64)
    tag = f"ctc T={T} {'priors' if priors else 'plain'}"
    line(tag + " d_logits", g_scale, g_own, g_err, g_gate, f"  (lengths one short {c_short:.3e}, blank 0 {c_blank:.3e})")
    line(tag + " loss", l_scale, l_own, l_err, l_gate, f"  (nll rel {rel:.2e})")
    assert rel <= 1e-9
    assert l_err <= l_gate and g_err <= g_gate
    assert c_short > g_gate and c_blank > g_gate, "a wrong target length / blank must turn the gate red"
    for b in range(3):
        assert bool((d[b, :, int(il[b]):] == 0).all())


def test_ctc_row_does_not_depend_on_the_batch():
    """row 1 alone equals row 1 in the batch, bit for bit (gradient scale aside: weight / (B U) is a power-of-two factor here)"""
    for case in (3, 4):
        logits, targets, il, tl, pri, _ = ctc_refs(case)
        lp32 = torch.log_softmax(logits, dim=-1)
        _, nll, d = device_ctc(lp32, targets, il, tl, weight=3.0)  # batch of 3, weight 3: the factor is 1 / U
        _, nll1, d1 = device_ctc(lp32[1:2], targets[1:2], il[1:2], tl[1:2], weight=1.0)
        assert torch.equal(nll[1:2], nll1)
        assert torch.equal(d[1:2], d1)
        _, nll_b, d_b = device_ctc(lp32, targets, il, tl, weight=3.0)
        assert torch.equal(nll, nll_b) and torch.equal(d, d_b), "two runs of the same batch differ"


def test_ctc_refuses_rows_without_faulting():
    """The wrapper's checks bypassed (check=False).  T = 4: a healthy row; U = 3 with one repeat at 4 frames (tight: one
    path, status 0) and at 3 frames (no valid path: status 1); a target equal to the blank and a length above T (status 2).
    Refused rows: nll = +inf, zero gradient; the healthy rows equal the batch without the refused ones bit for bit."""
    from stylish_tts_amd.lib import StyError
    g = torch.Generator().manual_seed(4)
    lp32 = torch.log_softmax(3 * torch.randn(5, 4, TC.V1, generator=g), dim=-1)
    targets = torch.tensor([[3, 4, 5], [7, 7, 9], [7, 7, 9], [3, TC.BLANK, 5], [3, 4, 5]])
    il, tl = torch.tensor([4, 4, 3, 4, 5]), torch.tensor([3, 3, 3, 3, 3])
    loss, nll, d, status = device_ctc(lp32, targets, il, tl, check=False, weight=5.0)
    assert status.cpu().tolist() == [0, 0, 1, 2, 2]
    assert math.isinf(float(loss)) and float(loss) > 0
    assert bool(torch.isinf(nll[2:]).all()) and bool((d[2:] == 0).all())
    _, nll2, d2, st2 = device_ctc(lp32[:2], targets[:2], il[:2], tl[:2], check=False, weight=2.0)
    assert st2.cpu().tolist() == [0, 0] and torch.equal(nll[:2], nll2) and torch.equal(d[:2], d2)
    _, nll64 = TC.ctc_reference(lp32[:2].double(), targets[:2], il[:2], tl[:2])
    assert ((nll[:2].cpu() - nll64).abs() / nll64).max().item() <= 1e-9
    with pytest.raises(StyError, match=r"row\(s\) \[3, 4\]"):
        device_ctc(lp32, targets, il, tl)


# ---- the training graph --------------------------------------------------------------------------------------------
def trainable(hidden, P):
    from stylish_tts_amd.alignment import TrainableTextAligner
    m = TrainableTextAligner(AC.N_MELS, AC.TOKENS, hidden_dim=hidden)
    m.load_state_dict(P, strict=True)
    return m.to(DEV).enable_training()


def device_step(m, mel, lengths, targets, tl, drop_p, seed):
    """forward_train + ctc_loss + backward into zeroed .grad -> the quantities of TC.graph_reference, by key"""
    from stylish_tts_amd.alignment import ctc_loss
    for p in m.parameters():
        if p.grad is not None:
            p.grad.zero_()
    lp = m.forward_train(mel.to(DEV), lengths.to(DEV), drop_p, seed)
    loss, _, d = ctc_loss(lp, targets, lengths, tl, TC.BLANK)
    m.backward(d)
    torch.cuda.synchronize()
    out = {"log_probs": lp.cpu(), "loss": loss.cpu()}
    sd = m.state_dict()
    out.update({k: v.cpu() for k, v in sd.items() if "running_" in k})
    out.update({"grad." + k: p.grad.cpu().clone() for k, p in m.named_parameters()})
    return out


def check_graph(tag, got, r64, r32, c64, control_skip=()):
    worst_ratio, worst_control = 0.0, float("inf")
    for k in sorted(r64):
        if k == "loss":
            continue
        g, scale, own = TC.gate(r64[k], r32[k])
        err, ctl = TC.dist(got[k], r64[k]), TC.dist(c64[k], r64[k])
        line(f"{tag} {k}", scale, own, err, g, f"  (control {ctl:.3e})")
        worst_ratio = max(worst_ratio, err / g)
        if k not in control_skip:
            worst_control = min(worst_control, ctl / g)
    print(f"  align_train_parity {tag}: worst device distance {worst_ratio:.3f} gates, nearest control {worst_control:.3g} gates")
    for k in sorted(r64):
        if k == "loss":
            continue
        g, _, _ = TC.gate(r64[k], r32[k])
        assert TC.dist(got[k], r64[k]) <= g, k
        if k not in control_skip:
            assert TC.dist(c64[k], r64[k]) > g, f"{k}: the control must turn the gate red"


@pytest.mark.parametrize("hidden,T", [(80, 9), (80, 34), (80, 66), (640, 34)])
def test_training_graph_vs_float64_autograd(hidden, T):
    """dropout off: log_probs, the updated running buffers and every parameter gradient, per tensor.  Control: batch
    statistics over the valid frames only.  hidden 640 routes the convs to other kernels; its gate is the measured one too
    (single ReLU pre-activations change sign between precisions, the fp32 CPU run sits further from float64 there)."""
    mel, lengths, targets, tl, P = TC.graph_case(hidden, T)
    r64 = TC.graph_reference(P, mel, lengths, targets, tl, torch.float64)
    r32 = TC.graph_reference(P, mel, lengths, targets, tl, torch.float32)
    c64 = TC.graph_reference(P, mel, lengths, targets, tl, torch.float64, masked_stats=True)
    m = trainable(hidden, P)
    got = device_step(m, mel, lengths, targets, tl, 0.0, 1)
    assert int(m.state_dict()["encoder.layers.0.2.num_batches_tracked"]) == 101
    check_graph(f"graph hidden={hidden} T={T}", got, r64, r32, c64)


def test_training_graph_with_dropout():
    """dropout 0.1: the restatement multiplies by hash_uniform(seed, site, B C T) >= p.  Control: the sites shifted by one
    (the running buffers of layer 0 lie in front of every dropout and do not see it)."""
    hidden, T, seed = 80, 34, 77
    mel, lengths, targets, tl, P = TC.graph_case(hidden, T)
    r64 = TC.graph_reference(P, mel, lengths, targets, tl, torch.float64, 0.1, seed)
    r32 = TC.graph_reference(P, mel, lengths, targets, tl, torch.float32, 0.1, seed)
    c64 = TC.graph_reference(P, mel, lengths, targets, tl, torch.float64, 0.1, seed, site_shift=1)
    got = device_step(trainable(hidden, P), mel, lengths, targets, tl, 0.1, seed)
    check_graph(f"graph dropout hidden={hidden} T={T}", got, r64, r32, c64,
                control_skip=("encoder.layers.0.2.running_mean", "encoder.layers.0.2.running_var"))


def test_second_backward_and_bf16_are_refused():
    import stylish_tts_amd as S
    from stylish_tts_amd import lib as L
    from stylish_tts_amd.alignment import ctc_loss
    mel, lengths, targets, tl, P = TC.graph_case(80, 9)
    m = trainable(80, P)
    lp = m.forward_train(mel.to(DEV), lengths.to(DEV), 0.0, 1)
    _, _, d = ctc_loss(lp, targets, lengths, tl, TC.BLANK)
    m.backward(d)
    with pytest.raises(S.StyError, match="one backward per"):
        m.backward(d)
    with pytest.raises(S.StyError, match="fp32 operands"):
        m.set_train_opts(compute_bf16=True)
    lib = L.load()
    h = C.c_void_p()
    assert lib.sty_model_create(b"text_aligner_train", C.byref(h)) == 0
    opts = L.TrainOpts(0, 0, 0, 0, 0.1, 0, 0.2, 1, 0, 0.2)
    assert lib.sty_model_set_train_opts(h, C.byref(opts)) == -1 and b"fp32 operands" in lib.sty_last_error()
    assert lib.sty_model_enable_training(h) == 0
    lib.sty_model_destroy(h)


def test_validation_forward_is_the_inference_forward():
    """the eval-mode forward of the trainable kind equals TextAligner.forward bit for bit, before and after a training step"""
    import stylish_tts_amd as S
    from stylish_tts_amd.alignment import ctc_loss
    mel, lengths, targets, tl, P = TC.graph_case(80, 34)
    m = trainable(80, P)
    ref = S.TextAligner(AC.N_MELS, AC.TOKENS, hidden_dim=80)
    for step in range(2):
        ref.load_state_dict(m.state_dict(), strict=True)
        ref = ref.to(DEV).eval()
        with torch.no_grad():
            a, b = m(mel.to(DEV), lengths.to(DEV)), ref(mel.to(DEV), lengths.to(DEV))
        assert torch.equal(a, b)
        lp = m.forward_train(mel.to(DEV), lengths.to(DEV), 0.1, 5)
        _, _, d = ctc_loss(lp, targets, lengths, tl, TC.BLANK)
        m.backward(d)


# ---- trainer and command -------------------------------------------------------------------------------------------
def synthetic_batch(B=4, T=40, seed=3):
    g = torch.Generator().manual_seed(seed)
    audio = 0.1 * torch.randn(B, T * 300, generator=g)
    tl = torch.tensor([9, 7, 5, 3])[:B]
    texts = torch.zeros(B, int(tl.max()), dtype=torch.long)
    import numpy as np
    rs = np.random.RandomState(seed)
    for b in range(B):
        texts[b, :int(tl[b])] = torch.tensor(TC.make_targets(rs, int(tl[b])))
    return dict(audio_gt=audio.to(DEV), texts=texts.to(DEV), text_lengths=tl.to(DEV))


def make_trainer(lr=1e-3, seed=0):
    from stylish_tts_amd.alignment import AlignmentTrainer, TrainableTextAligner
    torch.manual_seed(1234)
    m = TrainableTextAligner(AC.N_MELS, AC.TOKENS, hidden_dim=80).to(DEV)
    return AlignmentTrainer(m, lr=lr, w_align=1.0, mean=-4.0, std=4.0, dropout=0.1, seed=seed)


def test_trainer_learns_one_batch():
    """30 steps at lr 1e-3 on one fixed batch: finite throughout, the loss ends below 0.6 x its first value (a wide margin,
    not tuned), the running buffers moved, num_batches_tracked counts the steps"""
    tr = make_trainer()
    batch = synthetic_batch()
    rm0 = tr.aligner.state_dict()["encoder.layers.1.2.running_mean"].clone()
    losses = [float(tr.train_batch(seed=i, **batch)["align_loss"]) for i in range(30)]
    assert all(math.isfinite(v) for v in losses), losses
    print(f"\n  align_train trainer: loss {losses[0]:.4f} -> {losses[-1]:.4f} in 30 steps (ratio {losses[-1] / losses[0]:.3f})")
    assert losses[-1] < 0.6 * losses[0]
    sd = tr.aligner.state_dict()
    assert not torch.equal(sd["encoder.layers.1.2.running_mean"], rm0)
    assert all(int(sd[f"encoder.layers.{i}.2.num_batches_tracked"]) == 30 for i in range(3))
    out, (total, frames) = tr.validate(**batch)
    assert math.isfinite(float(out["align_loss"])) and 0.0 < float(out["confidence"]) <= 1.0 and frames > 0


def test_checkpoint_round_trip(tmp_path):
    """save after 3 steps, load into a fresh trainer: the next step's loss and parameters are equal bit for bit"""
    from stylish_tts_amd import stage_io as IO
    batch = synthetic_batch()
    a = make_trainer()
    for i in range(3):
        a.train_batch(seed=i, **batch)
    IO.save_checkpoint(str(tmp_path / "ck"), **a.checkpoint_state())
    assert (tmp_path / "ck" / "pytorch_model.bin").exists()
    b = make_trainer()
    st = b.checkpoint_state()
    IO.load_checkpoint(str(tmp_path / "ck"), st["models"], optimizers=st["optimizers"])
    la, lb = a.train_batch(seed=3, **batch)["align_loss"], b.train_batch(seed=3, **batch)["align_loss"]
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    sa, sb = a.aligner.state_dict(), b.aligner.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def _dataset(tmp_path, n, n_val, **plan):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_sample_dataset as M
    import yaml
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    root = tmp_path / "data"
    lines = M.make(str(root), n=n, seed=33, n_val=n_val)
    for f in ("alignment.safetensors", "pitch.safetensors"):
        os.remove(root / f)
    cfg = yaml.safe_load(_default_config_yaml(root))
    cfg["training_plan"]["alignment"].update(plan)
    cfg["training"].update(val_interval=4, save_interval=100, log_interval=1)
    cfg_path, mdl_path = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    mdl_path.write_text(_default_model_yaml())
    return root, lines, str(cfg_path), str(mdl_path)


def test_train_align_command_end_to_end(tmp_path):
    """make_sample_dataset's layout -> train_align (6 steps, one val pass) -> alignment_model.safetensors, which loads into
    TextAligner (strict) and from which `align` writes one entry per segment"""
    import stylish_tts_amd as S
    from stylish_tts_amd import align as A
    from stylish_tts_amd import train_align as TA
    root, lines, cfg, mdl = _dataset(tmp_path, n=8, n_val=2, probe_batch_max=3, epochs=50)
    logged = []
    TA.train_align(cfg, mdl, str(tmp_path / "out"), max_steps=6, log=logged.append)
    assert any("utterances/s" in ln for ln in logged), logged
    print("\n  " + [ln for ln in logged if "utterances/s" in ln][-1])
    assert any("confidence" in ln for ln in logged), logged
    path = root / "alignment_model.safetensors"
    assert path.exists() and (tmp_path / "out" / "alignment" / "checkpoint_final" / "pytorch_model.bin").exists()
    sd = load_file(str(path))
    m = S.TextAligner(AC.N_MELS, AC.TOKENS, hidden_dim=640)
    m.load_state_dict(sd, strict=True)
    A.align(cfg, mdl, "torch", 4, log=lambda *_: None)
    result = load_file(str(root / "alignment.safetensors"))
    assert sorted(result) == sorted(ln.split("|")[0] for ln in lines)


def test_second_epoch_applies_the_priors(tmp_path):
    """a 2-batch dataset, max_steps across the epoch boundary: the second epoch trains with log_priors, all >= -12"""
    from stylish_tts_amd import train_align as TA
    root, lines, cfg, mdl = _dataset(tmp_path, n=5, n_val=1, probe_batch_max=2, epochs=50)
    ctx = TA.train_align(cfg, mdl, str(tmp_path / "out"), max_steps=5, log=lambda *_: None)
    pri = ctx.trainer.priors.log_priors
    assert ctx.manifest.current_epoch >= 2
    assert pri is not None and pri.numel() == AC.TOKENS + 1 and float(pri.min()) >= -12.0
    assert ctx.applied_priors_steps >= 1
