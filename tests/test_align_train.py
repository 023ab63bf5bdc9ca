"""The alignment stage's training path without a device: the new symbols and the new model kind, the argument checks of the
CTC entry point, the label priors' bookkeeping against the literal formula, the trainable shell's state_dict, and the
command's refusals.  (The kernels are tested in tests/test_align_train_gpu.py.)"""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests import align_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sty_ctc_loss_workspace_bytes", "sty_ctc_loss_fwd_bwd", "sty_aligner_train_workspace_bytes", "sty_aligner_fwd_train",
       "sty_aligner_bwd")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from stylish_tts_amd import lib as L
    return L.load()


def test_new_symbols_are_declared_and_exported(lib):
    from stylish_tts_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "stylish_hip.h")).read()
    declared = set(re.findall(r"\b(sty_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert "alignment stage, training" in hdr


def test_ctc_workspace_refuses_bad_sizes(lib):
    need = C.c_size_t()
    assert lib.sty_ctc_loss_workspace_bytes(3, 1030, 179, 512, C.byref(need)) == 0
    assert need.value >= 3 * 1030 * 1025 * 8
    assert lib.sty_ctc_loss_workspace_bytes(3, 10, 179, 513, C.byref(need)) == -1 and b"U <= 512" in lib.sty_last_error()
    assert lib.sty_ctc_loss_workspace_bytes(0, 10, 179, 5, C.byref(need)) == -1
    assert lib.sty_ctc_loss_workspace_bytes(1, 0, 179, 5, C.byref(need)) == -1
    assert lib.sty_ctc_loss_workspace_bytes(1, 10, 179, 5, None) == -1
    # the entry point checks its arguments before it touches the device
    assert lib.sty_ctc_loss_fwd_bwd(1, 4, 179, 2, None, None, 0.3, None, None, None, 178, 1.0, None, None, None, None, None, 0,
                                    None) == -1


def test_training_kind_exists_and_waits_for_finalize(lib):
    h = C.c_void_p()
    assert lib.sty_model_create(b"text_aligner_train", C.byref(h)) == 0
    assert lib.sty_model_enable_training(h) == 0
    need = C.c_size_t()
    assert lib.sty_aligner_train_workspace_bytes(h, 2, 16, C.byref(need)) == -5  # STY_ESTATE: not finalized
    assert lib.sty_aligner_workspace_bytes(h, 2, 16, C.byref(need)) == -5
    assert lib.sty_aligner_bwd(h, None, None) == -5
    lib.sty_model_destroy(h)
    # the entry points belong to the new kind only
    assert lib.sty_model_create(b"text_aligner", C.byref(h)) == 0
    assert lib.sty_aligner_train_workspace_bytes(h, 2, 16, C.byref(need)) == -1
    assert b"does not provide this entry point" in lib.sty_last_error()
    lib.sty_model_destroy(h)


def test_label_priors_follow_the_literal_formula():
    """losses.py:537-560, 617-653 on host tensors: logsumexp over the valid frames of every batch, combined by logsumexp;
    log_priors = max(log_sum - log(frames + 1e-9), -12); the sums start again"""
    from stylish_tts_amd.alignment import LabelPriors
    g = torch.Generator().manual_seed(0)
    a = torch.log_softmax(3 * torch.randn(3, 20, 9, generator=g), dim=-1)
    b = torch.log_softmax(3 * torch.randn(2, 11, 9, generator=g), dim=-1)
    a[:, :, 4] = -40.0  # a class nobody emits: floored
    b[:, :, 4] = -40.0
    la, lb = torch.tensor([20, 7, 1]), torch.tensor([11, 5])
    p = LabelPriors()
    assert p.log_priors is None
    p.accumulate(a, la)
    p.accumulate(b, lb)
    assert p.log_priors is None and p.num_frames == 44
    p.on_epoch_end()
    flat = torch.cat([a[i, :int(n)] for i, n in enumerate(la)] + [b[i, :int(n)] for i, n in enumerate(lb)], 0)
    want = torch.logsumexp(flat.double(), dim=0) - math.log(44 + 1e-9)
    want = torch.where(want < -12.0, torch.tensor(-12.0, dtype=torch.float64), want)
    assert p.log_priors.shape == (9,) and float(p.log_priors[4]) == -12.0
    assert (p.log_priors.double() - want).abs().max().item() < 1e-5
    assert p.log_sum is None and p.num_frames == 0
    q = LabelPriors()
    q.load_state_dict(p.state_dict())
    assert torch.equal(q.log_priors, p.log_priors)
    p.on_epoch_end()  # an epoch without a batch keeps the priors
    assert torch.equal(q.log_priors, p.log_priors)


def test_trainable_shell_has_the_inference_shells_state_dict():
    import stylish_tts_amd as S
    from stylish_tts_amd.alignment import TrainableTextAligner
    a, b = TrainableTextAligner(hidden_dim=80), S.TextAligner(hidden_dim=80)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert all(sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype for k in sa)
    assert sorted(sa.keys()) == sorted(AC.aligner_weights(80).keys())
    assert a.KIND == "text_aligner_train" and b.KIND == "text_aligner"
    b.load_state_dict(sa, strict=True)
    with pytest.raises(S.StyError, match="fp32 operands"):
        a.set_train_opts(compute_bf16=True)
    with pytest.raises(S.StyError):
        a.forward_train(torch.zeros(1, 80, 4), torch.tensor([4]))  # no CPU path


def test_train_align_refuses_what_it_cannot_run(tmp_path):
    from stylish_tts_amd import train_align as TA
    from stylish_tts_amd.alignment import AlignmentTrainer, ctc_loss
    from stylish_tts_amd.lib import StyError
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    cfg, mdl = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg.write_text(_default_config_yaml(tmp_path / "nowhere"))
    mdl.write_text(_default_model_yaml())
    with pytest.raises(StyError, match="model config path is required"):
        TA.train_align(str(cfg), "", str(tmp_path / "out"))
    if not torch.cuda.is_available():
        with pytest.raises(StyError, match="no HIP device"):
            TA.train_align(str(cfg), str(mdl), str(tmp_path / "out"))
    else:
        with pytest.raises(StyError, match="not found"):
            TA.train_align(str(cfg), str(mdl), str(tmp_path / "out"))
    with pytest.raises(StyError, match="HIP device"):
        ctc_loss(torch.zeros(1, 4, 179), torch.zeros(1, 2, dtype=torch.long), torch.tensor([4]), torch.tensor([2]), 178)
    import stylish_tts_amd as S
    with pytest.raises(StyError, match="TrainableTextAligner"):
        AlignmentTrainer(S.TextAligner(hidden_dim=80))
    os.environ["WORLD_SIZE"] = "2"
    try:
        with pytest.raises(StyError, match="one process"):
            TA.train_align(str(cfg), str(mdl), str(tmp_path / "out"))
    finally:
        del os.environ["WORLD_SIZE"]
    with pytest.raises(SystemExit):
        TA.main(["--help"])


def test_ctc_recurrence_restatement_against_torch():
    """tests/align_train_cases.ctc_nll_recurrence, the gradient's reference where the scores carry priors: on normalised
    log-probs its values and its gradient are torch's ctc_loss's (float64, 1e-12); with priors the VALUES still agree and
    torch's gradient does not (its backward folds a log_softmax in, i.e. assumes normalised log-probs) -- which is why the
    device's gradient is held to the recurrence there"""
    from tests import align_train_cases as TC
    for case in (0, 3):
        logits, tg, il, tl, pri = TC.ctc_case(case)
        _, nll_t, g_t = TC.ctc_from_logits(logits, tg, il, tl, torch.float64, recurrence=False)
        _, _, g_r = TC.ctc_from_logits(logits, tg, il, tl, torch.float64, recurrence=True)
        assert (g_t - g_r).abs().max().item() < 1e-12
        lp = torch.log_softmax(logits.double(), -1)
        assert ((TC.ctc_nll_recurrence(lp, tg, il, tl) - nll_t).abs() / nll_t).max().item() < 1e-12
        lpp = lp - TC.PRIOR_SCALE * pri.double()
        _, nll_p = TC.ctc_reference(lpp, tg, il, tl)
        assert ((TC.ctc_nll_recurrence(lpp, tg, il, tl) - nll_p).abs() / nll_p).max().item() < 1e-12
        _, _, gp_t = TC.ctc_from_logits(logits, tg, il, tl, torch.float64, log_priors=pri, recurrence=False)
        _, _, gp_r = TC.ctc_from_logits(logits, tg, il, tl, torch.float64, log_priors=pri)
        assert (gp_t - gp_r).abs().max().item() > 1e-2
        # a finite difference of the loss sides with the recurrence
        z = logits.double().clone()
        b, t, v = 2, 0, int(tg[2, 0])
        h = 1e-5

        def loss_at(zz):
            q = torch.log_softmax(zz, -1) - TC.PRIOR_SCALE * pri.double()
            return float(TC.ctc_reference(q, tg, il, tl)[0])
        zp, zm = z.clone(), z.clone()
        zp[b, t, v] += h
        zm[b, t, v] -= h
        fd = (loss_at(zp) - loss_at(zm)) / (2 * h)
        assert abs(fd - float(gp_r[b, t, v])) < 1e-6 * max(1.0, abs(fd))
