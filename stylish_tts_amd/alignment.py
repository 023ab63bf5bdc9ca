"""The alignment stage (train_alignment / validate_alignment, train/stage_type.py:268-341) on the HIP path: the TextAligner
in its training graph, the CTC loss with its gradient on the device, the label priors' bookkeeping and the trainer the
`train-align` command (stylish_tts_amd/train_align.py) drives.

  TrainableTextAligner   TextAligner under the model kind `text_aligner_train`: forward_train / backward, the same state_dict
  ctc_loss               sty_ctc_loss_fwd_bwd: exact CTC in float64 log-space (the reference asks k2 for use_double_scores=True;
                         k2's output_beam = 10 pruning is not reproduced), the log-softmax backward folded into the gradient
  LabelPriors            CTCLossWithLabelPriors' bookkeeping (train/losses.py:537-560, 617-653)
  AlignmentTrainer       one optimizer step / one validation batch

One process: the priors' all-gather over ranks (losses.py:619-624) is not built, a world size above one is refused.
"""
import ctypes as C
import math
import os

import torch

from . import lib as L
from .align import ALIGNER_MEL, TextAligner, _stream, forced_align
from .modules import _f32

PRIOR_SCALE = 0.3     # CTCLossWithLabelPriors(prior_scaling_factor=0.3) (train/train_context.py)
PRIOR_FLOOR = -12.0   # losses.py:646-649


class TrainableTextAligner(TextAligner):
    """TextAligner with the training graph (model kind `text_aligner_train`: same keys, same plan).  forward() is the eval-mode
    forward on running statistics, bit for bit TextAligner's; forward_train() is CTCModel.forward under module.train(), to be
    followed by ONE backward(d_logits).  A file written from this state_dict loads into TextAligner unchanged."""
    KIND = "text_aligner_train"

    def enable_training(self):
        self._train = True
        return self

    def set_train_opts(self, **kw):
        if kw.get("compute_bf16"):
            raise L.StyError("TrainableTextAligner: compute_bf16 is refused: the aligner runs fp32 operands (alignment "
                             "decisions are arg-max decisions)")
        return super(TextAligner, self).set_train_opts(**kw)

    def forward_train(self, mels, mel_lengths, drop_p=0.1, seed=1):
        """mels [B, n_mels, T], mel_lengths [B] -> log_probs [B, T, tokens + 1].  BatchNorm runs on batch statistics over all
        B * T positions and updates running_mean / running_var in place; num_batches_tracked (int64, never bound) is counted
        here.  Dropout masks are hash(seed, site, element) and are recomputed by the backward."""
        if mels.dim() != 3 or mels.shape[1] != self.n_mels or tuple(mel_lengths.shape) != (mels.shape[0],):
            raise L.StyError(f"TrainableTextAligner: mels {tuple(mels.shape)} / mel_lengths {tuple(mel_lengths.shape)} do "
                             f"not fit [B, {self.n_mels}, T] / [B]")
        if not 0.0 <= float(drop_p) < 1.0:
            raise L.StyError("TrainableTextAligner: drop_p must be in [0, 1)")
        dev = mels.device
        self._train = True
        self._tape_id += 1
        lib = self._ensure(dev)
        B, _, T = mels.shape
        x = _f32(mels.detach(), dev)
        ln = mel_lengths.to(dev, torch.int64).contiguous()
        out = torch.empty(B, T, self.tokens + 1, dtype=torch.float32, device=dev)
        need = C.c_size_t()
        L.check(lib.sty_aligner_train_workspace_bytes(self._handle, B, T, C.byref(need)))
        if getattr(self, "_train_ws", None) is None or self._train_ws.numel() < need.value or self._train_ws.device != dev:
            self._train_ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        self._train_keep = [x, ln]
        L.check(lib.sty_aligner_fwd_train(self._handle, B, T, L.ptr(x), L.ptr(ln), float(drop_p), int(seed) & 0xFFFFFFFF,
                                          L.ptr(out), L.ptr(self._train_ws), self._train_ws.numel(), _stream(dev)))
        self._train_shape = (B, self.tokens + 1, T)
        for i in range(3):
            self.get_buffer(f"encoder.layers.{i}.2.num_batches_tracked").add_(1)
        return out

    def backward(self, d_logits):
        """d loss / d logits [B, tokens + 1, T] (channel-major, as ctc_loss returns it); parameter gradients are added to
        .grad.  A second backward of the same forward raises."""
        lib = L.load()
        if tuple(d_logits.shape) != getattr(self, "_train_shape", None):
            raise L.StyError(f"TrainableTextAligner.backward: d_logits {tuple(d_logits.shape)} does not fit the recorded "
                             f"forward {getattr(self, '_train_shape', None)}")
        d = _f32(d_logits, d_logits.device)
        L.check(lib.sty_aligner_bwd(self._handle, L.ptr(d), _stream(d.device)))


def ctc_loss(log_probs, targets, input_lengths, target_lengths, blank, *, log_priors=None, prior_scale=PRIOR_SCALE,
             weight=1.0, want_grad=True, check=True):
    """log_probs [B, T, V1] fp32 on the device, targets [B, U], input_lengths / target_lengths [B] ->
    (loss [1] = mean_b(nll_b / max(U_b, 1)), unweighted; nll [B] float64; d_logits [B, V1, T] = weight * d loss / d logits, or
    None).  With log_priors [V1] the scores are log_probs - prior_scale * log_priors.  A row without a valid path has
    nll = +inf (the loss is then +inf: zero_infinity=False) and a zero gradient; a row whose length or target is out of range
    raises, naming the rows (check=False hands the status out as the fourth value instead)."""
    if not log_probs.is_cuda:
        raise L.StyError("ctc_loss: log_probs must live on a HIP device (there is no CPU path)")
    if log_probs.dim() != 3 or targets.dim() != 2 or targets.shape[0] != log_probs.shape[0]:
        raise L.StyError(f"ctc_loss: log_probs {tuple(log_probs.shape)} / targets {tuple(targets.shape)} do not fit "
                         "[B, T, V1] / [B, U]")
    lib = L.load()
    dev = log_probs.device
    B, T, V1 = log_probs.shape
    U = targets.shape[1]
    lp = _f32(log_probs, dev)
    tg = targets.to(dev, torch.int64).contiguous()
    il = input_lengths.to(dev, torch.int64).contiguous()
    tl = target_lengths.to(dev, torch.int64).contiguous()
    if tuple(il.shape) != (B,) or tuple(tl.shape) != (B,):
        raise L.StyError("ctc_loss: input_lengths / target_lengths must be [B]")
    pri = None
    if log_priors is not None:
        pri = _f32(log_priors.reshape(-1), dev)
        if pri.numel() != V1:
            raise L.StyError(f"ctc_loss: log_priors must hold {V1} values (got {pri.numel()})")
    nll = torch.empty(B, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    d_logits, ws, nws = None, None, 0
    if want_grad:
        d_logits = torch.empty(B, V1, T, dtype=torch.float32, device=dev)
        need = C.c_size_t()
        L.check(lib.sty_ctc_loss_workspace_bytes(B, T, V1, U, C.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        nws = ws.numel()
    L.check(lib.sty_ctc_loss_fwd_bwd(B, T, V1, U, L.ptr(lp), L.ptr(pri), float(prior_scale), L.ptr(tg), L.ptr(il), L.ptr(tl),
                                     int(blank), float(weight), L.ptr(nll), L.ptr(loss), L.ptr(status), L.ptr(d_logits),
                                     L.ptr(ws), nws, _stream(dev)))
    if not check:
        return loss, nll, d_logits, status
    bad = [i for i, s in enumerate(status.cpu().tolist()) if s == 2]
    if bad:
        raise L.StyError(f"ctc_loss: row(s) {bad}: a length or a target token is out of range")
    return loss, nll, d_logits


class LabelPriors:
    """CTCLossWithLabelPriors' bookkeeping (train/losses.py:537-560, 617-653): a running logsumexp over the valid frames of
    every TRAINING batch; at the end of an epoch log_priors = max(log_sum - log(frames + 1e-9), -12) and the sums start again.
    `log_priors` is None during the first epoch.  Plain torch ops on whatever device the log-probs live on."""

    def __init__(self, scale=PRIOR_SCALE):
        self.scale = scale
        self.log_priors, self.log_sum, self.num_frames = None, None, 0

    def accumulate(self, log_probs, input_lengths):
        """log_probs [B, T, V1], input_lengths [B]"""
        T = log_probs.shape[1]
        lengths = input_lengths.to(log_probs.device)
        valid = torch.arange(T, device=log_probs.device)[None, :] < lengths[:, None]
        lp = log_probs.detach().masked_fill(~valid[:, :, None], -float("inf"))
        batch = torch.logsumexp(lp.reshape(-1, lp.shape[-1]), dim=0)
        self.num_frames += int(lengths.sum())
        self.log_sum = batch if self.log_sum is None else torch.logaddexp(self.log_sum, batch)

    def on_epoch_end(self):
        if self.log_sum is None:
            return
        new = self.log_sum - math.log(self.num_frames + 1e-9)
        self.log_priors = torch.clamp(new, min=PRIOR_FLOOR)
        self.log_sum, self.num_frames = None, 0

    def state_dict(self):
        return {"log_priors": None if self.log_priors is None else self.log_priors.detach().cpu(),
                "log_sum": None if self.log_sum is None else self.log_sum.detach().cpu(), "num_frames": self.num_frames}

    def load_state_dict(self, sd, device=None):
        put = lambda t: None if t is None else (t.to(device) if device is not None else t)
        self.log_priors, self.log_sum, self.num_frames = put(sd["log_priors"]), put(sd["log_sum"]), int(sd["num_frames"])


class AlignmentTrainer:
    """train_alignment / validate_alignment (stage_type.py:268-325) with AdamW on flat buckets (train/optimizers.py:110-118)."""

    def __init__(self, aligner, lr=1e-4, betas=(0.85, 0.99), eps=1e-9, weight_decay=1e-4, w_align=1.0, mean=-4.0, std=4.0,
                 dropout=0.1, seed=0, hop_length=300, n_fft=ALIGNER_MEL["n_fft"], win_length=ALIGNER_MEL["win_length"],
                 bucket_bytes=25 << 20, log=print, deterministic=False):
        import random
        # deterministic=True switches the process-wide deterministic mode on (lib.set_deterministic) before anything is sized;
        # False leaves the switch as it is (STY_DETERMINISTIC=1 or an earlier call may have set it)
        if deterministic:
            L.set_deterministic(True)
        from .frontend import MelSpec
        from .optim import FlatAdamW
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise L.StyError("the alignment stage runs in one process: the label priors' all-gather over ranks "
                             "(train/losses.py:619-624) is not built")
        if not isinstance(aligner, TrainableTextAligner):
            raise L.StyError("AlignmentTrainer needs a TrainableTextAligner (TextAligner is the inference-only kind)")
        self.aligner = aligner.enable_training()
        self.blank = aligner.tokens
        self.w_align, self.mean, self.std, self.dropout = float(w_align), mean, std, float(dropout)
        self.to_mel = MelSpec(int(n_fft), int(win_length), int(hop_length))
        self.priors = LabelPriors()
        self._rng = random.Random(seed)
        self.opt = {"text_aligner": FlatAdamW(list(self.aligner.named_parameters()), lr=lr, betas=betas, eps=eps,
                                              weight_decay=weight_decay, bucket_bytes=bucket_bytes)}
        self.base_lr = lr
        self.log = log
        self.skipped = 0

    def _mel(self, audio_gt):
        from .frontend import calculate_mel
        return calculate_mel(audio_gt, self.to_mel, self.mean, self.std)

    def train_batch(self, *, audio_gt, texts, text_lengths, paths=None, seed=None, **_):
        """One step.  Returns {"align_loss": loss [1]} (the unweighted value, as the reference logs it).  A step whose loss is
        not finite (a row without a valid path) is skipped: nothing is applied, a line names the files.  `seed`: the dropout
        seed of this step (the command passes the manifest's total step, so that a resumed run draws the same masks); None
        draws it from the trainer's own generator."""
        opt = self.opt["text_aligner"]
        opt.zero_grad()
        mels, mel_lengths = self._mel(audio_gt)
        drop_seed = self._rng.getrandbits(31) | 1 if seed is None else (int(seed) * 2654435761 + 1) & 0xFFFFFFFF
        log_probs = self.aligner.forward_train(mels, mel_lengths, self.dropout, drop_seed)
        pri = self.priors.log_priors  # from the second epoch on (losses.py:562-564)
        self.priors.accumulate(log_probs, mel_lengths)
        loss, nll, d_logits = ctc_loss(log_probs, texts, mel_lengths, text_lengths, self.blank, log_priors=pri,
                                       prior_scale=self.priors.scale, weight=self.w_align)
        if not bool(torch.isfinite(loss).all()):
            rows = [i for i, v in enumerate(nll.cpu().tolist()) if not math.isfinite(v)]
            names = [paths[i] for i in rows] if paths is not None else rows
            self.log(f"align_loss is not finite: step skipped (no valid CTC path for {names})")
            self.skipped += 1
            self.aligner.backward(torch.zeros_like(d_logits))  # closes the recorded forward; nothing is applied
            opt.zero_grad()
            return {"align_loss": loss}
        self.aligner.backward(d_logits)
        opt.grads.reduce_all()
        world = opt.grads.finish(average=False)
        opt.step(grad_scale=1.0 / world)
        return {"align_loss": loss}

    @torch.no_grad()
    def validate(self, *, audio_gt, texts, text_lengths, **_):
        """validate_alignment: the eval-mode forward, the CTC loss without priors (step_type="eval") and the confidence
        sum(exp(score)) / frames of the forced alignment -> ({"align_loss", "confidence"}, (confidence_total, frames))"""
        mels, mel_lengths = self._mel(audio_gt)
        log_probs = self.aligner(mels, mel_lengths)
        loss, _, _ = ctc_loss(log_probs, texts, mel_lengths, text_lengths, self.blank, want_grad=False)
        try:
            _, scores = forced_align(log_probs, texts, mel_lengths, text_lengths, self.blank)
        except L.StyError as e:  # rows without an alignment hold score 0 on every frame; they count as the reference's would not
            if not hasattr(e, "scores"):
                raise
            scores = e.scores
        valid = torch.arange(scores.shape[1], device=scores.device)[None, :] < mel_lengths.to(scores.device)[:, None]
        total = (scores.exp() * valid).sum()
        frames = int(mel_lengths.sum())
        return {"align_loss": loss, "confidence": total / max(frames, 1)}, (total, frames)

    def schedule(self, step, step_limit):
        from .optim import scheduled_lr
        self.opt["text_aligner"].lr = scheduled_lr(self.base_lr, step, step_limit)

    def on_epoch_end(self):
        self.priors.on_epoch_end()

    def checkpoint_state(self):
        return dict(models={"text_aligner": self.aligner}, optimizers=dict(self.opt))
