"""Host restatements and cases of the alignment stage's training path (tests/test_align_train.py,
tests/test_align_train_gpu.py).  Nothing here touches the GPU or the library.

  aligner_forward_train(P, mel, lengths, dt, drop_p, seed)   tdnn_blstm_ctc_model_base under module.train() restated with
                                       torch.nn.functional in dtype dt; the weights are autograd leaves.  masked_stats / site_shift
                                       are the negative controls (batch statistics over valid frames only; dropout sites off by one)
  ctc_reference(...)                   F.ctc_loss(reduction="none") on the CPU / clamp(U, 1), averaged
  ctc_nll_recurrence(...)              the alpha recurrence in torch ops, differentiable by autograd (the gradient's reference where
                                       the scores are not normalised: torch's ctc_loss backward assumes they are)
  ctc_from_logits(...)                 ctc_reference(log_softmax(logits) - scale * priors) with the gradient w.r.t. the logits
  gate(ref64, ref32)                   max(1e-5 max|ref64|, 4 |ref32 - ref64|), the rule of test_align_gpu.forward_gate
  CTC_CASES / ctc_case(i)              the kernel's cases: T, target lengths, input lengths, repeats
  graph_case(hidden, T)                the training graph's cases
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.blocks import hash_uniform
from tests import align_cases as AC

V1 = AC.TOKENS + 1
BLANK = AC.BLANK
# what sty_ctc_loss_fwd_bwd receives for 0.3: the C ABI takes prior_scale as a float
PRIOR_SCALE = float(torch.tensor(0.3, dtype=torch.float32))


def gate(ref64, ref32):
    """-> (gate, scale, own): the fp32 CPU run's own distance from float64 on this case sets the gate"""
    scale = ref64.abs().max().item()
    own = (ref32.double() - ref64).abs().max().item()
    return max(1e-5 * scale, 4 * own), scale, own


def dist(a, ref64):
    return (a.detach().cpu().double() - ref64).abs().max().item()


# ---- the TextAligner under module.train() ---------------------------------------------------------------------------
def aligner_forward_train(P, mel, lengths, dtype=torch.float64, drop_p=0.0, seed=1, masked_stats=False, site_shift=0):
    """mel [B, n_mels, T], lengths [B] -> dict(log_probs [B, T, V1], logits [B, T, V1], W = the leaves, running = the updated
    running_mean / running_var by key).  text_aligner.py:209-274 in training mode: the mask in front of each TDNN conv only,
    BatchNorm1d(affine=False) on the statistics of all B * T positions (momentum 0.1, unbiased running variance), Dropout
    behind each BatchNorm (sites 0-2) and each Ffn ReLU (sites 3-7) with the hash mask over the [B, C, T] linear index."""
    W = {k: v.to(dtype).clone().requires_grad_(True) for k, v in P.items()
         if v.is_floating_point() and "running_" not in k}
    running = {k: v.to(dtype).clone() for k, v in P.items() if "running_" in k}
    x = mel.to(dtype)
    B, _, T = x.shape
    valid = torch.arange(T)[None, :] < lengths.reshape(-1, 1)
    mask = valid.to(dtype)[:, None, :]

    def drop(y, site):  # y [B, C, T]
        if drop_p <= 0.0:
            return y
        u = hash_uniform(seed, site + site_shift, y.numel()).view(y.shape)
        return y * ((u >= drop_p).to(dtype) / (1.0 - drop_p))

    for i, k in enumerate(AC.TDNN_KERNELS):
        p = f"encoder.layers.{i}."
        x = torch.relu(F.conv1d(x * mask, W[p + "0.weight"], W[p + "0.bias"], padding=(k - 1) // 2))
        if masked_stats:  # the control: statistics over the valid frames only
            n = valid.sum().to(dtype)
            mu = (x * mask).sum(dim=(0, 2)) / n
            var = (((x - mu[None, :, None]) ** 2) * mask).sum(dim=(0, 2)) / n
            with torch.no_grad():
                running[p + "2.running_mean"].mul_(0.9).add_(0.1 * mu)
                running[p + "2.running_var"].mul_(0.9).add_(0.1 * var * n / (n - 1))
            x = (x - mu[None, :, None]) / torch.sqrt(var[None, :, None] + 1e-5)
        else:
            x = F.batch_norm(x, running[p + "2.running_mean"], running[p + "2.running_var"], None, None, True, 0.1, 1e-5)
        x = drop(x, i)
    y = x
    for j in range(5):
        q = f"encoder.layers.3.ffn.{3 * j}."
        y = torch.relu(F.linear(y.transpose(1, 2), W[q + "weight"], W[q + "bias"])).transpose(1, 2)
        y = drop(y, 3 + j)
    y = y + x
    logits = F.linear(y.transpose(1, 2), W["encoder_output_layer.weight"], W["encoder_output_layer.bias"])
    return dict(log_probs=F.log_softmax(logits, dim=-1), logits=logits, W=W, running=running)


# ---- CTC ------------------------------------------------------------------------------------------------------------
def ctc_reference(log_probs, targets, input_lengths, target_lengths, blank=BLANK):
    """log_probs [B, T, V1] (CPU, any float dtype) -> (loss = mean_b(nll_b / clamp(U_b, 1)), nll [B])"""
    nll = F.ctc_loss(log_probs.transpose(0, 1), targets, input_lengths, target_lengths, blank=blank, reduction="none",
                     zero_infinity=False)
    return (nll / target_lengths.clamp(min=1).to(nll.dtype)).mean(), nll


def ctc_nll_recurrence(log_probs, targets, input_lengths, target_lengths, blank=BLANK):
    """The alpha recurrence written out in torch ops, differentiable by autograd: nll [B].  torch's own ctc_loss backward
    returns exp(log_probs) - occupancy, i.e. it assumes NORMALISED log-probs (the log_softmax backward is folded into it);
    on log_probs - scale * priors that is not the gradient of the loss.  This restatement has no such assumption; on
    normalised log-probs its gradient equals torch's (tests/test_align_train.py holds it to that)."""
    big = -1e30  # stands in for -inf: logsumexp of three of them stays finite and carries no gradient to the result
    B, T, _ = log_probs.shape
    U = targets.shape[1]
    S = 2 * U + 1
    ext = torch.full((B, S), blank, dtype=torch.long)
    ext[:, 1::2] = targets
    skip = torch.zeros(B, S, dtype=torch.bool)
    if U > 1:
        skip[:, 3::2] = targets[:, 1:] != targets[:, :-1]
    s_idx = torch.arange(S)[None, :]
    skip &= s_idx < (2 * target_lengths[:, None] + 1)  # (padding tokens are never entered by a skip)
    lp = torch.gather(log_probs, 2, ext[:, None, :].expand(B, T, S))  # [B, T, S]
    neg = lp.new_full((B, S), big)
    alpha = torch.where(s_idx < 2, lp[:, 0], neg)
    pad = lp.new_full((B, 2), big)
    for t in range(1, T):
        prev = torch.cat([pad, alpha], dim=1)
        x2 = torch.where(skip, prev[:, :S], neg)
        new = torch.logsumexp(torch.stack([prev[:, 2:], prev[:, 1:S + 1], x2]), dim=0) + lp[:, t]
        alpha = torch.where((t < input_lengths)[:, None], new, alpha)
    last = 2 * target_lengths  # state S_b - 1; states beyond it are padding and feed nothing below them
    end = torch.cat([pad, alpha], dim=1)
    a1 = end.gather(1, (last + 2)[:, None])[:, 0]
    a2 = end.gather(1, (last + 1)[:, None])[:, 0]
    return -torch.logsumexp(torch.stack([a1, a2]), dim=0)


def ctc_from_logits(logits, targets, input_lengths, target_lengths, dtype, blank=BLANK, log_priors=None, weight=1.0,
                    recurrence=None):
    """-> (loss, nll, d (weight * loss) / d logits [B, T, V1]) in `dtype`, through autograd.  The loss values come from
    F.ctc_loss; so does the gradient on normalised log-probs.  With priors the scores are not normalised and the gradient comes
    from ctc_nll_recurrence (recurrence=True forces it, the test of the restatement itself)."""
    z = logits.detach().to(dtype).clone().requires_grad_(True)
    lp = F.log_softmax(z, dim=-1)
    if log_priors is not None:
        lp = lp - torch.tensor(PRIOR_SCALE, dtype=dtype) * log_priors.to(dtype)
    loss, nll = ctc_reference(lp, targets, input_lengths, target_lengths, blank)
    if recurrence if recurrence is not None else log_priors is not None:
        nll_r = ctc_nll_recurrence(lp, targets, input_lengths, target_lengths, blank)
        (weight * (nll_r / target_lengths.clamp(min=1).to(dtype)).mean()).backward()
    else:
        (weight * loss).backward()
    return loss.detach(), nll.detach(), z.grad


def make_targets(rs, U, repeat_every=0, lo=1):
    """U tokens in [lo, TOKENS) without accidental adjacent repeats (lo = 1: the tokens stay valid for the blank = 0
    control); repeat_every = k: tokens k - 1, 2 k - 1, ... repeat their predecessor"""
    t = []
    for i in range(U):
        if repeat_every and i > 0 and (i + 1) % repeat_every == 0:
            t.append(t[-1])
            continue
        v = int(rs.randint(lo, AC.TOKENS))
        while t and v == t[-1]:
            v = int(rs.randint(lo, AC.TOKENS))
        t.append(v)
    return t


# T, target lengths, input lengths, repeat_every
CTC_CASES = [
    (8, (0, 1, 2), (8, 1, 5), 0),
    (66, (31, 32, 33), (66, 66, 40), 0),
    (130, (64, 65, 20), (130, 129, 97), 0),
    (12, (4, 4, 4), (6, 12, 9), 2),        # row 0: exactly one valid path (T = U + repeats)
    (520, (255, 100, 3), (520, 300, 7), 7),
    (1030, (510, 200, 1), (1030, 700, 2), 11),
]


def ctc_case(i):
    """-> logits [3, T, V1] fp32 (3 * randn), targets [3, U], input_lengths, target_lengths, log_priors [V1] in [-12, 0]"""
    T, tl, il, rep = CTC_CASES[i]
    rs = np.random.RandomState(100 + i)
    logits = torch.from_numpy(rs.standard_normal((3, T, V1)).astype(np.float32) * 3.0)
    U = max(max(tl), 1)
    targets = torch.zeros(3, U, dtype=torch.long)
    for b, u in enumerate(tl):
        targets[b, :u] = torch.tensor(make_targets(rs, u, rep), dtype=torch.long)
    priors = torch.from_numpy(rs.uniform(-12.0, 0.0, size=V1).astype(np.float32))
    return logits, targets, torch.tensor(il), torch.tensor(tl), priors


def graph_case(hidden, T, seed_offset=0):
    """B = 3: mel [3, n_mels, T], lengths [T, 5T/8, max(3, T/4)], target lengths [T/3, T/6, 1], targets, the seeded weights"""
    g = torch.Generator().manual_seed(7000 * hidden + T + seed_offset)
    mel = torch.randn(3, AC.N_MELS, T, generator=g)
    lengths = torch.tensor([T, (5 * T) // 8, max(3, T // 4)])
    tl = torch.tensor([T // 3, max(T // 6, 1), 1])
    rs = np.random.RandomState(hidden + T)
    targets = torch.zeros(3, int(tl.max()), dtype=torch.long)
    for b in range(3):
        targets[b, :int(tl[b])] = torch.tensor(make_targets(rs, int(tl[b])), dtype=torch.long)
    return mel, lengths, targets, tl, AC.aligner_weights(hidden, 11 + hidden)


def graph_reference(P, mel, lengths, targets, tl, dtype, drop_p=0.0, seed=1, **control):
    """the restatement's log_probs, updated running buffers and parameter gradients of the CTC loss, detached, by key"""
    r = aligner_forward_train(P, mel, lengths, dtype, drop_p, seed, **control)
    loss, _ = ctc_reference(r["log_probs"], targets, lengths, tl)
    loss.backward()
    out = {"log_probs": r["log_probs"].detach(), "loss": loss.detach()}
    out.update({k: v.detach() for k, v in r["running"].items()})
    out.update({"grad." + k: v.grad.detach() for k, v in r["W"].items()})
    return out
