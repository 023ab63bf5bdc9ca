"""Shared cases and host restatements of the alignment stage (tests/test_align.py, tests/test_align_gpu.py,
tools/gen_golden_align.py).  Nothing here touches the GPU or the library.

  aligner_weights(hidden, seed)        a seeded TextAligner state_dict (the reference's keys), running_mean != 0, running_var != 1
  aligner_forward(P, mel, lengths, dt) tdnn_blstm_ctc_model_base in eval mode restated with torch.nn.functional, in dtype dt
  viterbi_fp32(lp, targets, blank)     the forced-alignment recurrence in numpy float32 (max and + only): the device kernel's
                                       twin, bit for bit
  forced_align_rows(...)               the same for a padded batch, with the entry point's output conventions
  torchaudio_forced_align(...)         viterbi_fp32 behind torchaudio.functional.forced_align's signature (the stub
                                       tools/gen_golden_align.py gives the reference; torchaudio is not installed)
  brute_force(lp, targets, blank)      every valid path enumerated
  durations_chain(...)                 float64 forward -> fp32 Viterbi -> durations_from_labels
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

N_MELS, TOKENS = 80, 178
BLANK = TOKENS
SMALL_HIDDEN, SMALL_SEED = 80, 11
TDNN_KERNELS = (5, 3, 3)
# The seeded aligners give the blank a negative output bias: a trained aligner on pad-wrapped text puts the pad symbol, not
# the blank, on the leading silence, and torch_align's loop miscounts a path that STARTS with a blank (align_text.py:328-349).
BLANK_BIAS = -4.0


def aligner_weights(hidden=SMALL_HIDDEN, seed=SMALL_SEED, n_mels=N_MELS, tokens=TOKENS):
    g = torch.Generator().manual_seed(seed)

    def uni(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    P, cin = {}, n_mels
    for i, k in enumerate(TDNN_KERNELS):
        bound = (cin * k) ** -0.5  # torch's default Conv1d / Linear initialisation range
        P[f"encoder.layers.{i}.0.weight"] = uni((hidden, cin, k), bound * 3 ** 0.5)
        P[f"encoder.layers.{i}.0.bias"] = uni((hidden,), bound)
        P[f"encoder.layers.{i}.2.running_mean"] = 0.3 * torch.randn(hidden, generator=g) + 0.2
        P[f"encoder.layers.{i}.2.running_var"] = 0.25 + 0.5 * torch.rand(hidden, generator=g)
        P[f"encoder.layers.{i}.2.num_batches_tracked"] = torch.tensor(100 + i, dtype=torch.int64)
        cin = hidden
    for j in range(5):
        bound = hidden ** -0.5
        P[f"encoder.layers.3.ffn.{3 * j}.weight"] = uni((hidden, hidden), bound * 3 ** 0.5)
        P[f"encoder.layers.3.ffn.{3 * j}.bias"] = uni((hidden,), bound)
    bound = hidden ** -0.5
    P["encoder_output_layer.weight"] = uni((tokens + 1, hidden), bound * 3)  # log-probs that differ by a few nats
    b = uni((tokens + 1,), bound)
    b[tokens] = BLANK_BIAS
    P["encoder_output_layer.bias"] = b
    return P


def aligner_forward(P, mel, lengths, dtype=torch.float64):
    """mel [B, n_mels, T], lengths [B] -> log_probs [B, T, tokens + 1] in `dtype` (text_aligner.py:73-127, 209-274, eval mode;
    the three masks zero the frames at or beyond a row's length in front of each TDNN conv, nothing is masked after it)"""
    W = {k: v.to(dtype) for k, v in P.items() if v.is_floating_point()}
    x = mel.to(dtype)
    T = x.shape[2]
    mask = (torch.arange(T)[None, :] < lengths.reshape(-1, 1)).to(dtype)[:, None, :]
    for i, k in enumerate(TDNN_KERNELS):
        p = f"encoder.layers.{i}."
        x = F.conv1d(x * mask, W[p + "0.weight"], W[p + "0.bias"], padding=(k - 1) // 2)
        x = F.batch_norm(torch.relu(x), W[p + "2.running_mean"], W[p + "2.running_var"], None, None, False, 0.1, 1e-5)
    x = x.transpose(1, 2)
    y = x
    for j in range(5):
        y = torch.relu(F.linear(y, W[f"encoder.layers.3.ffn.{3 * j}.weight"], W[f"encoder.layers.3.ffn.{3 * j}.bias"]))
    y = y + x
    return F.log_softmax(F.linear(y, W["encoder_output_layer.weight"], W["encoder_output_layer.bias"]), dim=-1)


def repeats(targets):
    return sum(1 for i in range(1, len(targets)) if targets[i] == targets[i - 1])


def viterbi_fp32(lp, targets, blank):
    """lp [T, V1] -> (labels int32 [T], scores float32 [T], best total float32).  States blank, tok, blank, ..., blank;
    x0 = stay, x1 = from s - 1, x2 = from s - 2 (token states whose token differs from the previous token);
    x2 if x2 > x1 and x2 > x0, else x1 if x1 > x0 and x1 > x2, else x0; end in S - 1 if alpha[S - 1] > alpha[S - 2] else S - 2."""
    lp = np.ascontiguousarray(np.asarray(lp, dtype=np.float32))
    targets = [int(t) for t in targets]
    T, U = lp.shape[0], len(targets)
    S = 2 * U + 1
    if T < U + repeats(targets) or T < 1:
        raise ValueError("no alignment exists: input length < target length + repeats")
    cls = np.full(S, blank, dtype=np.int64)
    cls[1::2] = targets
    skip = np.zeros(S, dtype=bool)
    for i in range(1, U):
        skip[2 * i + 1] = targets[i] != targets[i - 1]
    ninf = np.float32(-np.inf)
    alpha = np.full(S, ninf, dtype=np.float32)
    alpha[:min(S, 2)] = lp[0, cls[:min(S, 2)]]
    back = np.zeros((T, S), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            x0 = alpha
            x1 = np.concatenate([[ninf], alpha[:-1]]).astype(np.float32)
            x2 = np.where(skip, np.concatenate([[ninf, ninf], alpha[:-2]])[:S], ninf).astype(np.float32)
            t2 = (x2 > x1) & (x2 > x0)
            t1 = ~t2 & (x1 > x0) & (x1 > x2)
            best = np.where(t2, x2, np.where(t1, x1, x0)).astype(np.float32)
            back[t] = 2 * t2 + t1
            alpha = (best + lp[t, cls]).astype(np.float32)
    s = S - 2 if (S >= 2 and not alpha[S - 1] > alpha[S - 2]) else S - 1
    total = alpha[s]
    labels = np.empty(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        labels[t] = cls[s]
        s -= int(back[t, s])
    return labels, lp[np.arange(T), labels], total


def forced_align_rows(log_probs, targets, input_lengths, target_lengths, blank):
    """[B, T, V1], [B, U], [B], [B] -> labels int32 [B, T] (-1 past a row's length), scores float32 [B, T] (0 there), status [B]
    (1: no alignment exists, the row is all -1 / 0)"""
    lp = log_probs.detach().cpu().float().numpy()
    B, T, _ = lp.shape
    labels = np.full((B, T), -1, dtype=np.int32)
    scores = np.zeros((B, T), dtype=np.float32)
    status = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n, u = int(input_lengths[b]), int(target_lengths[b])
        tg = [int(v) for v in targets[b, :u]]
        if n < u + repeats(tg):
            status[b] = 1
        elif n > 0:
            labels[b, :n], scores[b, :n], _ = viterbi_fp32(lp[b, :n], tg, blank)
    return torch.from_numpy(labels), torch.from_numpy(scores), torch.from_numpy(status)


def torchaudio_forced_align(log_probs, targets, input_lengths=None, target_lengths=None, blank=0):
    """torchaudio.functional.forced_align's signature and return convention for one utterance: ([1, T] labels, [1, T] scores)"""
    assert log_probs.shape[0] == 1 and targets.shape[0] == 1
    n = int(input_lengths[0]) if input_lengths is not None else log_probs.shape[1]
    u = int(target_lengths[0]) if target_lengths is not None else targets.shape[1]
    labels, scores, _ = viterbi_fp32(log_probs[0, :n].detach().cpu().float().numpy(), targets[0, :u].tolist(), blank)
    return torch.from_numpy(labels.astype(np.int64))[None], torch.from_numpy(scores.copy())[None]


def brute_force(lp, targets, blank):
    """max over EVERY valid state path (start in state 0 or 1, steps of 0 / 1 / allowed 2, end in S - 1 or S - 2) of the fp32
    sum of its log-probs in frame order -> (best total, the label paths that reach it)"""
    lp = np.asarray(lp, dtype=np.float32)
    targets = [int(t) for t in targets]
    T, U = lp.shape[0], len(targets)
    S = 2 * U + 1
    cls = [blank if s % 2 == 0 else targets[s // 2] for s in range(S)]
    skip = [s % 2 == 1 and s >= 3 and targets[s // 2] != targets[s // 2 - 1] for s in range(S)]
    best, arg = None, []
    for s0 in range(min(S, 2)):
        for steps in itertools.product((0, 1, 2), repeat=T - 1):
            s, path, ok = s0, [s0], True
            for d in steps:
                s += d
                if s >= S or (d == 2 and not skip[s]):
                    ok = False
                    break
                path.append(s)
            if not ok or s not in (S - 1, S - 2) or s < 0:
                continue
            total = np.float32(lp[0, cls[path[0]]])
            for t in range(1, T):
                total = np.float32(total + lp[t, cls[path[t]]])
            labels = [cls[q] for q in path]
            if best is None or total > best:
                best, arg = total, [labels]
            elif total == best and labels not in arg:
                arg.append(labels)
    return best, arg


def collapse(labels, blank):
    """CTC collapse: merge repeats, drop blanks"""
    out, prev = [], None
    for v in labels:
        v = int(v)
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return out


def random_targets(rs, U, tokens=TOKENS, repeat_every=0):
    """U tokens in [0, tokens); repeat_every > 0: every repeat_every-th token repeats its predecessor"""
    t = rs.randint(0, tokens, size=U).tolist()
    if repeat_every:
        for i in range(repeat_every, U, repeat_every):
            t[i] = t[i - 1]
    return t


def random_log_probs(rs, T, V1=TOKENS + 1, spread=3.0):
    x = torch.from_numpy(rs.standard_normal((T, V1)).astype(np.float32) * spread)
    return torch.log_softmax(x, dim=-1)


def durations_chain(P, mel, lengths, texts, text_lengths, blank=BLANK, log=lambda *_: None):
    """float64 forward -> fp32 Viterbi -> durations_from_labels for every row of a batch: list of [1, U_b]"""
    from stylish_tts_amd.align import durations_from_labels
    lp = aligner_forward(P, mel, lengths, torch.float64).float()
    labels, _, status = forced_align_rows(lp, texts, lengths, text_lengths, blank)
    assert not status.any()
    return [durations_from_labels(labels[b, :int(lengths[b])], texts[b:b + 1, :int(text_lengths[b])], blank, log=log)
            for b in range(lp.shape[0])]


# hand-made label paths for torch_align's loop (text, path): B = BLANK
_B = BLANK
LABEL_PATHS = {
    "plain": ([5, 9, 12], [5, 5, 9, 9, 9, 12]),
    "blank_inside": ([5, 9, 12], [5, _B, _B, 9, 12, _B, _B]),
    "leading_blank": ([5, 9, 12], [_B, _B, 5, 5, 9, 12, 12]),
    "repeat_with_blank": ([7, 7, 3], [7, 7, _B, 7, 3, 3]),
    "longer_than_sequence": ([5, 9], [5, _B, 9, 9, _B, 4, 4, _B]),
    "mismatch": ([5, 9, 12], [5, 5, 30, 30, 12, 12]),
}
