"""The `align` entry point on the reference's unchanged YAML files (train/cli.py:114-153 `align`,
train/dataprep/align_text.py): a trained `alignment_model.safetensors` + a dataset -> `alignment.safetensors` (the durations
`train` reads), `scores_val.txt` and `scores_train.txt`.  Inference only: training the aligner is `train_align.py`.

    python -m stylish_tts_amd.align CONFIG.yml --model-config MODEL.yml [--method torch] [-bs 8]

or `stylish_tts_amd.align.align(config_path, model_config_path, method, batch_size)` -- the reference command's arguments in
the reference command's order.

Per batch (one length bin, val split first, then train): wave -> mel (the `text_aligner` section's n_fft / win_length at hop
hop_length * coarse_multiplier, normalised) -> TextAligner -> log-probs [B, T, tokens + 1] -> CTC forced alignment against
the cleaned text (blank = tokens) -> frame labels [B, T] int32 + their log-probs; only the labels and scores (B * T * 8
bytes) go back to the host, where `durations_from_labels` -- the loop of `torch_align`, align_text.py:324-354 -- turns a
row's labels into the float [1, U] durations the file holds.  The score of a segment is `scores.exp().mean()` over its
frames (align_text.py:286).

The reference's `torch` method walks the dataset one utterance at a time; here `batch_size` rows of one length bin go
through every call.  A row's result does not depend on its neighbours: the convs see each row's own frames only, the
dynamic programme runs one workgroup per row.  `--method k2` needs the k2 package (and has another duration rule): refused.
"""
import ctypes as C
import os
import os.path as osp
import shutil
import time

import torch

from . import lib as L
from .manifest import text_aligner_manifest
from .modules import _HipModule, _f32, _no_autograd

ALIGNER_MEL = dict(n_fft=2048, win_length=1200)  # train/config/model.yml `text_aligner` section


def _log(msg):
    print(f"[stylish_tts_amd.align] {msg}", flush=True)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class TextAligner(_HipModule):
    """tdnn_blstm_ctc_model_base(n_mels, tokens) (text_aligner.py:33-45) in eval mode, with the reference's state_dict keys:
    `load_state_dict(load_file("alignment_model.safetensors"))` works unchanged.
    forward(mels [B, n_mels, T] -- channel-major, as calculate_mel returns them -- or, with time_major=True, the reference's
    [B, T, n_mels]; mel_lengths [B]) -> log_probs [B, T, tokens + 1] (the reference returns [T, B, K] and align_text.py:303
    rearranges it).  Frames at or beyond a row's length are zeroed in front of each TDNN conv, as text_aligner.py:221-225."""
    KIND = "text_aligner"

    def __init__(self, n_mels=80, tokens=178, hidden_dim=640):
        super().__init__()
        self.n_mels, self.tokens, self.hidden_dim = int(n_mels), int(tokens), int(hidden_dim)
        self._build(text_aligner_manifest(self.n_mels, self.tokens, self.hidden_dim))

    def enable_training(self):
        raise L.StyError("TextAligner: inference only (the training graph is alignment.TrainableTextAligner)")

    def set_train_opts(self, **kw):
        if kw.get("compute_bf16"):
            raise L.StyError("TextAligner: compute_bf16 is refused: the kind is inference-only and runs fp32 operands "
                             "(alignment decisions are arg-max decisions)")
        return super().set_train_opts(**kw)

    def forward(self, mels, mel_lengths, time_major=False):
        _no_autograd("TextAligner.forward")
        if mels.dim() != 3:
            raise L.StyError(f"TextAligner: mels must be [B, n_mels, T] (got {tuple(mels.shape)})")
        if time_major:
            mels = mels.transpose(1, 2)
        B, F, T = mels.shape
        if F != self.n_mels or tuple(mel_lengths.shape) != (B,) or T < 1:
            raise L.StyError(f"TextAligner: mels {tuple(mels.shape)} / mel_lengths {tuple(mel_lengths.shape)} do not fit "
                             f"[B, {self.n_mels}, T] / [B]")
        dev = mels.device
        lib = self._ensure(dev)
        x = _f32(mels, dev)
        ln = mel_lengths.to(dev, torch.int64).contiguous()
        out = torch.empty(B, T, self.tokens + 1, dtype=torch.float32, device=dev)
        need = C.c_size_t()
        L.check(lib.sty_aligner_workspace_bytes(self._handle, B, T, C.byref(need)))
        ws = self._workspace(need.value, dev)
        L.check(lib.sty_aligner_fwd(self._handle, B, T, L.ptr(x), L.ptr(ln), L.ptr(out), L.ptr(ws), ws.numel(), _stream(dev)))
        return out


@torch.no_grad()
def forced_align(log_probs, targets, input_lengths, target_lengths, blank):
    """torchaudio.functional.forced_align for a batch, on the device (sty_forced_align): log_probs [B, T, V1] fp32, targets
    [B, U], input_lengths / target_lengths [B] -> (labels [B, T] int32, scores [B, T] fp32), both on the device; frames at or
    beyond a row's input length hold label -1 and score 0.  Raises, naming the rows, where no alignment exists
    (input length < target length + adjacent repeats: torchaudio raises too) or a length / target is out of range."""
    if not log_probs.is_cuda:
        raise L.StyError("forced_align: log_probs must live on a HIP device (there is no CPU path)")
    if log_probs.dim() != 3 or targets.dim() != 2 or targets.shape[0] != log_probs.shape[0]:
        raise L.StyError(f"forced_align: log_probs {tuple(log_probs.shape)} / targets {tuple(targets.shape)} do not fit "
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
        raise L.StyError("forced_align: input_lengths / target_lengths must be [B]")
    labels = torch.empty(B, T, dtype=torch.int32, device=dev)
    scores = torch.empty(B, T, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    need = C.c_size_t()
    L.check(lib.sty_forced_align_workspace_bytes(B, T, U, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    L.check(lib.sty_forced_align(B, T, V1, U, L.ptr(lp), L.ptr(tg), L.ptr(il), L.ptr(tl), int(blank), L.ptr(labels),
                                 L.ptr(scores), L.ptr(status), L.ptr(ws), ws.numel(), _stream(dev)))
    st = status.cpu().tolist()
    if any(st):
        short = [i for i, s in enumerate(st) if s == 1]
        bad = [i for i, s in enumerate(st) if s not in (0, 1)]
        err = L.StyError("forced_align: " + "; ".join(
            ([f"row(s) {short}: input length is shorter than target length + adjacent repeats, no alignment exists"] if short
             else []) + ([f"row(s) {bad}: a length or a target token is out of range"] if bad else [])))
        err.status, err.labels, err.scores = st, labels, scores
        raise err
    return labels, scores


def durations_from_labels(labels, text, blank, log=print):
    """The loop of torch_align (align_text.py:324-354) on one row's frame labels (1-D, the valid frames only) and its text
    [1, U]: durations float [1, U].  A literal port, quirks included: `text_index` advances at the first token after a blank,
    also when the path STARTS with blanks -- the leading blanks then count for token 0 and the first token is compared with
    token 1; a path with more tokens than the text stops counting at the first frame past the end (first warning, `break`); a
    frame whose label is neither blank nor the current token is not counted (second warning)."""
    alignment = [int(v) for v in torch.as_tensor(labels).reshape(-1).tolist()]
    tokens = [int(v) for v in torch.as_tensor(text).reshape(1, -1)[0].tolist()]
    counts = [0] * len(tokens)
    text_index = 0
    last_text = alignment[0]
    was_blank = False
    for a in alignment:
        if a == blank:
            was_blank = True
        elif a != last_text or was_blank:
            text_index += 1
            last_text = a
            was_blank = False
        if text_index >= len(tokens):
            log("WARNING: alignment is longer than the sequence, likely an untrained model.")
            break
        if a == blank or a == tokens[text_index]:
            counts[text_index] += 1
        else:
            log("WARNING: the alignment doesn't match the sequence, likely an untrained model.")
    return torch.tensor([counts], dtype=torch.float)


def score_line(score, name):
    """one line of scores_val.txt / scores_train.txt (align_text.py:171-189)"""
    return str(score) + " " + name + "\n"


def _refuse_method(method):
    if method == "k2":
        raise L.StyError("align --method k2: the k2 package is not a dependency of this path (and its duration rule differs "
                         "from the torch method's, align_text.py:407-476); use --method torch")
    if method != "torch":
        raise NotImplementedError(method)


@torch.no_grad()
def calculate_alignments(lines, dataset, aligner, norm, to_mel, blank, batch_size, device, log=_log):
    """align_text.py:260-287 for one split, `batch_size` rows of one length bin per call -> ({name: [1, U]}, {name: score})"""
    from . import data as D
    from .frontend import calculate_mel
    time_bins, _ = dataset.time_bins()
    sampler = D.LengthBinSampler(time_bins, lambda key: int(batch_size), shuffle=False)
    loader = torch.utils.data.DataLoader(dataset, batch_sampler=sampler, num_workers=0,
                                         collate_fn=D.Collater(stage="alignment", hop_length=to_mel.hop_length))
    alignment_map, scores_map = {}, {}
    for waves, texts, text_lengths, paths, _, _ in loader:
        mels, mel_lengths = calculate_mel(waves.to(device), to_mel, norm.mel_log_mean, norm.mel_log_std)
        log_probs = aligner(mels, mel_lengths)
        labels, scores = forced_align(log_probs, texts.to(device), mel_lengths, text_lengths.to(device), blank)
        mean_scores = scores.exp().mean(dim=1).cpu().tolist()  # every row of a bin has the bin's frame count
        labels = labels.cpu()
        for i, name in enumerate(paths):
            n = int(text_lengths[i])
            alignment_map[name] = durations_from_labels(labels[i], texts[i:i + 1, :n], blank)
            scores_map[name] = mean_scores[i]
    return alignment_map, scores_map


def align_text(config, model_config, method, batch_size, *, device=None, log=_log):
    """align_text.py:92-201.  Everything that can be refused without a device is refused first."""
    from safetensors.torch import load_file, save_file
    from . import data as D
    from . import stage_io as IO
    from .frontend import MelSpec
    from .voicepack import _need_device
    _refuse_method(method)
    if int(batch_size) < 1:
        raise L.StyError("align: batch size must be at least 1")
    ds = config.dataset
    root = ds.path
    path = lambda p: osp.join(root, p)
    model_path = path(getattr(ds, "alignment_model_path", "alignment_model.safetensors"))
    for what, p in (("train_data", path(ds.train_data)), ("val_data", path(ds.val_data)), ("wav_path", path(ds.wav_path)),
                    ("alignment_model_path", model_path)):
        if not osp.exists(p):
            raise L.StyError(f"dataset.{what} not found at {p}")
    device = _need_device("the alignment pass", device)
    splits = {}
    for what in ("val_data", "train_data"):
        with open(path(ds[what]), encoding="utf-8") as f:
            splits[what] = [ln for ln in f.read().splitlines() if ln.strip()]
    # normalisation statistics through a temporary stage directory, as the reference's TrainContext("temp", ...) does
    out_dir = osp.join(root, "temp")
    norm = IO.NormalizationStats()
    IO.init_normalization(norm, out_dir, root, splits["train_data"], path(ds.wav_path), model_config, device=str(device),
                          log=log)
    ta = getattr(model_config, "text_aligner", None) or {}
    hop = model_config.hop_length * model_config.coarse_multiplier
    to_mel = MelSpec(int(ta.get("n_fft", ALIGNER_MEL["n_fft"])), int(ta.get("win_length", ALIGNER_MEL["win_length"])), hop)
    tokens = int(model_config.text_encoder.tokens)
    state = load_file(model_path)
    hidden = int(state["encoder_output_layer.weight"].shape[1])
    aligner = TextAligner(int(model_config.n_mels), tokens, hidden)
    aligner.load_state_dict(state)
    aligner = aligner.to(device).eval()
    symbols = getattr(model_config, "symbol", None)
    results, seen = {}, 0
    t0 = time.perf_counter()
    for what, scores_file in (("val_data", "scores_val.txt"), ("train_data", "scores_train.txt")):
        dataset = D.SampleDataset(data_list=splits[what], root_path=path(ds.wav_path), pitch_path=None, alignment_path="",
                                  text_cleaner=D.TextCleaner(symbols), sample_rate=model_config.sample_rate,
                                  hop_length=model_config.hop_length, coarse_multiplier=model_config.coarse_multiplier)
        durations, scores = calculate_alignments(splits[what], dataset, aligner, norm, to_mel, tokens, batch_size, device, log)
        with open(path(scores_file), "w", encoding="utf-8") as f:
            for name in scores.keys():
                f.write(score_line(scores[name], name))
        results[what] = durations
        seen += len(durations)
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    result = results["val_data"] | results["train_data"]
    out = path(ds.alignment_path)
    if osp.exists(out):
        os.unlink(out)
    save_file(result, out)
    shutil.rmtree(out_dir)
    log(f"{seen} utterances in {dt:.2f} s ({seen / max(dt, 1e-9):.1f} utterances/s at batch size {int(batch_size)}); wrote {out}")
    return result


def align(config_path, model_config_path, method="torch", batch_size=8, **kw):
    """train/cli.py:114-153 `align`: same arguments, same order."""
    from .config import load_config_yaml
    from .train import get_model_config
    _refuse_method(method)
    kw.get("log", _log)("Calculate alignment...")
    config = load_config_yaml(config_path)
    model_config = get_model_config(model_config_path)
    return align_text(config, model_config, method, batch_size, **kw)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m stylish_tts_amd.align", description=__doc__.split("\n\n")[0])
    ap.add_argument("config_path")
    ap.add_argument("--model-config", dest="model_config_path", default="")
    ap.add_argument("--method", default="torch", help="torch (k2 is refused: the package is not a dependency)")
    ap.add_argument("-bs", "--batch-size", dest="batch_size", type=int, default=8)
    a = ap.parse_args(argv)
    align(a.config_path, a.model_config_path, a.method, a.batch_size)


if __name__ == "__main__":
    main()
