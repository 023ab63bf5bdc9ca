"""The `voicepack` entry point on the reference's unchanged YAML files (train/cli.py:414-428 `voicepack`,
train/voicepack.py:12-171): a trained checkpoint + the train split -> the table of style vectors the inference graph takes
as inputs (`speech_style`, `pe_style`, `duration_style` of ExportModel; consumed by stylish_tts_amd.speak).

    python -m stylish_tts_amd.voicepack CONFIG.yml --model-config MODEL.yml --voicepack OUT.safetensors --checkpoint DIR

or `stylish_tts_amd.voicepack.voicepack(config_path, dynamic, model_config_path, voicepack_path, checkpoint)` -- the reference
command's arguments in the reference command's order.

Per utterance (`calculate_style`, voicepack.py:139-170): energy mel (n_fft 512) -> log energy; style mel (the `style_encoder`
section); speech / pitch-energy / duration style encoders -> one row [192] = speech | pe | duration.  The reference walks the
dataset at batch size 1; the dataset pads every wave to its length bin's frame count, so a row computed in a batch of one
bin is the same function of the same padded wave, and the pass here runs whole bins at `batch_size`.

The table (`make_static`, voicepack.py:116-136): rows are filed under text_length - 1 in 512 buckets; row i of the pack is
the mean of the rows in a window that starts at [i, i + 1) and widens by one on both sides until it holds `min_styles`
(100) rows.  KEPT QUIRK: `lower` goes negative and is then used as a Python slice start, i.e. it wraps to the END of the
table -- for a dataset whose texts are 16..200 tokens long the pack's first rows are the mean over the LONGEST texts, not
the shortest -- and the process gives up only once `lower < 0 and upper > 512` with the window still short.  That arithmetic
is reproduced exactly (`resolve_windows`), so a voicepack made here from a reference checkpoint is the one the reference
would have made; there is no "fixed" mode.  The sums are float64 on the device (csrc/voicepack.hip), each row of the pack is
rounded to fp32 once; the reference averages in fp32.

NOT KEPT: tts/cli.py:78 picks row `max(511, min(2, len(tokens)))` with tokens of shape [1, n], which is 511 for every
input.  `style_index(n_tokens)` returns the bucket make_static files an utterance of that length under,
min(max(n_tokens, 1), 512) - 1; `reference_index=True` returns 511.

The dynamic voicepack (voicepack.py:36-49, 97-113) keys rows by a sentence-transformers embedding of the plain text; that
package is not a dependency of this path: `dynamic=True` raises.
"""
import ctypes as C
import os.path as osp
import time

import torch

from . import lib as L
from .config import check_supported, load_config_yaml

ROWS, STYLE_ROW = 512, 192  # voicepack.py:117 (512 buckets); three style vectors of model.yml's style_dim 64
MIN_STYLES = 100            # voicepack.py:127


def _log(msg):
    print(f"[stylish_tts_amd.voicepack] {msg}", flush=True)


def _refuse_dynamic(what):
    raise L.StyError(f"{what}: the dynamic voicepack needs the `sentence_transformers` package (an SBERT embedding per plain "
                     "text, train/voicepack.py:36-49), which is not a dependency of this path; the static voicepack is built")


def style_index(n_tokens, reference_index=False, rows=ROWS):
    """Row of the static pack for an utterance of n_tokens tokens (pad symbols included, as TextCleaner returns them): the
    bucket make_static files such an utterance under.  reference_index=True: what tts/cli.py:78 computes, rows - 1 always."""
    if reference_index:
        return rows - 1
    return min(max(int(n_tokens), 1), rows) - 1


def _slice_bounds(lower, upper, rows):
    """list[lower:upper] of a list of `rows` items, as Python normalises it (upper >= 1 here)"""
    lo = lower if lower >= 0 else max(0, rows + lower)
    return lo, min(upper, rows)


def resolve_windows(counts, min_styles=MIN_STYLES):
    """voicepack.py:123-130 on the bucket counts alone (host only): for every row i the window [lower, upper) starts at
    [i, i + 1) and widens by one on both sides while it holds fewer than min_styles rows; `styles[lower:upper]` is a Python
    slice, so a negative `lower` wraps to the end of the table.  Returns (lo, hi): the normalised windows, lo[i] < hi[i].
    Raises where the reference exits: right after a widening that leaves lower < 0 and upper > rows."""
    counts = [int(c) for c in counts]
    rows = len(counts)
    if min_styles < 1:
        raise L.StyError("resolve_windows: min_styles must be at least 1")
    prefix = [0]
    for c in counts:
        prefix.append(prefix[-1] + c)

    def held(lower, upper):
        lo, hi = _slice_bounds(lower, upper, rows)
        return prefix[hi] - prefix[lo] if lo < hi else 0

    los, his = [], []
    for i in range(rows):
        lower, upper = i, i + 1
        while held(lower, upper) < min_styles:
            lower -= 1
            upper += 1
            if lower < 0 and upper > rows:
                raise L.StyError(f"Need at least {min_styles} styles to make a voicepack (row {i}: the window ran off both ends "
                                 f"of the table; {prefix[-1]} styles in all)")
        lo, hi = _slice_bounds(lower, upper, rows)
        los.append(lo)
        his.append(hi)
    return los, his


class StylePack:
    """The table of make_static on the device: `.add(styles [n, dim] on the device, text_lengths [n] on the HOST)` files a
    batch, `.finalize()` -> pack [rows, dim] fp32 on the device.  min_styles is the reference's constant (100), exposed so
    that a small dataset can make a pack.  Nothing but `counts` (rows * 8 bytes) is read back, once, in finalize."""

    def __init__(self, rows=ROWS, dim=STYLE_ROW, min_styles=MIN_STYLES):
        self.rows, self.dim, self.min_styles = int(rows), int(dim), int(min_styles)
        self.sums = self.counts = None
        self.windows = None

    def add(self, styles, text_lengths):
        if not styles.is_cuda:
            raise L.StyError("StylePack.add: styles must be on a HIP device (there is no CPU path)")
        if text_lengths.is_cuda:
            raise L.StyError("StylePack.add: text_lengths is checked on the host: pass the collated CPU tensor")
        n = styles.shape[0]
        if styles.dim() != 2 or styles.shape[1] != self.dim or tuple(text_lengths.shape) != (n,):
            raise L.StyError(f"StylePack.add: styles {tuple(styles.shape)} / text_lengths {tuple(text_lengths.shape)} do not fit "
                             f"[n, {self.dim}] / [n]")
        tl = text_lengths.to(torch.int64)
        if n and (int(tl.min()) < 1 or int(tl.max()) > self.rows):
            raise L.StyError(f"StylePack.add: text length outside 1..{self.rows} ({int(tl.min())}..{int(tl.max())})")
        lib = L.load()
        dev = styles.device
        if self.sums is None:
            self.sums = torch.zeros(self.rows, self.dim, dtype=torch.float64, device=dev)
            self.counts = torch.zeros(self.rows, dtype=torch.int64, device=dev)
        styles = styles.detach().to(torch.float32).contiguous()
        tl = tl.contiguous().to(dev, non_blocking=True)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(lib.sty_pack_accumulate(n, self.dim, self.rows, L.ptr(styles), L.ptr(tl), L.ptr(self.sums),
                                        L.ptr(self.counts), st))

    def finalize(self):
        if self.sums is None:
            raise L.StyError(f"Need at least {self.min_styles} styles to make a voicepack (none were added)")
        lib = L.load()
        dev = self.sums.device
        lo, hi = resolve_windows(self.counts.cpu().tolist(), self.min_styles)  # the one read-back of the pass
        self.windows = (lo, hi)
        lo_d = torch.tensor(lo, dtype=torch.int32).to(dev)
        hi_d = torch.tensor(hi, dtype=torch.int32).to(dev)
        pack = torch.empty(self.rows, self.dim, dtype=torch.float32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(lib.sty_pack_finalize(self.rows, self.dim, L.ptr(self.sums), L.ptr(self.counts), L.ptr(lo_d), L.ptr(hi_d),
                                      L.ptr(pack), st))
        return pack


STYLE_KEYS = ("speech_style_encoder", "pe_style_encoder", "duration_style_encoder")  # the row's order (voicepack.py:160-167)


@torch.no_grad()
def calculate_style(waves, pitches, models, norm, to_mel=None, to_style_mel=None):
    """voicepack.py:139-170 for a batch of one length bin: waves [B, N], pitches [B, N // hop] on the device, models = the
    three style encoders under their build_model keys, norm = the checkpoint's NormalizationStats -> [B, 192]."""
    from .frontend import MelSpec, calculate_mel
    if not waves.is_cuda:
        raise L.StyError("calculate_style: no HIP device tensor (there is no CPU path)")
    to_mel = to_mel or MelSpec(512, 512, 300)
    to_style_mel = to_style_mel or MelSpec(2048, 1200, 300)
    mean, std = norm.mel_log_mean, norm.mel_log_std
    _, _, energy = calculate_mel(waves, to_mel, mean, std, want_energy=True)  # log(||mel||_2 over bins + 1e-9)
    style_mel, _ = calculate_mel(waves, to_style_mel, mean, std)
    speech = models["speech_style_encoder"](style_mel.unsqueeze(1))
    pe = models["pe_style_encoder"](style_mel, pitches.to(waves.device), energy)
    duration = models["duration_style_encoder"](style_mel.unsqueeze(1))
    return torch.cat([speech, pe, duration], dim=1)


def _model_registry(model_config, device):
    """only the lazy model registry of the training context (build_model's keys, the shells' constructors)"""
    from .train import TrainContext

    class _Ctx(TrainContext):
        def __init__(self):
            self.model_config, self.device, self.models = model_config, device, {}

    return _Ctx()


def _need_device(what, device):
    if not torch.cuda.is_available():
        raise L.StyError(f"no HIP device: {what} runs the models on the device and there is no CPU path in this package")
    device = torch.device(device or "cuda:0")
    torch.cuda.set_device(device)
    return device


def make_voicepack(config, model_config, dynamic, checkpoint, *, batch_size=32, min_styles=MIN_STYLES, device=None, log=_log):
    """voicepack.py:12-94 -> the static pack [512, 192] (fp32, on the device).  Everything that can be refused without a
    device is refused first."""
    from . import data as D
    from . import stage_io as IO
    from .frontend import MelSpec
    check_supported(model_config)
    if dynamic:
        _refuse_dynamic("make_voicepack(dynamic=True)")
    norm = IO.NormalizationStats()
    if not osp.isdir(checkpoint):
        raise L.StyError(f"checkpoint directory {checkpoint} not found")
    IO.load_checkpoint(checkpoint, {}, normalization=norm)
    if norm.frames <= 0:  # voicepack.py:15-16
        raise L.StyError(f"No normalization state found in {checkpoint} (frames = {norm.frames}). Cannot generate voicepack.")
    device = _need_device("the voicepack pass", device)
    ctx = _model_registry(model_config, device)
    models = {k: ctx.model(k) for k in STYLE_KEYS}
    IO.load_checkpoint(checkpoint, models)  # (a missing model file is a StyError that names it)
    for m in models.values():
        m.eval()
    ds = config.dataset
    path = lambda p: osp.join(ds.path, p)
    for what in ("train_data", "wav_path", "pitch_path"):
        if not osp.exists(path(ds[what])):
            raise L.StyError(f"dataset.{what} not found at {path(ds[what])}")
    with open(path(ds.train_data), encoding="utf-8") as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    symbols = getattr(model_config, "symbol", None)
    dataset = D.SampleDataset(data_list=lines, root_path=path(ds.wav_path), pitch_path=path(ds.pitch_path),
                              alignment_path=path(ds.alignment_path), text_cleaner=D.TextCleaner(symbols),
                              sample_rate=model_config.sample_rate, hop_length=model_config.hop_length,
                              coarse_multiplier=model_config.coarse_multiplier)
    time_bins, _ = dataset.time_bins()
    sampler = D.LengthBinSampler(time_bins, lambda key: int(batch_size), shuffle=False)
    loader = torch.utils.data.DataLoader(dataset, batch_sampler=sampler, num_workers=0,
                                         collate_fn=D.Collater(stage="voicepack", hop_length=model_config.hop_length))
    to_mel = MelSpec(model_config.n_fft, model_config.win_length, model_config.hop_length)
    se = model_config.style_encoder
    to_style_mel = MelSpec(se.n_fft, se.win_length, se.hop_length)
    pack = StylePack(ROWS, 3 * int(model_config.style_dim), min_styles)
    t0, seen = time.perf_counter(), 0
    for waves, _, text_lengths, _, pitches, _ in loader:
        styles = calculate_style(waves.to(device), pitches.to(device), models, norm, to_mel, to_style_mel)
        pack.add(styles, text_lengths)
        seen += waves.shape[0]
    result = pack.finalize()
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    log(f"{seen} utterances in {dt:.2f} s ({seen / max(dt, 1e-9):.1f} utterances/s at batch size {int(batch_size)}, "
        f"{len(time_bins)} length bins)")
    return result


def voicepack(config_path, dynamic, model_config_path, voicepack_path, checkpoint, **kw):
    """train/cli.py:414-428 `voicepack`: same arguments, same order; writes {"voicepack_static": [512, 192]}."""
    from safetensors.torch import save_file
    from .train import get_model_config
    log = kw.get("log", _log)
    log("Generate dynamic voicepack..." if dynamic else "Generate static voicepack...")
    config = load_config_yaml(config_path)
    model_config = get_model_config(model_config_path)
    result = make_voicepack(config, model_config, dynamic, checkpoint, **kw)
    save_file({"voicepack_static": result.cpu().contiguous()}, voicepack_path)
    log(f"wrote {voicepack_path}")
    return result


def read_voicepack(path):
    """tts/cli.py:38-47: the static pack of a voicepack file as a CPU tensor [rows, 192]."""
    from safetensors import safe_open
    if not osp.isfile(path):
        raise L.StyError(f"voicepack file {path} not found")
    with safe_open(path, framework="pt", device="cpu") as f:
        keys = set(f.keys())
        if "voicepack_dynamic" in keys:
            _refuse_dynamic(f"{path} holds `voicepack_dynamic`")
        if "voicepack_static" not in keys:
            raise L.StyError(f"Could not find voicepack key in {path} (keys: {sorted(keys)})")
        pack = f.get_tensor("voicepack_static")
    if pack.dim() != 2 or pack.shape[1] != STYLE_ROW:
        raise L.StyError(f"{path}: voicepack_static has shape {tuple(pack.shape)}, expected [rows, {STYLE_ROW}]")
    return pack.float()


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m stylish_tts_amd.voicepack", description=__doc__.split("\n\n")[0])
    ap.add_argument("config_path")
    ap.add_argument("--dynamic", action="store_true", help="refused: needs sentence_transformers")
    ap.add_argument("--model-config", dest="model_config_path", default="")
    ap.add_argument("--voicepack", dest="voicepack_path", required=True, help="path to write the voicepack to")
    ap.add_argument("--checkpoint", required=True, help="checkpoint directory with the three style encoders")
    ap.add_argument("--batch-size", type=int, default=32)
    a = ap.parse_args(argv)
    voicepack(a.config_path, a.dynamic, a.model_config_path, a.voicepack_path, a.checkpoint, batch_size=a.batch_size)


if __name__ == "__main__":
    main()
