"""The `pitch` entry point on the reference's unchanged YAML files (train/cli.py:205-243 `pitch --method rmvpe`,
train/dataprep/pitch_extractor.py, train/dataprep/rmvpe/): a dataset + RMVPE weights -> `<dataset.path>/<pitch_path>`
(`pitch.safetensors`), the file every training stage reads.

    python -m stylish_tts_amd.pitch CONFIG.yml --model-config MODEL.yml --rmvpe rmvpe.safetensors [-bs 8] [-k 8] [--method rmvpe]

or `stylish_tts_amd.pitch.pitch(config_path, model_config_path, workers, method, rmvpe_path=..., batch_size=8)`.

`--rmvpe` is required and names a local file: `rmvpe.safetensors` of the `stylish-tts/pitch_extractor` repository (the
reference fetches it with hf_hub_download, pitch_extractor.py:51-53).  This command never downloads anything.

Per wave (pitch_extractor.py:137-149, rmvpe/inference.py:45-62): 24 kHz -> Resample(24000, 16000, lowpass_filter_width=128) ->
log-mel (1024-point, hop 200 = 16000 // (24000 // 300), 128 HTK mel bins, 30-8000 Hz, magnitude) -> the deep U-Net, BiGRU and
salience head on the frame axis reflected to a multiple of 32 -> the arg-max-centred local average -> f0 in Hz; `f0[:-1]` as
float32 [1, frame_count], NaN -> -10.  All of it runs on the device: RMVPE.mel / mel2hidden / decode below.

The list walk is `audio_list` (train/dataprep/align_text.py:594-618): the validation list first, then the training list; a
wave shorter than 0.25 s is skipped with a line; every other wave is centre-padded with zeros to its length bin's
frame_count * 300 samples.  The reference walks one wave at a time over `-k` worker threads; here every wave of a length bin
has the same padded length, so `-bs` of them go through each call and no raggedness arises.  A row's result does not depend
on its neighbours (tests/test_pitch_gpu.py).  `-k` is accepted for command-line compatibility and unused.

`--method pyworld` (the reference's default: CPU harvest / dio + stonemask) needs the pyworld package, which is not a
dependency of this path: refused with NotImplementedError, as `align --method k2` is.  Viterbi decoding (`use_viterbi`, which
the reference's command never turns on) is not built.

The front end restates torchaudio's resampler and librosa's mel basis from their documented closed forms; neither package is
part of this image: PARITY UNPINNED at that boundary (tests/pitch_cases.py has the float64 restatement the kernels are held
to).  No trained RMVPE weights were available where this was built: the network is held to the reference's own class on
key-filled weights, the decode to the reference's own function; that the f0 of real speech is right is not shown by a test.
"""
import ctypes as C
import os.path as osp
import time

import numpy as np
import torch

from . import lib as L
from .manifest import rmvpe_manifest
from .modules import _HipModule, _f32, _no_autograd

N_MELS, N_CLASS, MIN_FRAMES = 128, 360, 17
ZERO_VALUE = -10.0  # pitch_extractor.py:138


def _log(msg):
    print(f"[stylish_tts_amd.pitch] {msg}", flush=True)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def mel_frames(samples):
    """frames of the log-mel of `samples` samples at 24 kHz: ceil(2 N / 3) // 200 + 1"""
    return ((2 * int(samples) + 2) // 3) // 200 + 1


class RMVPE(_HipModule):
    """E2E0(n_blocks, 1, (2, 2), 5, inter_layers, 1, en_out_channels) (rmvpe/model.py:49-86) in eval mode with the reference's
    state_dict keys: `load_state_dict(load_file("rmvpe.safetensors"))` works unchanged.  The methods are the reference's RMVPE
    class (rmvpe/inference.py:12-62) for a batch of equally long waves:
      mel(audio [B, N] at 24 kHz) -> log-mel [B, 128, n];  mel2hidden(mel) -> salience [B, n, 360];
      decode(hidden, thred=0.03) -> f0 [B, n] in Hz;  infer_from_audio(audio) = decode(mel2hidden(mel(audio)))."""
    KIND = "rmvpe"

    def __init__(self, n_blocks=4, inter_layers=4, en_out_channels=16):
        super().__init__()
        self.n_blocks, self.inter_layers, self.en_out_channels = int(n_blocks), int(inter_layers), int(en_out_channels)
        self._build(rmvpe_manifest(self.n_blocks, self.inter_layers, self.en_out_channels))

    @classmethod
    def from_state_dict(cls, state):
        """the module whose n_blocks / inter_layers / en_out_channels are those of a reference-layout state_dict"""
        count = lambda fmt: next(i for i in range(1, 1 << 10) if fmt.format(i) not in state)
        m = cls(count("unet.encoder.layers.0.conv.{}.conv.0.weight"), count("unet.intermediate.layers.{}.conv.0.conv.0.weight"),
                int(state["cnn.weight"].shape[1]))
        m.load_state_dict(state, strict=True)
        return m

    def enable_training(self):
        raise L.StyError("RMVPE: inference only (training the pitch extractor is out of scope)")

    def set_train_opts(self, **kw):
        if kw.get("compute_bf16"):
            raise L.StyError("RMVPE: compute_bf16 is refused: the kind is inference-only and runs fp32 operands (pitch values "
                             "hang on an arg-max)")
        return super().set_train_opts(**kw)

    @staticmethod
    def mel(audio):
        _no_autograd("RMVPE.mel")
        if audio.dim() != 2 or not audio.is_cuda:
            raise L.StyError(f"RMVPE.mel: audio must be [B, N] on a HIP device (got {tuple(audio.shape)} on {audio.device}); "
                             "there is no CPU path")
        lib = L.load()
        dev = audio.device
        B, N = audio.shape
        x = _f32(audio, dev)
        need = C.c_size_t()
        L.check(lib.sty_rmvpe_mel_workspace_bytes(B, N, C.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        out = torch.empty(B, N_MELS, mel_frames(N), dtype=torch.float32, device=dev)
        L.check(lib.sty_rmvpe_mel_fwd(B, N, L.ptr(x), L.ptr(out), L.ptr(ws), ws.numel(), _stream(dev)))
        return out

    def mel2hidden(self, mel):
        _no_autograd("RMVPE.mel2hidden")
        if mel.dim() != 3 or mel.shape[1] != N_MELS:
            raise L.StyError(f"RMVPE.mel2hidden: mel must be [B, {N_MELS}, n] (got {tuple(mel.shape)})")
        B, _, n = mel.shape
        if n < MIN_FRAMES:
            raise L.StyError(f"RMVPE.mel2hidden: {n} frames cannot be reflected to a multiple of 32 (at least {MIN_FRAMES})")
        dev = mel.device
        lib = self._ensure(dev)
        x = _f32(mel, dev)
        out = torch.empty(B, n, N_CLASS, dtype=torch.float32, device=dev)
        need = C.c_size_t()
        L.check(lib.sty_rmvpe_workspace_bytes(self._handle, B, n, C.byref(need)))
        ws = self._workspace(need.value, dev)
        L.check(lib.sty_rmvpe_fwd(self._handle, B, n, L.ptr(x), L.ptr(out), L.ptr(ws), ws.numel(), _stream(dev)))
        return out

    forward = mel2hidden

    @staticmethod
    def decode(hidden, thred=0.03, use_viterbi=False):
        if use_viterbi:
            raise NotImplementedError("RMVPE.decode(use_viterbi=True): Viterbi decoding is not built")
        if hidden.dim() != 3 or hidden.shape[2] != N_CLASS or not hidden.is_cuda:
            raise L.StyError(f"RMVPE.decode: hidden must be [B, n, {N_CLASS}] on a HIP device (got {tuple(hidden.shape)} on "
                             f"{hidden.device})")
        lib = L.load()
        dev = hidden.device
        B, n, _ = hidden.shape
        h = _f32(hidden, dev)
        f0 = torch.empty(B, n, dtype=torch.float32, device=dev)
        L.check(lib.sty_rmvpe_decode(B, n, L.ptr(h), float(thred), L.ptr(f0), _stream(dev)))
        return f0

    def infer_from_audio(self, audio, thred=0.03):
        return self.decode(self.mel2hidden(self.mel(audio)), thred=thred)


def _refuse_method(method):
    if method == "pyworld":
        raise NotImplementedError("pitch --method pyworld: the pyworld package is not a dependency of this path; use "
                                  "--method rmvpe")
    if method != "rmvpe":
        raise NotImplementedError(method)


def audio_list(list_path, wav_dir, coarse_hop_length, sample_rate=24000, log=_log):
    """align_text.py:594-618: (name, frame_count, wave padded to frame_count * coarse_hop_length) of every line of a list"""
    from . import data as D
    with open(list_path, encoding="utf-8") as f:
        for line in f:
            if not line.strip():
                continue
            name = line.split("|")[0]
            wave, sr = D.read_wav(osp.join(wav_dir, name))
            if sr != sample_rate:
                raise ValueError(f"{name}: sample rate {sr}, expected {sample_rate} (resample the dataset first)")
            time_bin = D.get_time_bin(wave.shape[0], coarse_hop_length)
            if time_bin == -1:
                log(f"Skipping {name}: Too short")
                continue
            frame_count = D.get_frame_count(time_bin)
            total = frame_count * coarse_hop_length
            pad_start = (total - wave.shape[0]) // 2
            pad_end = total - wave.shape[0] - pad_start
            yield name, frame_count, np.concatenate([np.zeros([pad_start]), wave, np.zeros([pad_end])], axis=0)


def to_pitch_entry(f0_row):
    """pitch_extractor.py:137-149: f0 [frame_count + 1] -> float32 [1, frame_count], NaN -> -10"""
    pitch = f0_row.detach().float().cpu().reshape(1, -1)[:, :-1].clone()
    pitch[torch.isnan(pitch)] = ZERO_VALUE
    return pitch


@torch.no_grad()
def calculate_pitch_set(list_path, wav_dir, model, coarse_hop_length, batch_size, device, sample_rate=24000, log=_log):
    """one list -> ({name: [1, frame_count]}, seconds of audio): `batch_size` waves of one length bin per call"""
    result, pending, seconds = {}, {}, 0.0

    def flush(frames):
        names, waves = zip(*pending.pop(frames))
        audio = torch.from_numpy(np.stack(waves)).float().to(device)
        f0 = model.infer_from_audio(audio)
        for i, name in enumerate(names):
            result[name] = to_pitch_entry(f0[i])

    for name, frames, wave in audio_list(list_path, wav_dir, coarse_hop_length, sample_rate, log):
        seconds += wave.shape[0] / sample_rate
        pending.setdefault(frames, []).append((name, wave))
        if len(pending[frames]) >= batch_size:
            flush(frames)
    for frames in sorted(pending):
        flush(frames)
    return result, seconds


def calculate_pitch(config, model_config, method, workers, *, rmvpe_path, batch_size=8, device=None, log=_log):
    """pitch_extractor.py:19-42.  Everything that can be refused without a device is refused first."""
    from safetensors.torch import load_file, save_file
    from .voicepack import _need_device
    _refuse_method(method)
    if not rmvpe_path:
        raise L.StyError("pitch: --rmvpe is required: the path of rmvpe.safetensors (repository stylish-tts/pitch_extractor); "
                         "this command never downloads anything")
    if int(batch_size) < 1:
        raise L.StyError("pitch: batch size must be at least 1")
    ds = config.dataset
    root = ds.path
    path = lambda p: osp.join(root, p)
    for what, p in (("train_data", path(ds.train_data)), ("val_data", path(ds.val_data)), ("wav_path", path(ds.wav_path)),
                    ("--rmvpe", rmvpe_path)):
        if not osp.exists(p):
            raise L.StyError(f"{what if what.startswith('--') else 'dataset.' + what} not found at {p}")
    device = _need_device("the pitch pass", device)
    model = RMVPE.from_state_dict(load_file(rmvpe_path)).to(device).eval()
    hop = model_config.hop_length * model_config.coarse_multiplier
    if model_config.sample_rate // model_config.hop_length != 80:
        raise L.StyError("pitch: the RMVPE front end is built for 80 frames per second (hop 200 at 16 kHz; sample_rate 24000, "
                         "hop_length 300)")
    result, seconds = {}, 0.0
    t0 = time.perf_counter()
    for what in ("val_data", "train_data"):
        part, sec = calculate_pitch_set(path(ds[what]), path(ds.wav_path), model, hop, int(batch_size), device,
                                        model_config.sample_rate, log)
        result |= part
        seconds += sec
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    out = path(ds.pitch_path)
    save_file(result, out)
    log(f"{len(result)} utterances, {seconds:.1f} s of audio in {dt:.2f} s ({seconds / max(dt, 1e-9):.1f} audio-seconds per "
        f"second at batch size {int(batch_size)}); wrote {out}")
    return result


def pitch(config_path, model_config_path, workers=8, method="rmvpe", **kw):
    """train/cli.py:205-243 `pitch`: the reference command's arguments in the reference command's order."""
    from .config import load_config_yaml
    from .train import get_model_config
    _refuse_method(method)
    if not kw.get("rmvpe_path"):
        raise L.StyError("pitch: --rmvpe is required: the path of rmvpe.safetensors (repository stylish-tts/pitch_extractor); "
                         "this command never downloads anything")
    kw.get("log", _log)("Calculate pitch...")
    config = load_config_yaml(config_path)
    model_config = get_model_config(model_config_path)
    return calculate_pitch(config, model_config, method, workers, **kw)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m stylish_tts_amd.pitch", description=__doc__.split("\n\n")[0])
    ap.add_argument("config_path")
    ap.add_argument("-mc", "--model-config", dest="model_config_path", default="")
    ap.add_argument("-k", "--workers", type=int, default=8, help="accepted for compatibility with the reference; unused")
    ap.add_argument("--method", default="rmvpe", help="rmvpe (pyworld is refused: the package is not a dependency)")
    ap.add_argument("--rmvpe", dest="rmvpe_path", default="", help="rmvpe.safetensors of stylish-tts/pitch_extractor (required)")
    ap.add_argument("-bs", "--batch-size", dest="batch_size", type=int, default=8)
    a = ap.parse_args(argv)
    pitch(a.config_path, a.model_config_path, a.workers, a.method, rmvpe_path=a.rmvpe_path, batch_size=a.batch_size)


if __name__ == "__main__":
    main()
