"""`speak`: phoneme lines -> a wav, from a checkpoint directory plus a voicepack, with every model on the HIP path (the
reference's tts/cli.py:32-96 `speak_document` runs the exported ONNX file under onnxruntime; here the same graph is
stylish_tts_amd.ExportModel on the models of a checkpoint).

    python -m stylish_tts_amd.speak CHECKPOINT VOICEPACK INFILE OUTFILE --model-config MODEL.yml [--reference-index]
                                    [--compute {fp32,bf16,bf16x3}]

INFILE holds one `phonemes|plain text` line per utterance (tts/cli.py:62-66; phoneme input only, as the reference).  Per
line: TextCleaner -> the pack's row for that token count (voicepack.style_index; --reference-index: row 511 for every
line, which is what tts/cli.py:78 computes) -> ExportModel.forward with seed = the line's index -> -25 LUFS
(loudness.normalize) -> * 32768 -> int16.  The reference's `.astype(np.int16)` WRAPS a sample beyond full scale to the
other sign; here such a sample SATURATES.  The utterances are concatenated into one 24 kHz PCM16 wav (stdlib `wave`).  An
utterance shorter than one 0.4 s loudness block is written un-normalised, with a logged warning (pyloudnorm raises there).

--compute: fp32 (default) multiplies fp32 operands; bf16 rounds the operands of the dense convs / Linears of the three models
to bf16 (set_train_opts(compute_bf16=True): fastest, outside the fp32 parity gates); bf16x3 keeps fp32 accuracy and runs the
speech predictor's 32-channel vocoder convs on the bf16 matrix cores with every operand split into three bf16 pieces
(SpeechPredictor.set_fp32_split).
"""
import wave

import numpy as np
import torch

from . import lib as L
from .config import check_supported

TARGET_LUFS = -25.0  # tts/cli.py:87
COMPUTE_MODES = ("fp32", "bf16", "bf16x3")
SPEAK_KEYS = ("speech_predictor", "pitch_energy_predictor", "duration_predictor")


def _log(msg):
    print(f"[stylish_tts_amd.speak] {msg}", flush=True)


def to_int16(audio):
    """float audio -> int16 as `np.multiply(audio, 32768).astype(np.int16)` (tts/cli.py:88) for every sample inside full
    scale (truncation towards zero), saturating outside it"""
    return np.clip(np.multiply(audio, 32768.0), -32768.0, 32767.0).astype(np.int16)


class Speaker:
    """The three inference models of a checkpoint directory in ExportModel + the static voicepack split 64 / 64 / 64
    (tts/cli.py:49-51)."""

    def __init__(self, checkpoint, model_config_path, voicepack_path, device=None, compute="fp32"):
        import stylish_tts_amd as S
        from . import stage_io as IO
        from .data import TextCleaner
        from .train import get_model_config
        from .voicepack import _model_registry, _need_device, read_voicepack
        if compute not in COMPUTE_MODES:
            raise L.StyError(f"speak: compute mode {compute!r} is none of {', '.join(COMPUTE_MODES)}")
        self.compute = compute
        mc = self.model_config = check_supported(get_model_config(model_config_path))
        pack = read_voicepack(voicepack_path)  # (refuses a dynamic pack and a file without a voicepack key)
        self.device = _need_device("speak", device)
        ctx = _model_registry(mc, self.device)
        models = {k: ctx.model(k) for k in SPEAK_KEYS}
        IO.load_checkpoint(checkpoint, models)
        if compute == "bf16":
            for m in models.values():
                m.set_train_opts(compute_bf16=True)
        elif compute == "bf16x3":  # the speech predictor alone has the split mode; the other two models stay fp32
            models["speech_predictor"].set_fp32_split(True)
        self.model = S.ExportModel(class_count=mc.duration_predictor.duration_classes,
                                   max_dur=mc.duration_predictor.max_duration, coarse_multiplier=mc.coarse_multiplier,
                                   **models).eval()
        self.pack = pack.to(self.device)
        sd = int(mc.style_dim)
        self.speech_pack, self.pe_pack, self.duration_pack = (self.pack[:, i * sd:(i + 1) * sd] for i in range(3))
        self.text_cleaner = TextCleaner(getattr(mc, "symbol", None))
        self.sample_rate = int(mc.sample_rate)

    def tokenize(self, phonemes):
        return self.text_cleaner(phonemes)

    def styles(self, n_tokens, reference_index=False):
        from .voicepack import style_index
        i = style_index(n_tokens, reference_index, rows=self.pack.shape[0])
        return self.speech_pack[i:i + 1], self.pe_pack[i:i + 1], self.duration_pack[i:i + 1]

    def speak(self, phonemes, *, seed, reference_index=False):
        """one utterance -> float32 audio [samples] (numpy, on the host), not normalised"""
        tokens = self.tokenize(phonemes)
        texts = torch.tensor([tokens], dtype=torch.int64, device=self.device)
        text_lengths = torch.tensor([len(tokens)], dtype=torch.int64, device=self.device)
        speech, pe, duration = self.styles(len(tokens), reference_index)
        audio = self.model(texts, text_lengths, speech, pe, duration, seed=int(seed))
        return audio.reshape(-1).float().cpu().numpy()


def read_lines(infile):
    """[(line index, phonemes)] of the non-blank lines"""
    out = []
    with open(infile, "r", encoding="utf-8") as f:
        for i, line in enumerate(f):
            if not line.strip():
                continue
            fields = line.strip().split("|")
            if len(fields) < 2:
                raise L.StyError(f"{infile} line {i + 1}: expected `phonemes|plain text`")
            out.append((i, fields[0]))
    return out


def speak_document(infile, outfile, speaker, *, reference_index=False, target_lufs=TARGET_LUFS, log=_log):
    """tts/cli.py:32-96.  Returns the int16 segments (one per utterance) that were concatenated into `outfile`."""
    from .loudness import normalize
    segments = []
    for i, phonemes in read_lines(infile):
        audio = speaker.speak(phonemes, seed=i, reference_index=reference_index)
        audio = normalize(audio, target_lufs, speaker.sample_rate, log=log)
        segments.append(to_int16(audio))
    if not segments:
        raise L.StyError(f"{infile}: no utterances")
    with wave.open(outfile, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(speaker.sample_rate)
        f.writeframes(np.concatenate(segments).astype("<i2").tobytes())
    log(f"wrote {len(segments)} utterances, {sum(len(s) for s in segments) / speaker.sample_rate:.2f} s, to {outfile}")
    return segments


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m stylish_tts_amd.speak", description=__doc__.split("\n\n")[0])
    ap.add_argument("checkpoint", help="checkpoint directory with the duration, pitch / energy and speech predictors")
    ap.add_argument("voicepack", help="file written by python -m stylish_tts_amd.voicepack")
    ap.add_argument("infile")
    ap.add_argument("outfile")
    ap.add_argument("--model-config", dest="model_config_path", default="")
    ap.add_argument("--reference-index", dest="reference_index", action="store_true",
                    help="row 511 of the voicepack for every line, as the reference's speak computes it")
    ap.add_argument("--compute", choices=COMPUTE_MODES, default="fp32",
                    help="operand mode: fp32; bf16 (rounded operands, all three models); bf16x3 (fp32 accuracy on the bf16 "
                         "matrix cores for the speech predictor's 32-channel vocoder convs)")
    a = ap.parse_args(argv)
    _log(f"compute mode {a.compute}")
    speak_document(a.infile, a.outfile, Speaker(a.checkpoint, a.model_config_path, a.voicepack, compute=a.compute),
                   reference_index=a.reference_index)


if __name__ == "__main__":
    main()
