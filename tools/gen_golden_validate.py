"""Golden fixture of the duration stage's validation samples by RUNNING THE REFERENCE'S OWN `validate_duration`
(train/stage_type.py:557-633; build container only):

    python tools/gen_golden_validate.py

The stand-in `train` object, the models, their key-named weights and the inputs are those of tools/gen_golden_stages.py (same
seeds, every model in .eval(), oracle/frontend.py standing in for the absent torchaudio), so `duration.log.*` of
tests/golden/stages_small.safetensors are the losses this call logs.  validate_duration then synthesises every utterance of the
batch at B = 1 from its PREDICTED durations: prediction_to_duration -> duration_to_alignment -> pitch_energy_predictor with the
pe_style_encoder style -> speech_predictor with voiced = pred_pitch > 20.

Writes tests/golden/validate_small.safetensors, data only:
  duration [B, L]            the predicted durations
  frames [B]                 round(sum duration) per utterance -- the length of its alignment
  audio_sub.<i>, audio_norm.<i>, audio_len.<i>   a strided sample of utterance i's audio (at most SUB values; stride 1, the whole
                             waveform, when it has no more than that), its L2 norm, its sample count
  prior.<i> [1, 300 T_i]     the harmonic source's output of that call (SineGen's phase accumulation is what the HIP path pins
                             with prior_override, as every audio parity test does)
  noise_seed.<i>             torch.manual_seed(...) in front of utterance i's speech predictor call; the test regenerates the
                             draw (rand[1, 9] then randn[1, 300 T_i, 9], generator.py:345, 440)
and the log of the call.  The generator asserts that no predicted duration total lies within 1e-3 of a rounding boundary of
duration_to_alignment (the frame count is round(sum d)); otherwise a last-bit difference would change a frame count and the test
would compare audio of different lengths.  It holds with the stage fixture's weight seeds (duration predictor 3, its style
encoder 7: totals 42 and 38 frames); should a change of the inputs break it, pick other seeds for those two models here.
"""
import os
import sys
import types

import torch
from safetensors.torch import load_file, save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_import  # noqa: E402
from gen_golden_stages import _Mel, test_audio  # noqa: E402

OUT = os.environ.get("STY_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
G = os.path.join(ROOT, "tests", "golden")
NOISE_SEED = 123
SUB = 16384  # the fixture's utterances (42 and 38 frames) fit whole: the test can then take the mel-L1 bound too
MARGIN = 1e-3


def sub(t, n=SUB):
    f = t.detach().flatten()
    return f if f.numel() <= n else f[::f.numel() // n][:n].clone()


def main():
    mc = ref_import.model_config()
    for name in ("soundfile", "librosa", "librosa.filters", "tqdm", "tensorboard", "torch.utils.tensorboard",
                 "torch.utils.tensorboard.writer", "k2"):
        if name not in sys.modules:
            ref_import._stub(name, tqdm=lambda x, *a, **k: x, mel=None, SummaryWriter=object)
    ref_import._stub("stylish_tts.train.train_context", TrainContext=object)
    from oracle import frontend
    import torchaudio

    class MelScale(torch.nn.Module):
        def __init__(self, n_mels=128, sample_rate=24000, f_min=0.0, f_max=None, n_stft=201, norm=None, mel_scale="htk"):
            super().__init__()
            self.register_buffer("fb", frontend.mel_filterbank(n_stft, n_mels, sample_rate))

        def forward(self, spec):
            return torch.matmul(spec.transpose(-1, -2), self.fb).transpose(-1, -2)

    torchaudio.transforms.MelScale = MelScale
    from stylish_tts.lib.config_loader import load_config_yaml
    from stylish_tts.train import stage_type as ST
    from stylish_tts.train.losses import DurationLoss
    from stylish_tts.train.models.duration_predictor import DurationPredictor
    from stylish_tts.train.models.mel_style_encoder import MelStyleEncoder, PitchStyleEncoder
    from stylish_tts.train.models.pitch_energy_predictor import PitchEnergyPredictor
    from stylish_tts.train.models.speech_predictor import SpeechPredictor
    from stylish_tts.train.utils import DurationProcessor
    from oracle.manifest import (duration_predictor_manifest, pitch_energy_predictor_manifest,
                                 pitch_style_encoder_manifest, speech_predictor_manifest, style_encoder_manifest)
    from oracle.weights import fill_state_dict
    from tests.cases import make_case

    torch.set_num_threads(8)
    cfg = load_config_yaml("/root/reference/config/config.yml")
    cs = make_case("sp_small")
    B, T = cs["pitch"].shape
    audio_gt = test_audio(B, 300 * T, 21)
    stage_fx = load_file(os.path.join(G, "stages_small.safetensors"))
    assert torch.equal(audio_gt, stage_fx["audio_gt"])  # the stage fixture's inputs

    def filled(mod, manifest, seed, strict=True):
        miss, unexp = mod.load_state_dict(fill_state_dict(manifest, seed), strict=False)
        assert not unexp and (not strict and all(".stft." in k for k in miss) or not miss), (miss, unexp)
        return mod.eval()

    se_args = (mc.style_encoder.n_mels, mc.style_dim, mc.style_encoder.max_channels, mc.style_encoder.skip_downsample)
    model = ref_import._Munch(
        duration_style_encoder=filled(MelStyleEncoder(*se_args), style_encoder_manifest(), 7),
        duration_predictor=filled(DurationPredictor(style_dim=mc.style_dim, inter_dim=mc.inter_dim,
                                                    text_config=mc.text_encoder, duration_config=mc.duration_predictor),
                                  duration_predictor_manifest(), 3),
        speech_style_encoder=filled(MelStyleEncoder(*se_args), style_encoder_manifest(), 0),
        speech_predictor=filled(SpeechPredictor(mc), speech_predictor_manifest(), 0, strict=False),
        pe_style_encoder=filled(PitchStyleEncoder(*se_args, coarse_multiplier=mc.coarse_multiplier),
                                pitch_style_encoder_manifest(), 5),
        pitch_energy_predictor=filled(PitchEnergyPredictor(style_dim=mc.style_dim, inter_dim=mc.pitch_energy_predictor.inter_dim,
                                                           text_config=mc.text_encoder, duration_config=mc.duration_predictor,
                                                           pitch_energy_config=mc.pitch_energy_predictor),
                                      pitch_energy_predictor_manifest(), 4))
    weights = stage_fx["class_weights"]
    train = types.SimpleNamespace(
        model=model, model_config=mc, config=cfg, logger=None, writer=None,
        to_mel=_Mel(mc.n_fft, mc.win_length, mc.hop_length),
        to_style_mel=_Mel(mc.style_encoder.n_fft, mc.style_encoder.win_length, mc.style_encoder.hop_length),
        normalization=types.SimpleNamespace(mel_log_mean=-4.0, mel_log_std=4.0),
        duration_processor=DurationProcessor(mc.duration_predictor.duration_classes, mc.duration_predictor.max_duration),
        duration_loss=DurationLoss(class_count=mc.duration_predictor.duration_classes, weight=weights))
    batch = types.SimpleNamespace(audio_gt=audio_gt, text=cs["texts"], text_length=cs["text_lengths"], pitch=cs["pitch"],
                                  alignment=cs["durations"].unsqueeze(1))

    # every B = 1 speech predictor call: seed the global generator in front of it (SineGen draws from it), keep the source's output
    calls, priors = [0], []

    def seed_call(_mod, _args):
        torch.manual_seed(NOISE_SEED + calls[0])
        calls[0] += 1

    h1 = model.speech_predictor.register_forward_pre_hook(seed_call)
    h2 = model.speech_predictor.generator.basegen.m_source.register_forward_hook(
        lambda _m, _i, o: priors.append(o[0].detach().squeeze(2).clone()))
    captured = {}
    orig = train.duration_processor.prediction_to_duration

    def keep_duration(pred, lengths):
        captured["duration"] = orig(pred, lengths)
        return captured["duration"]

    train.duration_processor.prediction_to_duration = keep_duration
    log, _, results, _ = ST.validate_duration(batch, train)
    h1.remove()
    h2.remove()
    duration = captured["duration"].detach()
    assert len(results) == B and len(priors) == B
    out = {"duration": duration.contiguous()}
    frames = []
    for i in range(B):
        total = float(duration[i].sum())
        frac = total - int(total)
        assert abs(frac - 0.5) >= MARGIN, f"utterance {i}: duration total {total} is within {MARGIN} of a rounding boundary"
        n = int(round(total))
        assert results[i].numel() == 300 * n, (results[i].shape, n)
        frames.append(n)
        out[f"audio_sub.{i}"] = sub(results[i])
        out[f"audio_norm.{i}"] = results[i].detach().norm().reshape(1)
        out[f"audio_len.{i}"] = torch.tensor([float(results[i].numel())])
        out[f"prior.{i}"] = priors[i].contiguous()
        out[f"noise_seed.{i}"] = torch.tensor([float(NOISE_SEED + i)])
    out["frames"] = torch.tensor(frames, dtype=torch.float32)
    for k, v in log.metrics.items():
        out["log." + k] = torch.as_tensor(float(v)).reshape(1)
        ref = stage_fx["duration.log." + k].item()
        assert abs(float(v) - ref) <= 1e-6 * abs(ref), (k, float(v), ref)  # the eval-mode losses ARE the stage fixture's
    print("validate_duration:", {k: round(float(v), 6) for k, v in log.metrics.items()}, "frames", frames)
    path = os.path.join(OUT, "validate_small.safetensors")
    save_file({k: v.contiguous().float() for k, v in out.items()}, path,
              metadata={"audio_seed": "21", "case": "sp_small", "weights": "as stages_small", "noise_seed": str(NOISE_SEED),
                        "mel": "oracle/frontend.py stands in for torchaudio (absent)"})
    print("size KB", os.path.getsize(path) // 1024)


if __name__ == "__main__":
    main()
