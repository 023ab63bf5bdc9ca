"""Golden fixture of the reference's voicepack builder (train/voicepack.py) by RUNNING THE REFERENCE (build container only;
sentence_transformers, torchaudio, tqdm, soundfile and librosa are absent and stubbed).

    python tools/gen_golden_voicepack.py

Writes tests/golden/voicepack_small.safetensors + voicepack_small.json.  Only data is written.

(a) `make_static` with its `calculate_style` patched to hand out prepared rows (tests/voicepack_cases.make_rows: regenerated
    from a seed by the tests, only the text lengths and the reference's output are stored), on two histograms of text
    lengths: "wrap" (`lower` goes negative for the short rows) and "inside" (every window resolves inside [0, 512); many
    rows of that pack are identical, so its unique rows and a row index are stored).  A second run per histogram on one-hot
    bucket indicators reads the CONTENT of each of the reference's windows off its own output (first / last non-empty bucket,
    rows held) -- json `windows`; json `ref_to_f64_max` is the reference's (fp32 averaging) largest distance from the float64
    mean over those windows.  json `exit_cases`: whether the reference's make_static exits on the small histograms of
    tests/voicepack_cases.EXIT_CASES.
(b) `calculate_style` on four utterances in two length bins (padded by this package's loader, which tests/golden/data_small
    pins to the reference's; waves stored as the PCM16 integers they are), the three encoders under the key-named fill of
    oracle/weights.py, the two mel transforms = the oracle front end (torchaudio boundary: parity unpinned).
"""
import json
import os
import sys
import tempfile
import types
import wave

import numpy as np
import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NORM = (-3.2, 3.7)  # mel_log_mean, mel_log_std of the checkpoint in (b): not the defaults, so that they matter
SEEDS = dict(speech_style_encoder=0, pe_style_encoder=5, duration_style_encoder=7)
SR, HOP = 24000, 300


def run_make_static(RV, rows, lengths):
    """the reference's make_static over (rows, lengths) at batch size 1, in order; None where it exits"""
    RV.calculate_style = lambda batch, state, to_mel, to_style_mel, device: rows[batch[5]]
    it = ((i, (None, None, torch.tensor([int(n)]), None, None, i)) for i, n in enumerate(lengths))
    try:
        return RV.make_static(it, None, None, None, "cpu")
    except SystemExit:
        return None


def utterances(tmp):
    """four short synthetic utterances, two in length bin 1 (80 frames) and two in bin 2 (100 frames), through this package's
    loader: padded waves [4 x N_bin], pitch [4 x frames]"""
    from stylish_tts_amd import data as D
    rs = np.random.RandomState(77)
    os.makedirs(os.path.join(tmp, "wav"))
    lines, pitch = [], {}
    for i, nsamp in enumerate((12300, 17500, 18100, 23900)):
        frames_raw = nsamp // HOP + 1
        f0 = np.interp(np.linspace(0, 3, frames_raw), np.arange(4), rs.uniform(90, 260, size=4))
        a = rs.randint(0, frames_raw)
        f0[a:a + frames_raw // 6] = 0
        f0s = np.repeat(f0, HOP)[:nsamp]
        ph = 2 * np.pi * np.cumsum(f0s) / SR
        x = sum(np.sin((h + 1) * ph) / (h + 1) for h in range(8)) * 0.15 * (f0s > 0) + 0.01 * rs.standard_normal(nsamp)
        name = f"{i}.wav"
        with wave.open(os.path.join(tmp, "wav", name), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(SR)
            f.writeframes(np.clip(np.round(x * 32767.0), -32768, 32767).astype("<i2").tobytes())
        fc = D.get_frame_count(D.get_time_bin(nsamp, HOP))
        pad = (fc * HOP - nsamp) // 2 // HOP
        p = np.zeros(fc, np.float32)
        m = min(frames_raw, fc - pad)
        p[pad:pad + m] = f0[:m]
        pitch[name] = torch.from_numpy(p)[None]
        lines.append(f"{name}|{'ɑ' * (5 + 3 * i)}|0|utterance {i}")
    save_file(pitch, os.path.join(tmp, "pitch.safetensors"))
    ds = D.SampleDataset(data_list=lines, root_path=os.path.join(tmp, "wav"), pitch_path=os.path.join(tmp, "pitch.safetensors"),
                         alignment_path=None)
    col = D.Collater(stage="voicepack", hop_length=HOP)
    return [col([ds[i] for i in idx]) for idx in ((0, 1), (2, 3))]


def main():
    mc = ref_import.model_config()
    for name in ("soundfile", "librosa", "librosa.filters", "tqdm", "sentence_transformers", "prettytable"):
        if name not in sys.modules:
            ref_import._stub(name, tqdm=lambda x, *a, **k: x, mel=None, SentenceTransformer=object, PrettyTable=object)
    import torchaudio
    torchaudio.transforms.MelSpectrogram = object  # (make_voicepack's transforms: not run here, see (b))
    from stylish_tts.train import voicepack as RV
    from stylish_tts.train.models.mel_style_encoder import MelStyleEncoder, PitchStyleEncoder
    from oracle import frontend as ofe
    from oracle.manifest import pitch_style_encoder_manifest, style_encoder_manifest
    from oracle.weights import fill_state_dict
    from tests import voicepack_cases as VC

    torch.set_num_threads(8)
    reference_calculate_style = RV.calculate_style
    out, meta = {}, {"histograms": {}, "exit_cases": {}, "norm": list(NORM), "seeds": SEEDS}
    # ---- (a) ---------------------------------------------------------------------------------------------------------
    for name in VC.HISTOGRAMS:
        rows, lengths = VC.make_rows(name)
        pack = run_make_static(RV, rows, lengths.tolist())
        assert pack is not None and pack.shape == (VC.ROWS, VC.DIM) and pack.dtype == torch.float32
        onehot = torch.nn.functional.one_hot(lengths - 1, VC.ROWS).double()
        share = run_make_static(RV, onehot, lengths.tolist())  # share[i, b] = rows of bucket b / rows held, per window
        counts = VC.counts_of(lengths)
        contents = []
        for i in range(VC.ROWS):
            nz = torch.nonzero(share[i]).flatten().tolist()
            held = round(counts[nz[0]] / float(share[i, nz[0]]))
            assert held == sum(counts[b] for b in nz) and nz == [b for b in range(nz[0], nz[-1] + 1) if counts[b]], (i, nz)
            contents.append([nz[0], nz[-1], held])
        dist = (pack.double() - VC.float64_means(rows, lengths, contents)).abs().max().item()
        # a window whose content no symmetric window [i - k, i + k] with k <= i explains: `lower` went negative and wrapped
        reach = [max(i - c[0], c[1] - i, 0) for i, c in enumerate(contents)]
        wraps = any(k > i or sum(counts[max(i - k, 0):i + k + 1]) != c[2] for (i, c), k in zip(enumerate(contents), reach))
        meta["histograms"][name] = dict(n=len(lengths), windows=contents, ref_to_f64_max=dist, wraps=wraps)
        out[f"{name}.text_lengths"] = lengths
        if name == "inside":
            uniq, inverse = torch.unique(pack, dim=0, return_inverse=True)
            assert torch.equal(uniq[inverse], pack)
            out[f"{name}.pack_unique"], out[f"{name}.pack_index"] = uniq.contiguous(), inverse.to(torch.int32)
        else:
            out[f"{name}.pack"] = pack.contiguous()
        print(name, "rows", len(lengths), "reference to float64", dist, "wraps", wraps)
    assert meta["histograms"]["wrap"]["wraps"] and not meta["histograms"]["inside"]["wraps"]
    for name in VC.EXIT_CASES:
        lengths = VC.exit_case_lengths(name)
        meta["exit_cases"][name] = run_make_static(RV, torch.zeros(len(lengths), 4), lengths) is None
    print("exit cases", meta["exit_cases"])
    # ---- (b) ---------------------------------------------------------------------------------------------------------
    se_args = (mc.style_encoder.n_mels, mc.style_dim, mc.style_encoder.max_channels, mc.style_encoder.skip_downsample)

    def filled(mod, manifest, seed):
        miss, unexp = mod.load_state_dict(fill_state_dict(manifest, seed), strict=False)
        assert not miss and not unexp, (miss, unexp)
        return mod.eval()

    state = types.SimpleNamespace(
        norm=types.SimpleNamespace(mel_log_mean=NORM[0], mel_log_std=NORM[1]),
        model=types.SimpleNamespace(
            speech_style_encoder=filled(MelStyleEncoder(*se_args), style_encoder_manifest(), SEEDS["speech_style_encoder"]),
            pe_style_encoder=filled(PitchStyleEncoder(*se_args, coarse_multiplier=mc.coarse_multiplier),
                                    pitch_style_encoder_manifest(), SEEDS["pe_style_encoder"]),
            duration_style_encoder=filled(MelStyleEncoder(*se_args), style_encoder_manifest(), SEEDS["duration_style_encoder"])))
    to_mel = lambda w: ofe.mel_spectrogram(w, mc.n_fft, mc.win_length, mc.hop_length, mc.n_mels, mc.sample_rate)
    se = mc.style_encoder
    to_style_mel = lambda w: ofe.mel_spectrogram(w, se.n_fft, se.win_length, se.hop_length, se.n_mels, mc.sample_rate)
    with tempfile.TemporaryDirectory() as tmp:
        batches = utterances(tmp)
    for b, batch in enumerate(batches):
        waves, pitches = batch[0], batch[4]
        pcm = (waves * 32768.0).round()
        assert torch.equal(pcm / 32768.0, waves) and pcm.abs().max() <= 32767
        rows = []
        for i in range(waves.shape[0]):  # the reference's pass: batch size 1
            one = tuple(x[i:i + 1] if torch.is_tensor(x) else x for x in batch)
            rows.append(reference_calculate_style(one, state, to_mel, to_style_mel, "cpu"))
        out[f"bin{b}.waves_pcm16"], out[f"bin{b}.pitch"] = pcm.to(torch.int16), pitches.contiguous()
        out[f"bin{b}.styles"] = torch.stack(rows).contiguous()
        print("bin", b, "waves", tuple(waves.shape), "styles", tuple(out[f"bin{b}.styles"].shape))
    path = os.path.join(OUT, "voicepack_small.safetensors")
    save_file(out, path)
    with open(os.path.join(OUT, "voicepack_small.json"), "w") as f:
        json.dump(meta, f)
    print("size KB", os.path.getsize(path) // 1024, "+ json", os.path.getsize(os.path.join(OUT, "voicepack_small.json")) // 1024)


if __name__ == "__main__":
    main()
