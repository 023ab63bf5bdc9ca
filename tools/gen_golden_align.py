"""Golden fixtures of the alignment stage by RUNNING THE REFERENCE (build container only): its TextAligner
(train/models/text_aligner.py) and its `torch_align` / `calculate_alignment_single` (train/dataprep/align_text.py).

    python tools/gen_golden_align.py

Writes tests/golden/align_small.safetensors + align_small.json and tests/golden/manifest_text_aligner.json.  Only data is
written.  torchaudio is not installed: `torchaudio.functional.forced_align` is the fp32 restatement of
tests/align_cases.py behind torchaudio's signature (its tie rule is therefore unpinned), and the mel transform of
the end-to-end utterances is the oracle front end, as in tools/gen_golden_voicepack.py.

(a) the reference model at hidden_dim 80 under tests/align_cases.aligner_weights (seeded; running_mean != 0, running_var != 1)
    on an input [3, 66, 80] with lengths [66, 40, 1]: its fp32 log-probs and, from a .double() copy, its float64 log-probs;
(b) `torch_align` on the hand-made label paths of align_cases.LABEL_PATHS (the stub hands the path out): the durations and
    which warnings it printed;
(c) `calculate_alignment_single` on short synthetic utterances: the normalised mel it fed the model (so that the check is of
    the aligner and the dynamic programme, not of the mel front end), the text and the durations.  An utterance is kept only
    if the reference's label path does not move under 10 draws of uniform noise of the forward gate's size
    (max(1e-5 max|log-probs|, 4 x the reference's own fp32-to-float64 distance)) added to its log-probs.
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NORM = (-3.1, 3.6)
SR, HOP = 24000, 300


def reference_model(RT, AC, hidden, seed):
    m = RT.tdnn_blstm_ctc_model(input_dim=AC.N_MELS, num_symbols=AC.TOKENS, hidden_dim=hidden, drop_out=0.1,
                                tdnn_blstm_spec=[("tdnn", 5, 1, 1), ("tdnn", 3, 1, 1), ("tdnn", 3, 1, 1), ("ffn", 5)])
    miss, unexp = m.load_state_dict(AC.aligner_weights(hidden, seed), strict=True)
    assert not miss and not unexp
    return m.eval()


def main():
    ref_import.install()
    for name in ("soundfile", "librosa", "librosa.filters", "prettytable", "k2", "tensorboard", "torch.utils.tensorboard",
                 "torch.utils.tensorboard.writer"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                ref_import._stub(name, mel=None, PrettyTable=object, SummaryWriter=object)
    import torchaudio
    torchaudio.transforms.MelSpectrogram = object
    from tests import align_cases as AC
    torchaudio.functional.forced_align = AC.torchaudio_forced_align
    from stylish_tts.lib.text_utils import TextCleaner
    from stylish_tts.train.dataprep import align_text as RA
    from stylish_tts.train.models import text_aligner as RT
    from oracle import frontend as ofe
    from stylish_tts_amd import data as D

    torch.set_num_threads(8)
    mc = ref_import.model_config()
    out, meta = {}, {"norm": list(NORM), "seed": AC.SMALL_SEED, "hidden": AC.SMALL_HIDDEN}
    # ---- manifest at the default width ------------------------------------------------------------------------------
    full = RT.tdnn_blstm_ctc_model_base(mc.n_mels, mc.text_encoder.tokens)
    with open(os.path.join(OUT, "manifest_text_aligner.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in full.state_dict().items()}, f, indent=0)
    # ---- (a) --------------------------------------------------------------------------------------------------------
    model = reference_model(RT, AC, AC.SMALL_HIDDEN, AC.SMALL_SEED)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 66, AC.N_MELS, generator=g)  # the reference's layout [B, T, n_mels]
    lengths = torch.tensor([66, 40, 1])
    with torch.no_grad():
        lp32 = model(x, lengths)[0].permute(1, 0, 2).contiguous()
        lp64 = model.double()(x.double(), lengths)[0].permute(1, 0, 2).contiguous()
        model.float()
    out["fwd.input"], out["fwd.lengths"] = x.contiguous(), lengths
    out["fwd.log_probs_f32"], out["fwd.log_probs_f64"] = lp32, lp64
    meta["fwd_ref_f32_to_f64"] = (lp32.double() - lp64).abs().max().item()
    print("forward: max|lp|", lp64.abs().max().item(), "fp32 to float64", meta["fwd_ref_f32_to_f64"])
    # ---- (b) --------------------------------------------------------------------------------------------------------
    cfg = types.SimpleNamespace(text_encoder=types.SimpleNamespace(tokens=AC.BLANK))
    meta["label_paths"] = {}
    for name, (text, path) in AC.LABEL_PATHS.items():
        torchaudio.functional.forced_align = lambda **kw: (torch.tensor([path]), torch.zeros(1, len(path)))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            dur, _ = RA.torch_align(torch.zeros(1), torch.tensor([text]), None, None, None, cfg, name)
        out[f"paths.{name}.durations"] = dur.contiguous()
        meta["label_paths"][name] = dict(longer=buf.getvalue().count("longer than the sequence"),
                                         mismatch=buf.getvalue().count("doesn't match the sequence"))
        print(name, dur.tolist(), meta["label_paths"][name])
    torchaudio.functional.forced_align = AC.torchaudio_forced_align
    # ---- (c) --------------------------------------------------------------------------------------------------------
    train = types.SimpleNamespace(
        to_align_mel=lambda w: ofe.mel_spectrogram(w, mc.text_aligner.n_fft, mc.text_aligner.win_length,
                                                   mc.hop_length * mc.coarse_multiplier, mc.text_aligner.n_mels, mc.sample_rate),
        normalization=types.SimpleNamespace(mel_log_mean=NORM[0], mel_log_std=NORM[1]),
        text_cleaner=TextCleaner(mc.symbol))
    rs = np.random.RandomState(5)
    ipa = [c for c in D.SYMBOLS["letters_ipa"] if c.isalpha()][:60]
    gate = max(1e-5 * lp64.abs().max().item(), 4 * meta["fwd_ref_f32_to_f64"])
    kept = 0
    captured = {}
    real_calculate_mel = RA.calculate_mel

    def spy_mel(*a):
        captured["mel"], captured["len"] = real_calculate_mel(*a)
        return captured["mel"], captured["len"]

    RA.calculate_mel = spy_mel
    for i in range(12):
        if kept == 3:
            break
        nsamp = int(rs.randint(6300, 17700))
        f0 = np.interp(np.linspace(0, 3, nsamp), np.arange(4), rs.uniform(90, 260, size=4))
        ph = 2 * np.pi * np.cumsum(f0) / SR
        wave = sum(np.sin((h + 1) * ph) / (h + 1) for h in range(8)) * 0.15 + 0.01 * rs.standard_normal(nsamp)
        wave = np.clip(np.round(wave * 32767.0), -32768, 32767) / 32768.0
        fc = D.get_frame_count(D.get_time_bin(nsamp, HOP))
        pad = (fc * HOP - nsamp) // 2
        wave = np.concatenate([np.zeros(pad), wave, np.zeros(fc * HOP - nsamp - pad)])  # as audio_list pads it
        n_ph = int(rs.randint(4, 14))
        text = "".join(ipa[j] for j in rs.randint(0, len(ipa), size=n_ph))
        if i % 2:
            text = text[:2] + text[1] + text[2:]  # an adjacent repeat
        buf = io.StringIO()
        with torch.no_grad(), contextlib.redirect_stdout(buf):
            dur, scores = RA.calculate_alignment_single(train, model, mc, f"{i}.wav", text, wave, "cpu")
        tokens = torch.tensor([train.text_cleaner(text)])
        mel, n = captured["mel"], int(captured["len"][0])
        with torch.no_grad():
            lp = model(mel.transpose(1, 2), captured["len"])[0].permute(1, 0, 2)
        base, _ = AC.torchaudio_forced_align(lp, tokens, blank=AC.BLANK)
        stable = True
        gn = torch.Generator().manual_seed(100 + i)
        for _ in range(10):
            noisy = lp + (torch.rand(lp.shape, generator=gn) * 2 - 1) * gate
            stable = stable and torch.equal(AC.torchaudio_forced_align(noisy, tokens, blank=AC.BLANK)[0], base)
        print(f"utterance {i}: frames {n} tokens {tokens.shape[1]} stable {stable} warnings {len(buf.getvalue().splitlines())} "
              f"sum {dur.sum().item()}")
        if not stable or buf.getvalue():
            continue
        out[f"e2e.{kept}.mel"] = mel[0].contiguous()
        out[f"e2e.{kept}.text"] = tokens[0].contiguous()
        out[f"e2e.{kept}.durations"] = dur.contiguous()
        out[f"e2e.{kept}.score"] = scores.exp().mean().reshape(1)
        kept += 1
    assert kept == 3, kept
    meta["e2e"], meta["gate"] = kept, gate
    path = os.path.join(OUT, "align_small.safetensors")
    save_file(out, path)
    with open(os.path.join(OUT, "align_small.json"), "w") as f:
        json.dump(meta, f)
    print("size KB", os.path.getsize(path) // 1024)
    assert os.path.getsize(path) < 700 * 1024


if __name__ == "__main__":
    main()
