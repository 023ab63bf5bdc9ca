"""Host side of `voicepack` / `speak` (no GPU): the window arithmetic of the reference's make_static against what the
reference itself produced (tests/golden/voicepack_small.*, tools/gen_golden_voicepack.py), style_index, the BS.1770 meter,
and the refusals."""
import json
import math
import os

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

from tests import voicepack_cases as VC

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(G, "voicepack_small.safetensors")), json.load(open(os.path.join(G, "voicepack_small.json")))


def reference_pack(fx, name):
    if f"{name}.pack" in fx:
        return fx[f"{name}.pack"]
    return fx[f"{name}.pack_unique"][fx[f"{name}.pack_index"].long()]


@pytest.mark.parametrize("name", list(VC.HISTOGRAMS))
def test_windows_are_the_reference_windows(gold, name):
    """resolve_windows on the bucket counts alone gives, for every row of the pack, a window with the CONTENT of the
    reference's own (first / last non-empty bucket and rows held, read off the reference's output on one-hot rows), also
    where `lower` went negative and wrapped to the end of the table ("wrap"); the float64 mean over these windows, rounded
    to fp32, is within twice the reference's own distance from the float64 mean (the gate of the device kernels)."""
    from stylish_tts_amd.voicepack import resolve_windows
    fx, meta = gold
    h = meta["histograms"][name]
    rows, lengths = VC.make_rows(name)
    assert torch.equal(lengths, fx[f"{name}.text_lengths"]), "the seeded rows are not the ones the fixture was made from"
    counts = VC.counts_of(lengths)
    lo, hi = resolve_windows(counts, 100)
    assert len(lo) == len(hi) == 512 and all(0 <= a < b <= 512 for a, b in zip(lo, hi))
    contents = [VC.window_content(counts, a, b) for a, b in zip(lo, hi)]
    assert contents == h["windows"]
    wrapped = [i for i, a in enumerate(lo) if a > i]
    assert bool(wrapped) == h["wraps"]
    if name == "wrap":  # the short rows average the LONGEST texts
        assert wrapped[:3] == [0, 1, 2] and all(lo[i] > 100 for i in wrapped)
    mean = VC.float64_means(rows, lengths, contents).float()
    dist = (mean.double() - reference_pack(fx, name).double()).abs().max().item()
    print(f"\n  {name}: float64 mean (rounded once) vs the reference's fp32 mean {dist:.3e}; reference vs float64 {h['ref_to_f64_max']:.3e}")
    assert dist <= 2 * h["ref_to_f64_max"]


def test_windows_raise_where_the_reference_exits(gold):
    from stylish_tts_amd.lib import StyError
    from stylish_tts_amd.voicepack import resolve_windows
    _, meta = gold
    assert meta["exit_cases"]["99_in_one_bucket"] and not meta["exit_cases"]["100_in_one_bucket"]
    for name, exits in meta["exit_cases"].items():
        counts = VC.counts_of(VC.exit_case_lengths(name))
        if exits:
            with pytest.raises(StyError, match="Need at least 100 styles"):
                resolve_windows(counts, 100)
        else:
            lo, hi = resolve_windows(counts, 100)
            assert all(VC.window_content(counts, a, b)[2] >= 100 for a, b in zip(lo, hi)), name
    # the constant is a parameter: one row is enough for min_styles = 1, and the same row is not for 2
    one = VC.counts_of([37])
    lo, hi = resolve_windows(one, 1)
    assert (lo[36], hi[36]) == (36, 37)
    with pytest.raises(StyError):
        resolve_windows(one, 2)


def test_style_index():
    from stylish_tts_amd.voicepack import style_index
    assert [style_index(n) for n in (1, 37, 600)] == [0, 36, 511]
    assert style_index(0) == 0 and style_index(512) == 511
    assert [style_index(n, reference_index=True) for n in (1, 37, 600)] == [511, 511, 511]
    # the bucket make_static files an utterance of that length under
    assert VC.counts_of([37])[style_index(37)] == 1


def _sine(level_db=0.0, seconds=5.0, rate=24000):
    t = np.arange(int(seconds * rate)) / rate
    return 10.0 ** (level_db / 20.0) * np.sin(2 * np.pi * 997.0 * t)


def test_loudness_meter():
    """BS.1770-4: a full-scale 997 Hz sine reads -3.01 LKFS (the figure the standard fixes the K-filter offset by) within the
    ITU compliance tolerance of 0.1 LU, at 24 kHz and at 48 kHz; the meter is linear in level; normalisation lands on its
    target; what is shorter than one block comes back unchanged."""
    from stylish_tts_amd import loudness as LD
    full = LD.integrated_loudness(_sine(), 24000)
    print(f"\n  full-scale 997 Hz sine: {full:.4f} LKFS at 24 kHz, {LD.integrated_loudness(_sine(rate=48000), 48000):.4f} at 48 kHz")
    assert abs(full - (-3.01)) <= 0.1
    assert abs(LD.integrated_loudness(_sine(rate=48000), 48000) - (-3.01)) <= 0.1
    plain = VC.loudness_plain(_sine(seconds=2.0), 24000)  # the plain restatement (block loop, sample-by-sample filters)
    assert abs(LD.integrated_loudness(_sine(seconds=2.0), 24000) - plain) <= 1e-3
    assert abs(LD.integrated_loudness(_sine(-23.0), 24000) - (full - 23.0)) <= 1e-6
    stereo = np.stack([_sine(), _sine()], axis=1)  # two equal channels: + 3.01 dB
    assert abs(LD.integrated_loudness(stereo, 24000) - (full + 10 * math.log10(2.0))) <= 1e-6
    x = _sine(-23.0).astype(np.float32)
    y = LD.normalize(x, -25.0, 24000)
    assert y.dtype == np.float32 and abs(LD.integrated_loudness(y, 24000) - (-25.0)) <= 0.01
    # gating: five seconds of near-silence beside the tone do not pull the figure down
    gated = np.concatenate([_sine(-23.0), 1e-6 * _sine()])
    assert abs(LD.integrated_loudness(gated, 24000) - (full - 23.0)) <= 0.2  # (three blocks straddle the edge; ungated: -3 dB)
    logs = []
    short = _sine(seconds=0.39).astype(np.float32)
    assert LD.normalize(short, -25.0, 24000, log=logs.append) is short and "not normalised" in logs[0]
    silence = np.zeros(24000, np.float32)
    assert LD.normalize(silence, -25.0, 24000, log=logs.append) is silence and len(logs) == 2
    with pytest.raises(ValueError):
        LD.integrated_loudness(short, 24000)


def test_int16_saturates_where_the_reference_wraps():
    from stylish_tts_amd.speak import to_int16
    x = np.array([0.0, 0.5, -0.5, 0.99999, 1.0, 1.5, -1.0, -1.5, 0.25 + 0.9 / 32768], np.float32)
    assert to_int16(x).tolist() == [0, 16384, -16384, 32767, 32767, 32767, -32768, -32768, 8192]
    inside = np.abs(x) < 1.0
    assert np.array_equal(to_int16(x)[inside], np.multiply(x, 32768)[inside].astype(np.int16))  # the reference's own line


def _yamls(tmp_path):
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    cfg, mdl = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg.write_text(_default_config_yaml(tmp_path / "data"))
    mdl.write_text(_default_model_yaml())
    return str(cfg), str(mdl)


def _checkpoint(path, frames):
    from stylish_tts_amd import stage_io as IO
    norm = IO.NormalizationStats()
    norm.frames = frames
    IO.save_checkpoint(str(path), {}, normalization=norm)
    return str(path)


def test_make_voicepack_refusals(tmp_path):
    from stylish_tts_amd import voicepack as V
    from stylish_tts_amd.lib import StyError
    cfg, mdl = _yamls(tmp_path)
    good, empty = _checkpoint(tmp_path / "ckpt", 1000), _checkpoint(tmp_path / "ckpt0", 0)
    out = str(tmp_path / "pack.safetensors")
    with pytest.raises(StyError, match="sentence_transformers"):
        V.voicepack(cfg, True, mdl, out, good, log=lambda m: None)
    with pytest.raises(StyError, match="No normalization state"):
        V.voicepack(cfg, False, mdl, out, empty, log=lambda m: None)
    with pytest.raises(StyError, match="not found"):
        V.voicepack(cfg, False, mdl, out, str(tmp_path / "nowhere"), log=lambda m: None)
    with pytest.raises(StyError, match="model config path is required"):
        V.voicepack(cfg, False, "", out, good, log=lambda m: None)
    if not torch.cuda.is_available():
        with pytest.raises(StyError, match="no HIP device"):
            V.voicepack(cfg, False, mdl, out, good, log=lambda m: None)
        with pytest.raises(StyError, match="HIP device"):
            V.StylePack().add(torch.zeros(2, 192), torch.tensor([3, 4]))
        with pytest.raises(StyError, match="no HIP device"):
            V.calculate_style(torch.zeros(1, 24000), torch.zeros(1, 80), {}, None)
    assert not os.path.exists(out)
    with pytest.raises(SystemExit):
        V.main(["--help"])


def test_speaker_refusals(tmp_path):
    from stylish_tts_amd import speak as SP
    from stylish_tts_amd.lib import StyError
    _, mdl = _yamls(tmp_path)
    ckpt = _checkpoint(tmp_path / "ckpt", 1000)
    static, dynamic, other = (str(tmp_path / f"{n}.safetensors") for n in ("static", "dynamic", "other"))
    save_file({"voicepack_static": torch.zeros(512, 192)}, static)
    save_file({"voicepack_dynamic": torch.zeros(7, 192 + 768)}, dynamic)
    save_file({"something_else": torch.zeros(512, 192)}, other)
    with pytest.raises(StyError, match="sentence_transformers"):
        SP.Speaker(ckpt, mdl, dynamic)
    with pytest.raises(StyError, match="Could not find voicepack key"):
        SP.Speaker(ckpt, mdl, other)
    with pytest.raises(StyError, match="not found"):
        SP.Speaker(ckpt, mdl, str(tmp_path / "missing.safetensors"))
    if not torch.cuda.is_available():
        with pytest.raises(StyError, match="no HIP device"):
            SP.Speaker(ckpt, mdl, static)
    infile = tmp_path / "in.txt"
    infile.write_text("ɑbɑ|first\n\nno separator here\n", encoding="utf-8")
    with pytest.raises(StyError, match="line 3"):
        SP.read_lines(str(infile))
    infile.write_text("ɑbɑ|first\n\nbɑ|second\n", encoding="utf-8")
    assert SP.read_lines(str(infile)) == [(0, "ɑbɑ"), (2, "bɑ")]
    with pytest.raises(SystemExit):
        SP.main(["--help"])
