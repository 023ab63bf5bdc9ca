"""`voicepack` / `speak` on the device: the pack kernels against the reference's make_static, calculate_style against the
oracle and the reference's rows (tests/golden/voicepack_small.*, tools/gen_golden_voicepack.py), and the two commands end
to end on a synthetic dataset."""
import json
import os
import sys
import types
import wave

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from tests import voicepack_cases as VC

G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
SE_TOL, PSE_TOL = 1e-5, 2e-5  # test_hip_parity: test_mel_style_encoder, test_pitch_style_encoder_vs_reference_golden
FRONT_END_TOL = 1e-4          # test_hip_parity.test_mel_front_end: mel and log energy, relative to the tensor's scale


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(G, "voicepack_small.safetensors")), json.load(open(os.path.join(G, "voicepack_small.json")))


def reference_pack(fx, name):
    if f"{name}.pack" in fx:
        return fx[f"{name}.pack"]
    return fx[f"{name}.pack_unique"][fx[f"{name}.pack_index"].long()]


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def splits(n, sizes):
    out, i = [], 0
    while n > 0:
        out.append(min(n, sizes[i % len(sizes)]))
        n -= out[-1]
        i += 1
    return out


@pytest.mark.parametrize("name", list(VC.HISTOGRAMS))
def test_recorded_reference_distance_is_the_fixtures(gold, name):
    """(no GPU) the json's `ref_to_f64_max` is the distance of the stored reference pack from the float64 mean over the stored
    windows: the figure the device gate below is built on"""
    fx, meta = gold
    h = meta["histograms"][name]
    rows, lengths = VC.make_rows(name)
    assert torch.equal(lengths, fx[f"{name}.text_lengths"])
    dist = (reference_pack(fx, name).double() - VC.float64_means(rows, lengths, h["windows"])).abs().max().item()
    assert dist == pytest.approx(h["ref_to_f64_max"], rel=1e-9) and 0 < dist < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VC.HISTOGRAMS))
def test_pack_kernels_vs_reference_make_static(gold, name):
    """sty_pack_accumulate / sty_pack_finalize fed the fixture's rows in batches of uneven size: at most 1 fp32 ulp from the
    float64 mean over the reference's windows (float64 sums, one rounding); at most twice the reference's own (fp32
    averaging) distance from that mean away from the reference's rows; the same bits on a second run; within 1 ulp under
    a different batch split."""
    from stylish_tts_amd.voicepack import StylePack
    fx, meta = gold
    h = meta["histograms"][name]
    rows, lengths = VC.make_rows(name)
    counts = VC.counts_of(lengths)
    mean64 = VC.float64_means(rows, lengths, h["windows"])

    def run(sizes):
        sp, pos = StylePack(512, 192, 100), 0
        for n in splits(len(lengths), sizes):
            sp.add(rows[pos:pos + n].to(DEV), lengths[pos:pos + n])
            pos += n
        pack = sp.finalize()
        torch.cuda.synchronize()
        assert sp.counts.cpu().tolist() == counts
        assert [VC.window_content(counts, a, b) for a, b in zip(*sp.windows)] == h["windows"]
        return pack.cpu()

    a = run((1, 7, 32, 3, 64, 13))
    assert a.shape == (512, 192) and a.dtype == torch.float32 and bool(torch.isfinite(a).all())
    ulps = ((a.double() - mean64).abs() / VC.ulp32(mean64)).max().item()
    to_ref = (a.double() - reference_pack(fx, name).double()).abs().max().item()
    print(f"\n  {name}: {ulps:.3f} ulp from the float64 mean; {to_ref:.3e} from the reference (its own distance {h['ref_to_f64_max']:.3e})")
    assert ulps <= 1.0
    assert to_ref <= 2 * h["ref_to_f64_max"]
    assert torch.equal(a, run((1, 7, 32, 3, 64, 13))), "two runs over the same batches differ"
    b = run((50, 2, 17))
    assert ((a.double() - b.double()).abs() / VC.ulp32(mean64)).max().item() <= 1.0


@pytest.mark.gpu
def test_pack_refuses_bad_lengths_on_the_host():
    from stylish_tts_amd.lib import StyError
    from stylish_tts_amd.voicepack import StylePack
    sp = StylePack(512, 192, 1)
    x = torch.zeros(2, 192, device=DEV)
    for bad in ([0, 5], [5, 513]):
        with pytest.raises(StyError, match="outside 1..512"):
            sp.add(x, torch.tensor(bad))
    with pytest.raises(StyError, match="CPU tensor"):
        sp.add(x, torch.tensor([5, 6], device=DEV))
    with pytest.raises(StyError, match="none were added"):
        sp.finalize()
    sp.add(x + 1.5, torch.tensor([5, 512]))
    pack = sp.finalize()
    torch.cuda.synchronize()
    assert torch.equal(pack.cpu(), torch.full((512, 192), 1.5))


def _style_models(seeds):
    import stylish_tts_amd as S
    from oracle.manifest import pitch_style_encoder_manifest, style_encoder_manifest
    from oracle.weights import fill_state_dict
    P = {"speech_style_encoder": fill_state_dict(style_encoder_manifest(), seeds["speech_style_encoder"]),
         "pe_style_encoder": fill_state_dict(pitch_style_encoder_manifest(), seeds["pe_style_encoder"]),
         "duration_style_encoder": fill_state_dict(style_encoder_manifest(), seeds["duration_style_encoder"])}
    models = {}
    for k, p in P.items():
        m = S.PitchStyleEncoder() if k == "pe_style_encoder" else S.MelStyleEncoder()
        m.load_state_dict(p)
        models[k] = m.to(DEV).eval()
    return models, P


def _oracle_rows(P, style_mel, pitch, energy):
    from oracle import predictors as OP
    from oracle import style_encoder as ose
    with torch.no_grad():
        return torch.cat([ose.mel_style_encoder(P["speech_style_encoder"], "", style_mel[:, None]),
                          OP.pitch_style_encoder(P["pe_style_encoder"], style_mel, pitch, energy),
                          ose.mel_style_encoder(P["duration_style_encoder"], "", style_mel[:, None])], dim=1)


@pytest.mark.gpu
def test_calculate_style_vs_oracle_and_reference_rows(gold):
    """calculate_style on the fixture's four padded utterances (two length bins, batches of two):
    - each 64-wide part against the oracle encoder fed the HIP front end's OWN style mel and log energy, at the tolerance the
      inference tests of the same modules hold (1e-5 MelStyleEncoder, 2e-5 PitchStyleEncoder, of the part's scale);
    - a row computed alone (B = 1) against the same row of its bin's batch: the same tolerances (the tile / split-K choice
      depends on B, so not bit equality);
    - against the reference's calculate_style rows (its mels = the oracle front end).  The gate is the front end's own gate
      (1e-4 of the scale of mel / energy, test_mel_front_end) PROPAGATED through the encoders: the largest change of a part,
      relative to its scale, that the oracle encoders show when mel and energy move by 1e-4 of their scale with random
      signs (four sign patterns, seeded), plus the encoder tolerance above.  Measured on this fixture (MI355X): the sign patterns move a part by
      1.2e-7 .. 3.0e-7 of its scale (these encoders damp a mel perturbation by ~400x), so the gate is 1.02e-5 (speech,
      duration) / 2.03e-5 (pe); the HIP rows are 1.4e-7 .. 3.0e-7 from the reference's rows, 1.6e-7 .. 3.9e-7 from the oracle
      on the HIP mels, and a row computed alone is 0.7e-7 .. 1.9e-7 from the same row of its batch.  (A wrong input is far
      outside the gate: the default normalization instead of the checkpoint's moves the parts by 4e-4 .. 4e-3, zero pitch
      the pe part by 4e-2.)"""
    from oracle import frontend as ofe
    from stylish_tts_amd.frontend import MelSpec, calculate_mel
    from stylish_tts_amd.voicepack import calculate_style
    fx, meta = gold
    mean, std = meta["norm"]
    norm = types.SimpleNamespace(mel_log_mean=mean, mel_log_std=std)
    models, P = _style_models(meta["seeds"])
    tols = (SE_TOL, PSE_TOL, SE_TOL)
    names = ("speech", "pe", "duration")
    bad = []
    for b in range(2):
        waves, pitch, ref = fx[f"bin{b}.waves_pcm16"].float() / 32768.0, fx[f"bin{b}.pitch"], fx[f"bin{b}.styles"]
        got = calculate_style(waves.to(DEV), pitch.to(DEV), models, norm)
        _, _, energy = calculate_mel(waves.to(DEV), MelSpec(512, 512, 300), mean, std, want_energy=True)
        style_mel, _ = calculate_mel(waves.to(DEV), MelSpec(2048, 1200, 300), mean, std)
        alone = torch.cat([calculate_style(waves[i:i + 1].to(DEV), pitch[i:i + 1].to(DEV), models, norm) for i in range(2)])
        torch.cuda.synchronize()
        assert got.shape == (2, 192) and bool(torch.isfinite(got).all())
        style_mel, energy = style_mel.cpu(), energy.cpu()
        want = _oracle_rows(P, style_mel, pitch, energy)
        # the front-end gate, propagated: oracle front end -> oracle encoders, inputs moved by the gate with random signs
        o_mel = ofe.calculate_mel(waves, 2048, 1200, 300, mean, std)
        o_energy = ofe.log_energy(ofe.calculate_mel(waves, 512, 512, 300, mean, std), mean, std)
        base = _oracle_rows(P, o_mel, pitch, o_energy)
        g = torch.Generator().manual_seed(100 + b)
        moved = []
        for _ in range(4):
            sm = torch.randint(0, 2, o_mel.shape, generator=g).float() * 2 - 1
            se = torch.randint(0, 2, o_energy.shape, generator=g).float() * 2 - 1
            moved.append(_oracle_rows(P, o_mel + FRONT_END_TOL * o_mel.abs().max() * sm, pitch,
                                      o_energy + FRONT_END_TOL * o_energy.abs().max() * se))
        print(f"\n  bin {b}: oracle rows vs the reference's rows {rel_err(base, ref):.3e}")
        for j, (nm, tol) in enumerate(zip(names, tols)):
            s = slice(64 * j, 64 * j + 64)
            e_oracle, e_alone = rel_err(got[:, s], want[:, s]), rel_err(alone[:, s], got[:, s])
            gate = max(rel_err(m[:, s], base[:, s]) for m in moved) + tol
            e_ref = rel_err(got[:, s], ref[:, s])
            print(f"  bin {b} {nm:9s} vs oracle on the HIP mels {e_oracle:.3e} (tol {tol:.0e})  B=1 vs batch {e_alone:.3e}  "
                  f"vs reference rows {e_ref:.3e} (propagated front-end gate {gate:.3e})")
            if e_oracle > tol:
                bad.append(f"bin {b} {nm} vs oracle")
            if e_alone > tol:
                bad.append(f"bin {b} {nm} B=1 vs batch")
            if e_ref > gate:
                bad.append(f"bin {b} {nm} vs reference rows")
    assert not bad, bad


def _shells(mc, keys):
    """fresh shells of the chain's models under their build_model keys"""
    import stylish_tts_amd as S
    make = {"speech_style_encoder": S.MelStyleEncoder, "pe_style_encoder": S.PitchStyleEncoder,
            "duration_style_encoder": S.MelStyleEncoder,
            "duration_predictor": lambda: S.DurationPredictor(style_dim=mc.style_dim, inter_dim=mc.inter_dim,
                                                              text_config=mc.text_encoder, duration_config=mc.duration_predictor),
            "pitch_energy_predictor": lambda: S.PitchEnergyPredictor(
                style_dim=mc.style_dim, inter_dim=mc.pitch_energy_predictor.inter_dim, text_config=mc.text_encoder,
                duration_config=mc.duration_predictor, pitch_energy_config=mc.pitch_energy_predictor),
            "speech_predictor": lambda: S.SpeechPredictor(mc)}
    return {k: make[k]() for k in keys}


def _write_checkpoint(path, frames=12345):
    """the six models of the chain under the key-named fill + a normalization state, through save_checkpoint"""
    from oracle import manifest as OM
    from oracle.weights import fill_state_dict
    from stylish_tts_amd import stage_io as IO
    from stylish_tts_amd.config import load_model_config_yaml
    from tests.test_boundary import _default_model_yaml
    mc = load_model_config_yaml(_default_model_yaml())
    fill = {"speech_style_encoder": (OM.style_encoder_manifest, 0), "pe_style_encoder": (OM.pitch_style_encoder_manifest, 5),
            "duration_style_encoder": (OM.style_encoder_manifest, 7), "duration_predictor": (OM.duration_predictor_manifest, 3),
            "pitch_energy_predictor": (OM.pitch_energy_predictor_manifest, 4), "speech_predictor": (OM.speech_predictor_manifest, 0)}
    built = _shells(mc, fill)
    for k, (manifest, seed) in fill.items():
        missing, unexpected = built[k].load_state_dict(fill_state_dict(manifest(), seed), strict=False)
        assert not unexpected and all(".stft." in n for n in missing), (k, missing, unexpected)
    norm = IO.NormalizationStats()
    norm.mel_log_mean, norm.mel_log_std, norm.frames = -3.6, 3.9, frames
    IO.save_checkpoint(path, built, normalization=norm)
    return mc, norm


@pytest.mark.gpu
def test_voicepack_and_speak_end_to_end(tmp_path):
    """config.yml + model.yml + a checkpoint directory -> `voicepack` -> the file -> `speak_document` -> a wav.
    The pack is [512, 192], finite, and bit for bit the StylePack over calculate_style of the same batches; a row whose window
    holds exactly one bucket is that bucket's float64 mean (summed in row order, rounded once).  Every segment of the wav is
    the ExportModel output for the pack's row at style_index(token count) and seed = line index, brought to -25 LUFS and
    saturated to int16 (+-1 LSB), and measures -25 LUFS +- 0.05 where it is longer than one block."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import stylish_tts_amd as S
    from make_sample_dataset import make
    from stylish_tts_amd import data as D
    from stylish_tts_amd import loudness as LD
    from stylish_tts_amd import speak as SP
    from stylish_tts_amd import stage_io as IO
    from stylish_tts_amd import voicepack as V
    from stylish_tts_amd.lib import StyError
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    root = tmp_path / "data"
    make(str(root), 26, 5)
    cfg, mdl = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg.write_text(_default_config_yaml(root))
    mdl.write_text(_default_model_yaml())
    ckpt = str(tmp_path / "ckpt")
    mc, norm = _write_checkpoint(ckpt)
    out = str(tmp_path / "voice.safetensors")
    logs = []
    MIN, BATCH = 3, 4
    with pytest.raises(StyError, match="Need at least 100 styles"):  # 24 utterances are not enough for the reference's constant
        V.voicepack(str(cfg), False, str(mdl), out, ckpt, batch_size=BATCH, log=logs.append)
    assert not os.path.exists(out)
    V.voicepack(str(cfg), False, str(mdl), out, ckpt, batch_size=BATCH, min_styles=MIN, log=logs.append)
    assert any("utterances/s at batch size 4" in ln for ln in logs), logs
    file = load_file(out)
    assert list(file) == ["voicepack_static"]
    pack = file["voicepack_static"]
    assert pack.shape == (512, 192) and pack.dtype == torch.float32 and bool(torch.isfinite(pack).all())
    # the same batches through calculate_style + StylePack
    lines = [ln for ln in open(root / "training-list.txt", encoding="utf-8").read().splitlines() if ln.strip()]
    ds = D.SampleDataset(data_list=lines, root_path=str(root / "wav-dir"), pitch_path=str(root / "pitch.safetensors"),
                         alignment_path=str(root / "alignment.safetensors"))
    bins, _ = ds.time_bins()
    loader = torch.utils.data.DataLoader(ds, batch_sampler=D.LengthBinSampler(bins, lambda k: BATCH, shuffle=False),
                                         collate_fn=D.Collater(stage="voicepack", hop_length=300))
    models = _shells(mc, V.STYLE_KEYS)
    IO.load_checkpoint(ckpt, models)
    models = {k: m.to(DEV).eval() for k, m in models.items()}
    sp, rows, lengths = V.StylePack(512, 192, MIN), [], []
    for waves, _, text_lengths, _, pitches, _ in loader:
        styles = V.calculate_style(waves.to(DEV), pitches.to(DEV), models, norm)
        sp.add(styles, text_lengths)
        rows.append(styles.cpu())
        lengths.append(text_lengths)
    again = sp.finalize().cpu()
    torch.cuda.synchronize()
    assert torch.equal(pack, again), "the command's pack is not the StylePack over calculate_style of the same batches"
    rows, lengths = torch.cat(rows), torch.cat(lengths)
    assert len(lengths) == len(lines) == 24
    counts = VC.counts_of(lengths)
    single = [i for i, (a, b) in enumerate(zip(*sp.windows)) if b - a == 1]
    assert single and all(counts[i] >= MIN for i in single)
    for i in single:
        acc = torch.zeros(192, dtype=torch.float64)
        for r in rows[lengths == i + 1]:
            acc += r.double()
        assert torch.equal(pack[i], (acc / counts[i]).float()), i
    # ---- speak -------------------------------------------------------------------------------------------------------
    infile, wav = tmp_path / "in.txt", str(tmp_path / "out.wav")
    phonemes = ["ɑbɐ ɒdæ ɓfʙ, ɑβɔ ɕçɗ ɖðʤ əɘɚ ɛɜɝ.", "ɑɐɒ æɓʙ βɔɕ?"]
    infile.write_text(f"{phonemes[0]}|first line\n{phonemes[1]}|second line\n", encoding="utf-8")
    speaker = SP.Speaker(ckpt, str(mdl), out)
    segments = SP.speak_document(str(infile), wav, speaker, log=logs.append)
    with wave.open(wav, "rb") as f:
        assert (f.getframerate(), f.getnchannels(), f.getsampwidth()) == (24000, 1, 2)
        written = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    assert len(segments) == 2 and np.array_equal(written, np.concatenate(segments))
    chain = _shells(mc, SP.SPEAK_KEYS)
    IO.load_checkpoint(ckpt, chain)
    export = S.ExportModel(**{k: m.to(DEV) for k, m in chain.items()})
    cleaner, pos = D.TextCleaner(), 0
    for i, ph in enumerate(phonemes):
        tokens = cleaner(ph)
        row = pack[V.style_index(len(tokens))].to(DEV)[None]
        assert V.style_index(len(tokens)) == len(tokens) - 1
        audio = export(torch.tensor([tokens], device=DEV), torch.tensor([len(tokens)], device=DEV), row[:, :64], row[:, 64:128],
                       row[:, 128:], seed=i)
        torch.cuda.synchronize()
        audio = audio.reshape(-1).cpu().numpy()
        assert audio.shape[0] % 300 == 0 and audio.shape[0] > 0
        seg = written[pos:pos + audio.shape[0]].astype(np.int64)
        pos += audio.shape[0]
        measurable = audio.shape[0] >= LD.block_samples(24000) and np.isfinite(LD.integrated_loudness(audio, 24000))
        if measurable:
            gain = 10.0 ** ((-25.0 - LD.integrated_loudness(audio, 24000)) / 20.0)
            want = np.clip(audio.astype(np.float64) * gain * 32768.0, -32768, 32767)
            got_lufs = LD.integrated_loudness(seg / 32768.0, 24000)
            print(f"\n  line {i}: {len(tokens)} tokens, {audio.shape[0] / 24000:.2f} s, written segment measures {got_lufs:.3f} LUFS")
            assert abs(got_lufs - (-25.0)) <= 0.05
        else:
            want = np.clip(audio.astype(np.float64) * 32768.0, -32768, 32767)
        assert np.abs(seg - np.trunc(want)).max() <= 1, i
    assert pos == len(written)
    # --reference-index: row 511 for every line
    s511 = speaker.styles(5, reference_index=True)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(s511, (pack[511:, :64], pack[511:, 64:128], pack[511:, 128:])))
