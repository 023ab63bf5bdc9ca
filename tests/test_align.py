"""The alignment stage without a device: the host restatements of tests/align_cases.py against the reference's recorded
outputs (tests/golden/align_small.*, tools/gen_golden_align.py) and against brute force, the literal port of torch_align's
duration loop, the shell's state_dict layout, the command's refusals and file formats."""
import itertools
import json
import os

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

from tests import align_cases as AC

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(G, "align_small.safetensors")), json.load(open(os.path.join(G, "align_small.json")))


def test_forward_restatement_matches_the_reference(gold):
    """the torch.nn.functional restatement of the model against the reference module's own outputs: 1e-6 in fp32, 1e-12 in
    float64 (input [3, 66, 80], lengths [66, 40, 1]: a full row, a ragged row and a row of one frame)"""
    fx, meta = gold
    P = AC.aligner_weights(meta["hidden"], meta["seed"])
    mel = fx["fwd.input"].transpose(1, 2)  # the fixture holds the reference's [B, T, n_mels]
    lengths = fx["fwd.lengths"]
    assert lengths.tolist() == [66, 40, 1]
    e32 = (AC.aligner_forward(P, mel, lengths, torch.float32) - fx["fwd.log_probs_f32"]).abs().max().item()
    e64 = (AC.aligner_forward(P, mel, lengths, torch.float64) - fx["fwd.log_probs_f64"]).abs().max().item()
    print(f"\n  restatement vs reference: fp32 {e32:.3e}, float64 {e64:.3e}")
    assert fx["fwd.log_probs_f64"].dtype == torch.float64
    assert e32 <= 1e-6
    assert e64 <= 1e-12
    dist = (fx["fwd.log_probs_f32"].double() - fx["fwd.log_probs_f64"]).abs().max().item()
    assert dist == pytest.approx(meta["fwd_ref_f32_to_f64"], rel=1e-9)


def _small_targets():
    for U in (1, 2, 3):
        for tg in itertools.product((0, 1, 2), repeat=U):
            yield list(tg)


def test_viterbi_restatement_agrees_with_brute_force():
    """every target over three symbols with U <= 3 (with and without adjacent repeats) at every T from the tightest
    (U + repeats) to 7, random log-probs: the DP's total is the best total over all valid paths (bit-equal: both sum in
    frame order in fp32), its path is one of the best paths, and the path collapses to the target"""
    rs = np.random.RandomState(0)
    blank, cases = 3, 0
    for tg in _small_targets():
        for T in range(len(tg) + AC.repeats(tg), 8):
            lp = AC.random_log_probs(rs, T, V1=4, spread=2.0).numpy()
            labels, scores, total = AC.viterbi_fp32(lp, tg, blank)
            best, arg = AC.brute_force(lp, tg, blank)
            assert total == best, (tg, T)
            assert labels.tolist() in arg, (tg, T)
            assert AC.collapse(labels, blank) == tg
            assert np.array_equal(scores, lp[np.arange(T), labels])
            cases += 1
    assert cases > 150
    with pytest.raises(ValueError):
        AC.viterbi_fp32(AC.random_log_probs(rs, 2, V1=4).numpy(), [1, 1], blank)  # needs 3 frames


def test_viterbi_restatement_handles_minus_infinity():
    rs = np.random.RandomState(1)
    lp = AC.random_log_probs(rs, 9, V1=5).numpy()
    lp[:, 4] = -np.inf  # a class the target never uses
    lp[3, 1] = -np.inf  # and one it does, at one frame
    labels, scores, total = AC.viterbi_fp32(lp, [1, 2, 1], 0)
    assert AC.collapse(labels, 0) == [1, 2, 1] and np.isfinite(total) and not np.isnan(scores).any()


def test_durations_from_labels_is_the_reference_loop(gold, capsys):
    """the literal port of align_text.py:324-354 on the hand-made paths: a leading blank, a repeated token separated by a
    blank, a path longer than the text (first warning + break), a label that is not the current token (second warning)"""
    from stylish_tts_amd.align import durations_from_labels
    fx, meta = gold
    assert {"leading_blank", "repeat_with_blank", "longer_than_sequence", "mismatch"} <= set(AC.LABEL_PATHS)
    for name, (text, path) in AC.LABEL_PATHS.items():
        got = durations_from_labels(torch.tensor(path, dtype=torch.int32), torch.tensor([text]), AC.BLANK)
        printed = capsys.readouterr().out
        want = fx[f"paths.{name}.durations"]
        assert got.dtype == torch.float32 and got.shape == (1, len(text))
        assert torch.equal(got, want), (name, got, want)
        assert printed.count("longer than the sequence") == meta["label_paths"][name]["longer"], name
        assert printed.count("doesn't match the sequence") == meta["label_paths"][name]["mismatch"], name
    assert meta["label_paths"]["longer_than_sequence"]["longer"] == 1 and meta["label_paths"]["mismatch"]["mismatch"] >= 1


def test_shell_has_the_reference_state_dict_layout(gold):
    import stylish_tts_amd as S
    ref = json.load(open(os.path.join(G, "manifest_text_aligner.json")))
    m = S.TextAligner(80, 178)
    sd = m.state_dict()
    assert len(ref) == 27 and {k: list(v.shape) for k, v in sd.items()} == ref
    assert m.KIND == "text_aligner" and not sd["encoder.layers.0.2.num_batches_tracked"].is_floating_point()
    # the seeded small model loads strictly into a shell of its width
    small = S.TextAligner(80, 178, hidden_dim=AC.SMALL_HIDDEN)
    small.load_state_dict(AC.aligner_weights(), strict=True)
    with pytest.raises(S.StyError, match="inference only"):
        small.enable_training()
    with pytest.raises(S.StyError):
        small(torch.zeros(1, 80, 4), torch.tensor([4]))  # no autograd-free context / no device: refused, never a fallback


def test_k2_method_and_missing_inputs_are_refused(tmp_path):
    from stylish_tts_amd import align as A
    from stylish_tts_amd.config import load_config_yaml, load_model_config_yaml
    from stylish_tts_amd.lib import StyError
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    cfg, mdl = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg.write_text(_default_config_yaml(tmp_path / "nowhere"))
    mdl.write_text(_default_model_yaml())
    with pytest.raises(StyError, match="k2"):
        A.align(str(cfg), str(mdl), "k2", 8)
    with pytest.raises(StyError, match="k2"):
        A.main([str(cfg), "--model-config", str(mdl), "--method", "k2"])
    with pytest.raises(NotImplementedError):
        A.align_text(load_config_yaml(str(cfg)), load_model_config_yaml(_default_model_yaml()), "teytaut", 8)
    with pytest.raises(StyError, match="not found"):
        A.align(str(cfg), str(mdl), "torch", 8)
    with pytest.raises(SystemExit):
        A.main(["--help"])
    with pytest.raises(StyError, match="HIP device"):
        A.forced_align(torch.zeros(1, 4, 5), torch.zeros(1, 2, dtype=torch.long), torch.tensor([4]), torch.tensor([2]), 4)


def test_kind_refuses_training_and_bf16_without_a_device():
    import ctypes as C
    import stylish_tts_amd as S
    from stylish_tts_amd import lib as L
    lib = L.load()
    h = C.c_void_p()
    assert lib.sty_model_create(b"text_aligner", C.byref(h)) == 0
    assert lib.sty_model_enable_training(h) == -1 and b"inference-only" in lib.sty_last_error()
    opts = L.TrainOpts(0, 0, 0, 0, 0.1, 0, 0.2, 1, 0, 0.2)
    assert lib.sty_model_set_train_opts(h, C.byref(opts)) == -1
    need = C.c_size_t()
    assert lib.sty_aligner_workspace_bytes(h, 2, 80, C.byref(need)) == -5  # not finalized: STY_ESTATE
    lib.sty_model_destroy(h)
    assert lib.sty_forced_align_workspace_bytes(8, 520, 100, C.byref(need)) == 0 and need.value >= 8 * 520 * 4 * 16
    assert lib.sty_forced_align_workspace_bytes(1, 10, 513, C.byref(need)) == -1  # U <= 512
    with pytest.raises(S.StyError, match="inference-only"):
        S.TextAligner(80, 178, hidden_dim=80).set_train_opts(compute_bf16=True)


def test_scores_line_format():
    """align_text.py:171-189: `str(score) + " " + name + "\\n"`, the score a Python float"""
    from stylish_tts_amd.align import score_line
    s = torch.tensor([-0.5, -1.0, 0.0]).exp().mean().item()
    line = score_line(s, "12.wav")
    assert line == str(s) + " 12.wav\n" and line.endswith("\n")
    assert float(line.split(" ", 1)[0]) == s and line.split(" ", 1)[1] == "12.wav\n"


def test_sample_dataset_without_a_pitch_file(tmp_path):
    """pitch_path=None: the dataset opens no pitch file, items carry pitch None and the alignment collater takes them; with a
    path the behaviour is what it was"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_sample_dataset as M
    from stylish_tts_amd import data as D
    lines = M.make(str(tmp_path), n=4, seed=3, n_val=1)
    os.remove(tmp_path / "pitch.safetensors")
    ds = D.SampleDataset(data_list=lines, root_path=str(tmp_path / "wav-dir"), pitch_path=None, alignment_path="")
    item = ds[0]
    assert item[4] is None and item[5].shape == (3, item[1].shape[0])
    bins, _ = ds.time_bins()
    idx = next(iter(bins.values()))
    waves, texts, text_lengths, paths, pitches, _ = D.Collater(stage="alignment", hop_length=300)([ds[i] for i in idx])
    assert waves.shape[0] == len(idx) and not pitches.any() and paths[0].endswith(".wav")
    with pytest.raises(ValueError, match="Pitch not found"):
        D.Collater(stage="acoustic", hop_length=300)([ds[0]])
    with pytest.raises(Exception):
        D.SampleDataset(data_list=lines, root_path=str(tmp_path / "wav-dir"), pitch_path=str(tmp_path / "pitch.safetensors"),
                        alignment_path="")
    save_file({lines[0].split("|")[0]: torch.ones(1, 7)}, str(tmp_path / "pitch.safetensors"))
    ds2 = D.SampleDataset(data_list=lines, root_path=str(tmp_path / "wav-dir"), pitch_path=str(tmp_path / "pitch.safetensors"),
                          alignment_path="")
    assert torch.equal(ds2[0][4], torch.ones(1, 7))
