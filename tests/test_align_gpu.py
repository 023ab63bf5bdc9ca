"""The alignment stage on the device: the TextAligner forward against the reference's recorded outputs and the float64
restatement, the forced-alignment kernel against its fp32 twin (tests/align_cases.viterbi_fp32: integers equal, scores
bit-equal), the `align` command end to end on a synthetic dataset, and the kind's refusals."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

from tests import align_cases as AC

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
FWD_T = (2, 62, 64, 66, 130)


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(G, "align_small.safetensors")), json.load(open(os.path.join(G, "align_small.json")))


_MODELS = {}


def device_model(hidden):
    import stylish_tts_amd as S
    if hidden not in _MODELS:
        m = S.TextAligner(AC.N_MELS, AC.TOKENS, hidden_dim=hidden)
        m.load_state_dict(AC.aligner_weights(hidden, AC.SMALL_SEED + hidden), strict=True)
        _MODELS[hidden] = (m.to(DEV).eval(), AC.aligner_weights(hidden, AC.SMALL_SEED + hidden))
    return _MODELS[hidden]


def ragged_lengths(T):
    return torch.tensor([T, max(1, (T * 5) // 8), 1])  # a full row, a ragged row, a row of one frame


def forward_gate(ref64, ref32):
    """max(1e-5 max|ref|, 4 x the fp32 CPU run's own distance from float64 on this case) and its three numbers"""
    scale = ref64.abs().max().item()
    own = (ref32.double() - ref64).abs().max().item()
    return max(1e-5 * scale, 4 * own), scale, own


def test_forward_vs_reference_fixture(gold):
    """hidden_dim 80, the reference module's own outputs on [3, 66, 80] with lengths [66, 40, 1]; the gate's second term is
    the reference's fp32 run against its float64 run, both in the fixture.  Negative control: one length off by one."""
    import stylish_tts_amd as S
    fx, meta = gold
    m = S.TextAligner(AC.N_MELS, AC.TOKENS, hidden_dim=meta["hidden"])
    m.load_state_dict(AC.aligner_weights(meta["hidden"], meta["seed"]), strict=True)
    m = m.to(DEV).eval()
    ref64, ref32 = fx["fwd.log_probs_f64"], fx["fwd.log_probs_f32"]
    gate, scale, own = forward_gate(ref64, ref32)
    with torch.no_grad():
        got = m(fx["fwd.input"].to(DEV), fx["fwd.lengths"].to(DEV), time_major=True)
        off = m(fx["fwd.input"].to(DEV), (fx["fwd.lengths"] + torch.tensor([0, 1, 0])).to(DEV), time_major=True)
    torch.cuda.synchronize()
    err = (got.cpu().double() - ref64).abs().max().item()
    err_off = (off.cpu().double() - ref64).abs().max().item()
    print(f"\n  align_parity fixture hidden={meta['hidden']} T=66: max|ref| {scale:.4f}  reference fp32-to-f64 {own:.3e}  "
          f"device-to-f64 {err:.3e}  gate {gate:.3e}  (length off by one: {err_off:.3e})")
    assert got.shape == (3, 66, AC.TOKENS + 1) and bool(torch.isfinite(got).all())
    assert err <= gate
    assert err_off > gate, "a wrong length mask must turn the gate red"


@pytest.mark.parametrize("hidden", [80, 640])
@pytest.mark.parametrize("T", FWD_T)
def test_forward_vs_float64_restatement(hidden, T):
    """seeded weights at both widths, B = 3 ragged (full, 5/8, one frame); the gate's second term is measured on the case:
    the fp32 CPU run of the restatement (the reference's arithmetic, tests/test_align.py) against its float64 run"""
    m, P = device_model(hidden)
    g = torch.Generator().manual_seed(1000 * hidden + T)
    mel = torch.randn(3, AC.N_MELS, T, generator=g)
    lengths = ragged_lengths(T)
    ref64 = AC.aligner_forward(P, mel, lengths, torch.float64)
    ref32 = AC.aligner_forward(P, mel, lengths, torch.float32)
    gate, scale, own = forward_gate(ref64, ref32)
    with torch.no_grad():
        got = m(mel.to(DEV), lengths.to(DEV))
    torch.cuda.synchronize()
    err = (got.cpu().double() - ref64).abs().max().item()
    print(f"\n  align_parity hidden={hidden} T={T}: max|ref| {scale:.4f}  cpu fp32-to-f64 {own:.3e}  device-to-f64 {err:.3e}  "
          f"gate {gate:.3e}")
    assert got.shape == (3, T, AC.TOKENS + 1)
    assert err <= gate
    if T >= 62:  # negative control: the ragged row one frame longer
        with torch.no_grad():
            off = m(mel.to(DEV), (lengths + torch.tensor([0, 1, 0])).to(DEV))
        assert (off.cpu().double() - ref64).abs().max().item() > gate


# ---- the dynamic programme -----------------------------------------------------------------------------------------
def run_forced_align(lp, targets, in_len, tg_len, blank=AC.BLANK):
    """-> labels, scores, status on the host (the Python wrapper raises on a refused row and hands the buffers out on the error)"""
    from stylish_tts_amd.align import forced_align
    from stylish_tts_amd.lib import StyError
    try:
        labels, scores = forced_align(lp.to(DEV), targets, in_len, tg_len, blank)
        status = [0] * lp.shape[0]
    except StyError as e:
        if not hasattr(e, "status"):
            raise
        labels, scores, status = e.labels, e.scores, e.status
    torch.cuda.synchronize()
    return labels.cpu(), scores.cpu(), torch.tensor(status, dtype=torch.int32)


def dp_batch(rs, U):
    """four rows around one U: slack, tight (T = U + repeats), infeasible (one frame fewer), a shorter target"""
    rows = []
    t_slack = AC.random_targets(rs, U, repeat_every=5)
    rows.append((t_slack, U + AC.repeats(t_slack) + 7))
    t_tight = AC.random_targets(rs, U, repeat_every=3)
    rows.append((t_tight, U + AC.repeats(t_tight)))
    t_bad = AC.random_targets(rs, U, repeat_every=4)
    rows.append((t_bad, U + AC.repeats(t_bad) - 1))
    t_short = AC.random_targets(rs, U // 2 + 1)
    rows.append((t_short, U // 2 + 1 + AC.repeats(t_short) + 3))
    T = max(n for _, n in rows)
    targets = torch.zeros(len(rows), U, dtype=torch.long)
    for i, (tg, _) in enumerate(rows):
        targets[i, :len(tg)] = torch.tensor(tg)
    lp = torch.stack([AC.random_log_probs(rs, T) for _ in rows])
    return lp, targets, torch.tensor([n for _, n in rows]), torch.tensor([len(tg) for tg, _ in rows])


@pytest.mark.parametrize("U", [1, 2, 31, 32, 33, 63, 64, 65, 255, 510])
def test_forced_align_vs_fp32_restatement(U):
    """S = 2 U + 1 crosses the wave (64) and workgroup (256) edges.  One batch holds a row with slack, a tight row, an
    infeasible row (status 1, labels -1; every index of the kernel stays in range: the row is refused before the first
    frame is read) and a row with a shorter target and input; its neighbours are untouched by the refusal."""
    from stylish_tts_amd.lib import StyError
    rs = np.random.RandomState(U)
    lp, targets, in_len, tg_len = dp_batch(rs, U)
    want_l, want_s, want_st = AC.forced_align_rows(lp, targets, in_len, tg_len, AC.BLANK)
    labels, scores, status = run_forced_align(lp, targets, in_len, tg_len)
    assert want_st.tolist() == [0, 0, 1, 0] and status.tolist() == [0, 0, 1, 0]
    assert labels.dtype == torch.int32 and torch.equal(labels, want_l)
    assert torch.equal(scores, want_s), (scores - want_s).abs().max()
    assert bool((labels[2] == -1).all()) and bool((scores[2] == 0).all())
    for b in (0, 1, 3):
        n, u = int(in_len[b]), int(tg_len[b])
        assert AC.collapse(labels[b, :n], AC.BLANK) == targets[b, :u].tolist()
        assert bool((labels[b, n:] == -1).all()) and bool((scores[b, n:] == 0).all())
    from stylish_tts_amd.align import forced_align
    with pytest.raises(StyError, match=r"row\(s\) \[2\]"):
        forced_align(lp.to(DEV), targets, in_len, tg_len, AC.BLANK)


def test_forced_align_one_repeated_token_and_minus_infinity():
    rs = np.random.RandomState(77)
    U = 33
    tg = [7] * U  # 32 repeats: the tight length is 65, every token needs a blank in between
    lp = torch.stack([AC.random_log_probs(rs, 70), AC.random_log_probs(rs, 70)])
    lp[1, :, 100:140] = -float("inf")  # classes no path needs ...
    lp[1, 5, 7] = -float("inf")        # ... and the target's own token at one frame
    targets = torch.tensor([tg, tg])
    in_len, tg_len = torch.tensor([65, 70]), torch.tensor([U, U])
    want_l, want_s, _ = AC.forced_align_rows(lp, targets, in_len, tg_len, AC.BLANK)
    labels, scores, status = run_forced_align(lp, targets, in_len, tg_len)
    assert status.tolist() == [0, 0]
    assert torch.equal(labels, want_l) and torch.equal(scores, want_s)
    assert not bool(torch.isnan(scores).any())
    assert labels[0, :65].tolist() == [7, AC.BLANK] * 32 + [7]
    # a row whose every path runs through -inf: still a path, no NaN
    lp2 = AC.random_log_probs(rs, 12)[None].clone()
    lp2[0, :, 9] = -float("inf")
    l2, s2, st2 = run_forced_align(lp2, torch.tensor([[4, 9, 4]]), torch.tensor([12]), torch.tensor([3]))
    w2 = AC.forced_align_rows(lp2, torch.tensor([[4, 9, 4]]), torch.tensor([12]), torch.tensor([3]), AC.BLANK)
    assert st2.tolist() == [0] and torch.equal(l2, w2[0]) and torch.equal(s2, w2[1]) and not bool(torch.isnan(s2).any())


def test_forced_align_does_not_depend_on_the_batch():
    rs = np.random.RandomState(5)
    B, T, U = 8, 90, 40
    lp = torch.stack([AC.random_log_probs(rs, T) for _ in range(B)])
    tg_len = torch.tensor([40, 1, 17, 33, 40, 8, 25, 31])
    in_len = torch.tensor([90, 5, 60, 90, 64, 30, 90, 77])
    targets = torch.zeros(B, U, dtype=torch.long)
    for b in range(B):
        targets[b, :int(tg_len[b])] = torch.tensor(AC.random_targets(rs, int(tg_len[b]), repeat_every=6))
    labels, scores, status = run_forced_align(lp, targets, in_len, tg_len)
    assert status.tolist() == [0] * B
    for b in range(B):
        l1, s1, st1 = run_forced_align(lp[b:b + 1], targets[b:b + 1], in_len[b:b + 1], tg_len[b:b + 1])
        assert st1.tolist() == [0] and torch.equal(l1[0], labels[b]) and torch.equal(s1[0], scores[b])


def test_forced_align_refuses_out_of_range_rows():
    """a target equal to the blank / past the classes, a length past the buffers: status 2, labels -1, neighbours aligned"""
    rs = np.random.RandomState(9)
    lp = torch.stack([AC.random_log_probs(rs, 20) for _ in range(4)])
    targets = torch.tensor([[3, 4, 5], [3, AC.BLANK, 5], [3, 4, 999], [3, 4, 5]])
    in_len, tg_len = torch.tensor([20, 20, 20, 21]), torch.tensor([3, 3, 3, 3])
    labels, scores, status = run_forced_align(lp, targets, in_len, tg_len)
    assert status.tolist() == [0, 2, 2, 2]
    assert bool((labels[1:] == -1).all()) and bool((scores[1:] == 0).all())
    want = AC.forced_align_rows(lp[:1], targets[:1], in_len[:1], tg_len[:1], AC.BLANK)
    assert torch.equal(labels[:1], want[0]) and torch.equal(scores[:1], want[1])


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_fixture_utterances_reproduce_the_reference_durations(gold):
    """the reference's calculate_alignment_single on three utterances whose path is stable under noise of the forward
    gate's size (tools/gen_golden_align.py): from the mel it fed its model, the device gives its durations exactly"""
    import stylish_tts_amd as S
    from stylish_tts_amd.align import durations_from_labels, forced_align
    fx, meta = gold
    m = S.TextAligner(AC.N_MELS, AC.TOKENS, hidden_dim=meta["hidden"])
    m.load_state_dict(AC.aligner_weights(meta["hidden"], meta["seed"]), strict=True)
    m = m.to(DEV).eval()
    assert meta["e2e"] == 3
    for i in range(meta["e2e"]):
        mel, text, want = fx[f"e2e.{i}.mel"], fx[f"e2e.{i}.text"], fx[f"e2e.{i}.durations"]
        T = mel.shape[1]
        with torch.no_grad():
            lp = m(mel[None].to(DEV), torch.tensor([T], device=DEV))
        labels, scores = forced_align(lp, text[None], torch.tensor([T]), torch.tensor([text.shape[0]]), AC.BLANK)
        got = durations_from_labels(labels[0].cpu(), text[None], AC.BLANK)
        assert torch.equal(got, want), (i, got, want)
        assert got.sum().item() == T
        assert scores.exp().mean().item() == pytest.approx(fx[f"e2e.{i}.score"].item(), rel=1e-3)


def test_align_command_end_to_end(tmp_path):
    """config.yml + model.yml + alignment_model.safetensors + a synthetic dataset (no alignment and no pitch file) ->
    `python -m stylish_tts_amd.align` -> alignment.safetensors, scores_val.txt, scores_train.txt; SampleDataset loads the
    file; every row equals the restatement chain (float64 forward -> fp32 Viterbi -> durations_from_labels) on the same mel"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_sample_dataset as M
    from stylish_tts_amd import align as A
    from stylish_tts_amd import data as D
    from stylish_tts_amd.frontend import MelSpec, calculate_mel
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    root = tmp_path / "data"
    lines = M.make(str(root), n=10, seed=21, n_val=2)
    os.remove(root / "alignment.safetensors")
    os.remove(root / "pitch.safetensors")
    P = AC.aligner_weights()
    save_file({k: v.contiguous() for k, v in P.items()}, str(root / "alignment_model.safetensors"))
    cfg, mdl = tmp_path / "config.yml", tmp_path / "model.yml"
    cfg.write_text(_default_config_yaml(root))
    mdl.write_text(_default_model_yaml())
    logged = []
    A.align(str(cfg), str(mdl), "torch", 4, log=logged.append)
    assert any("utterances/s" in ln for ln in logged), logged
    print("\n  " + [ln for ln in logged if "utterances/s" in ln][0])
    assert not (root / "temp").exists()
    result = load_file(str(root / "alignment.safetensors"))
    names = [ln.split("|")[0] for ln in lines]
    assert sorted(result) == sorted(names)
    for split, fname, part in (("val", "scores_val.txt", names[8:]), ("train", "scores_train.txt", names[:8])):
        rows = open(root / fname, encoding="utf-8").read().splitlines()
        assert sorted(r.split(" ", 1)[1] for r in rows) == sorted(part), split
        assert all(0.0 < float(r.split(" ", 1)[0]) <= 1.0 for r in rows)
    norm = json.load(open(root / "normalization.json"))
    ds = D.SampleDataset(data_list=lines, root_path=str(root / "wav-dir"), pitch_path=None,
                         alignment_path=str(root / "alignment.safetensors"))
    to_mel = MelSpec(A.ALIGNER_MEL["n_fft"], A.ALIGNER_MEL["win_length"], 300)
    for i, name in enumerate(names):
        _, tokens, path, wave, _, alignment = ds[i]
        dur = result[name]
        frames = wave.shape[0] // 300
        assert dur.dtype == torch.float32 and dur.shape == (1, tokens.shape[0])
        assert dur.sum().item() == frames, (name, dur.sum().item(), frames)
        assert torch.equal(alignment, dur)
        mel, mel_len = calculate_mel(wave[None].to(DEV), to_mel, norm["mel_log_mean"], norm["mel_log_std"])
        assert int(mel_len[0]) == frames
        want = AC.durations_chain(P, mel.cpu(), mel_len.cpu(), tokens[None], torch.tensor([tokens.shape[0]]))[0]
        assert torch.equal(dur, want), (name, dur, want)
    # replaces an existing file, and the command-line form runs the same pass
    A.main([str(cfg), "--model-config", str(mdl), "-bs", "3"])
    again = load_file(str(root / "alignment.safetensors"))
    assert all(torch.equal(again[k], result[k]) for k in result), "the result depends on the batch size"


def test_training_and_bf16_are_refused_for_the_kind():
    import stylish_tts_amd as S
    from stylish_tts_amd import lib as L
    lib = L.load()
    h = C.c_void_p()
    assert lib.sty_model_create(b"text_aligner", C.byref(h)) == 0
    assert lib.sty_model_enable_training(h) == -1 and b"inference-only" in lib.sty_last_error()
    opts = L.TrainOpts(0, 0, 0, 0, 0.1, 0, 0.2, 1, 0, 0.2)
    assert lib.sty_model_set_train_opts(h, C.byref(opts)) == -1 and b"inference-only" in lib.sty_last_error()
    g = torch.zeros(4, device=DEV)
    assert lib.sty_model_bind_grad(h, b"encoder_output_layer.bias", L.ptr(g)) == -1
    lib.sty_model_destroy(h)
    m, _ = device_model(80)
    m.set_train_opts(compute_bf16=False)
    with pytest.raises(S.StyError, match="inference-only"):
        m.set_train_opts(compute_bf16=True)
    m.set_train_opts(compute_bf16=False)
    with torch.no_grad():
        out = m(torch.zeros(1, AC.N_MELS, 4, device=DEV), torch.tensor([4], device=DEV))
    assert out.shape == (1, 4, AC.TOKENS + 1)
