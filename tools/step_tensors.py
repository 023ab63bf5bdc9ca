"""One training step of one model, tensor by tensor: for refactors that must not move a value.

  python tools/step_tensors.py run MODEL [--bf16] --out FILE.npz
      one forward_train + backward of MODEL on cuda:0 (seeded weights, seeded inputs, default train options, a fresh
      model) -> every output, every returned input gradient and every parameter gradient as one .npz
  python tools/step_tensors.py cmp BASE1.npz [BASE2.npz ...] --change CHANGE.npz
      the tensors that are bit-identical across all BASE files must be bit-identical in CHANGE (exit status 1 otherwise);
      for the others (float-atomic sums) the spread of the BASE files and the distance of CHANGE are printed
  python tools/step_tensors.py sizes [--out FILE.txt]
      every sty_*_train_workspace_bytes entry at the shapes of `run` and at the c3 benchmark shape, fp32 and bf16, one line each

MODEL: duration (B 2, L 7), pitch_energy and speech (the sp_small case: B 2, L 40, T 80), style (2 x 1 x 80 x 62),
aligner (hidden 80, T 9: the smallest case of tests/test_align_train_gpu.py).  Reads nothing outside the repository.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEV = "cuda:0"


def dev(t):
    return t.to(DEV)


def _duration(bf16):
    import stylish_tts_amd as S
    from oracle.manifest import duration_predictor_manifest
    from oracle.weights import fill_state_dict
    m = S.DurationPredictor()
    m.load_state_dict(fill_state_dict(duration_predictor_manifest(), 0))
    g = torch.Generator().manual_seed(11)
    texts = torch.randint(1, m.cfg["tokens"], (2, 7), generator=g)
    lengths = torch.tensor([7, 4])
    style = torch.randn(2, m.cfg["style_dim"], generator=g)
    cot = torch.randn(2, 7, m.cfg["dp_classes"], generator=g)
    m = m.to(DEV).enable_training().set_train_opts(compute_bf16=bf16)
    out = m.forward_train(dev(texts), dev(lengths), dev(style))
    return m, {"out": out, "ret.d_style": m.backward(dev(cot))}


def _sp_small():
    from oracle import frontend
    from tests.cases import make_case
    cs = make_case("sp_small")
    return cs, frontend.duration_to_alignment(cs["durations"])


def _pitch_energy(bf16):
    import stylish_tts_amd as S
    from oracle.manifest import pitch_energy_predictor_manifest
    from oracle.weights import fill_state_dict
    cs, ali = _sp_small()
    m = S.PitchEnergyPredictor()
    m.load_state_dict(fill_state_dict(pitch_energy_predictor_manifest(), 4))
    g = torch.Generator().manual_seed(4)
    m = m.to(DEV).enable_training().set_train_opts(compute_bf16=bf16)
    f0, en = m.forward_train(dev(cs["texts"]), dev(cs["text_lengths"]), dev(ali), dev(cs["style"]))
    s1, s2 = torch.randn(f0.shape, generator=g), torch.randn(en.shape, generator=g)
    return m, {"pitch": f0, "energy": en, "ret.d_style": m.backward(dev(s1), dev(s2))}


def _style(bf16):
    import stylish_tts_amd as S
    from oracle.manifest import style_encoder_manifest
    from oracle.weights import fill_state_dict
    m = S.MelStyleEncoder()
    m.load_state_dict(fill_state_dict(style_encoder_manifest(), 0), strict=False)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 1, 80, 62, generator=g) * 0.8 - 0.3
    cot = torch.randn(2, 64, generator=g)
    m = m.to(DEV).enable_training().set_train_opts(compute_bf16=bf16)
    out = m.forward_train(dev(x))
    m.backward(dev(cot))
    return m, {"out": out}


def _speech(bf16):
    import stylish_tts_amd as S
    from oracle.manifest import speech_predictor_manifest
    from oracle.weights import fill_state_dict
    cs, ali = _sp_small()
    voiced = (cs["pitch"] > 20).float()
    m = S.SpeechPredictor()
    m.load_state_dict(fill_state_dict(speech_predictor_manifest(), 0), strict=False)
    m = m.to(DEV).enable_training().set_train_opts(compute_bf16=bf16)
    audio = m.forward_train(dev(cs["texts"]), dev(cs["text_lengths"]), dev(ali), dev(cs["pitch"]), dev(cs["energy"]),
                            dev(voiced), dev(cs["style"]), dev(cs["pitch"]), noise=dev(cs["noise"]), seed=7)
    g = torch.Generator().manual_seed(13)
    cot = torch.randn(audio.shape, generator=g) / audio.numel()
    d_style, d_energy, d_pitch = m.backward(dev(cot), want_pitch=True)
    return m, {"audio": audio, "ret.d_style": d_style, "ret.d_energy": d_energy, "ret.d_pitch": d_pitch}


def _aligner(bf16):
    from stylish_tts_amd.alignment import TrainableTextAligner, ctc_loss
    from tests import align_cases as AC
    from tests import align_train_cases as TC
    if bf16:
        raise SystemExit("the text aligner refuses compute_bf16")
    mel, lengths, targets, tl, P = TC.graph_case(80, 9)
    m = TrainableTextAligner(AC.N_MELS, AC.TOKENS, hidden_dim=80)
    m.load_state_dict(P, strict=True)
    m = m.to(DEV).enable_training()
    lp = m.forward_train(dev(mel), dev(lengths), 0.1, 5)
    loss, _, d = ctc_loss(lp, targets, lengths, tl, TC.BLANK)
    m.backward(d)
    outs = {"log_probs": lp, "loss": loss, "ret.d_log_probs": d}
    outs.update({"buf." + k: v for k, v in m.state_dict().items() if "running_" in k})
    return m, outs


MODELS = {"duration": _duration, "pitch_energy": _pitch_energy, "style": _style, "speech": _speech, "aligner": _aligner}


def run(model, bf16, out):
    m, outs = MODELS[model](bool(bf16))
    torch.cuda.synchronize()
    rec = {k: v.detach().float().cpu().numpy() for k, v in outs.items() if v is not None}
    for k, p in m.named_parameters():
        if p.grad is not None:
            rec["grad." + k] = p.grad.detach().float().cpu().numpy()
    bad = [k for k, v in rec.items() if not np.isfinite(v).all()]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **rec)
    print(f"step_tensors: {model} {'bf16' if bf16 else 'fp32'}: {len(rec)} tensors -> {out}"
          + (f"; NOT FINITE: {bad[:6]}" if bad else ""))
    return 1 if bad else 0


def cmp(base, change):
    bs = [np.load(b) for b in base]
    ch = np.load(change)
    names = sorted(bs[0].files)
    missing = [k for k in names if any(k not in b.files for b in bs[1:]) or k not in ch.files]
    extra = [k for k in ch.files if k not in names]
    stable, moved, noisy = 0, [], []
    for k in names:
        if k in missing:
            continue
        a = bs[0][k]
        if all(b[k].shape == a.shape and np.array_equal(b[k], a, equal_nan=True) for b in bs[1:]):
            stable += 1
            if not (ch[k].shape == a.shape and np.array_equal(ch[k], a, equal_nan=True)):
                moved.append((k, float(np.abs(ch[k].astype(np.float64) - a).max()) if ch[k].shape == a.shape else float("nan"),
                              float(np.abs(a).max())))
        else:
            spread = max(float(np.abs(b[k].astype(np.float64) - a).max()) for b in bs[1:])
            dist = min(float(np.abs(ch[k].astype(np.float64) - b[k]).max()) for b in bs)
            noisy.append((k, spread, dist, float(np.abs(a).max())))
    print(f"{len(names)} tensors; {stable} bit-identical across the {len(bs)} base runs, "
          f"{stable - len(moved)} of them bit-identical in {os.path.basename(change)}")
    for k, d, s in moved:
        print(f"  MOVED  {k}: max |d| {d:.3e} at scale {s:.3e}")
    for k, spread, dist, s in noisy:
        print(f"  noisy  {k}: base runs differ by {spread:.3e}, the change is {dist:.3e} from the nearest (scale {s:.3e})")
    if missing or extra:
        print(f"  NAMES DIFFER: missing {missing[:6]} extra {extra[:6]}")
    return 1 if moved or missing or extra else 0


def sizes(out):
    import stylish_tts_amd as S
    from stylish_tts_amd import lib as L
    from stylish_tts_amd.alignment import TrainableTextAligner
    from tests import align_cases as AC
    lib = L.load()
    lines = []

    def ask(tag, m, fn, *shape):
        for bf16 in (False, True):
            need = C.c_size_t()
            try:
                m.enable_training().set_train_opts(compute_bf16=bf16)
                m._ensure(torch.device(DEV))
                L.check(getattr(lib, fn)(m._handle, *shape, C.byref(need)))
                lines.append(f"{fn:42s} {tag:14s} {'x'.join(map(str, shape)):12s} {'bf16' if bf16 else 'fp32'} {need.value}")
            except Exception as e:  # (an entry that refuses a mode: say so and go on)
                lines.append(f"{fn:42s} {tag:14s} {'x'.join(map(str, shape)):12s} {'bf16' if bf16 else 'fp32'} "
                             f"refused: {str(e)[:80]}")

    sp = S.SpeechPredictor().to(DEV)
    for B, Lt, T in ((2, 40, 80), (32, 100, 520)):
        ask("speech", sp, "sty_speech_train_workspace_bytes", B, Lt, T)
        ask("speech", sp, "sty_vocoder_train_workspace_bytes", B, T)
    se = S.MelStyleEncoder().to(DEV)
    for B, T in ((2, 62), (32, 520)):
        ask("style", se, "sty_style_train_workspace_bytes", B, T)
    pse = S.PitchStyleEncoder().to(DEV)
    for B, T in ((2, 62), (32, 520)):
        ask("pitch_style", pse, "sty_pitch_style_train_workspace_bytes", B, T)
    dp = S.DurationPredictor().to(DEV)
    for B, Lt in ((2, 7), (32, 100)):
        ask("duration", dp, "sty_duration_train_workspace_bytes", B, Lt)
    pe = S.PitchEnergyPredictor().to(DEV)
    for B, Lt, T in ((2, 40, 80), (32, 100, 520)):
        ask("pitch_energy", pe, "sty_pitch_energy_train_workspace_bytes", B, Lt, T)
    al = TrainableTextAligner(AC.N_MELS, AC.TOKENS, hidden_dim=80).to(DEV)
    for B, T in ((3, 9), (32, 520)):
        ask("aligner", al, "sty_aligner_train_workspace_bytes", B, T)
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("model", choices=sorted(MODELS))
    r.add_argument("--bf16", action="store_true")
    r.add_argument("--out", required=True)
    c = sub.add_parser("cmp")
    c.add_argument("base", nargs="+")
    c.add_argument("--change", required=True)
    s = sub.add_parser("sizes")
    s.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cmd == "run":
        return run(a.model, a.bf16, a.out)
    if a.cmd == "cmp":
        return cmp(a.base, a.change)
    return sizes(a.out)


if __name__ == "__main__":
    sys.exit(main())
