"""Does a training step repeat?  Two fresh trainers of one stage, built from the same seeds on synthetic weights, run side by
side on the same batch; after every step everything that differs between the two is printed by name -- losses, gradients,
parameters, optimizer moments, buffers, tracked discriminator losses -- in backward order, so that the first name is the place
to look (what differs downstream of it usually differs because of it).

    python tools/repeat_step.py --stage acoustic|textual|duration|alignment [--compute bf16] [--steps N] [--deterministic]
                                [--B 5] [--T 80] [--L 24] [--no-adversarial]

Without --deterministic the default mode's order-dependent sums show up (departure 3); with it the exit status
is non-zero when anything differs.  B >= 3: a float sum of two terms onto zero does not depend on their order, so at B = 2 the
per-(b, c) sums over the batch repeat in either mode.  Uses the package alone (tests/test_deterministic_gpu.py builds its
trainers and compares their state with `build`, `batch_of` and `state_items` below).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stylish_tts_amd as S  # noqa: E402  (before torch: the package sets the hardware-queue count the step needs)
import torch  # noqa: E402

STAGES = ("acoustic", "textual", "duration", "alignment")
DISC_PICKS = (0, 2, 2)  # which spectrogram discriminator an acoustic step trains


def batch_of(B, T, L, device, seed=5, ragged=False):
    """One synthetic batch: T frames, L tokens drawn WITH repeats (the embedding's scatter-add then meets a row more than once),
    integer durations >= 1 summing to T.  ragged: text lengths L, L - 1, ... (the alignment stage's CTC targets)."""
    g = torch.Generator().manual_seed(seed)
    texts = torch.randint(1, 178, (B, L), generator=g)
    texts[:, 1::5] = texts[:, 0:1]  # every fifth token repeats the first, whatever the draw gave
    lengths = torch.full((B,), L, dtype=torch.int64)
    if ragged:
        lengths = torch.tensor([max(3, L - 2 * b) for b in range(B)])
        for b in range(B):
            texts[b, int(lengths[b]):] = 0
    dur = torch.ones(B, L)
    for b in range(B):
        dur[b] += torch.bincount(torch.multinomial(torch.ones(L), T - L, replacement=True, generator=g), minlength=L).float()
    t = torch.arange(300 * T) / 24000.0
    f0 = 110.0 + 100.0 * torch.rand(B, 1, generator=g)
    audio = sum(torch.sin(2 * torch.pi * f0 * (h + 1) * t) / (h + 1) for h in range(8)) * 0.15 \
        + 0.01 * torch.randn(B, 300 * T, generator=g)
    d = dict(audio_gt=audio, texts=texts, text_lengths=lengths, pitch=torch.rand(B, T, generator=g) * 200 + 80, durations=dur)
    return {k: v.to(device) for k, v in d.items()}


def build(stage, device, compute="fp32", deterministic=False, train_mode=True, lr=1e-3, adversarial=True):
    """A fresh trainer of `stage`: full-width synthetic weights (synthetic_weights.fill_state_dict), seeded discriminators."""
    from stylish_tts_amd import manifest as M
    from stylish_tts_amd.discriminators import ContextFreeDiscriminator, PitchDiscriminator, SpecDiscriminator
    from stylish_tts_amd.synthetic_weights import fill_state_dict
    common = dict(lr=lr, train_mode=train_mode, compute=compute, deterministic=deterministic, seed=0)

    def speech():
        sp, se = S.SpeechPredictor(), S.MelStyleEncoder()
        sp.load_state_dict(fill_state_dict(M.speech_predictor_manifest(), 0), strict=False)
        se.load_state_dict(fill_state_dict(M.style_encoder_manifest(), 0))
        return sp.to(device), se.to(device)

    if stage == "acoustic":
        from stylish_tts_amd.acoustic import AcousticTrainer
        sp, se = speech()
        torch.manual_seed(7)
        adv = dict(mrd=[SpecDiscriminator().to(device) for _ in range(3)], disc=ContextFreeDiscriminator().to(device)) \
            if adversarial else {}
        return AcousticTrainer(sp, se, **adv, **common)
    if stage == "textual":
        from stylish_tts_amd.textual import TextualTrainer
        sp, se = speech()
        pem, pse = S.PitchEnergyPredictor(), S.PitchStyleEncoder()
        pem.load_state_dict(fill_state_dict(M.pitch_energy_predictor_manifest(), 4))
        pse.load_state_dict(fill_state_dict(M.pitch_style_encoder_manifest(), 5))
        torch.manual_seed(11)
        return TextualTrainer(pem.to(device), pse.to(device), sp, se, PitchDiscriminator(dim_in=2, kernel=21).to(device), **common)
    if stage == "duration":
        from stylish_tts_amd.duration import DurationTrainer
        dpm, dse = S.DurationPredictor(), S.MelStyleEncoder()
        dpm.load_state_dict(fill_state_dict(M.duration_predictor_manifest(), 3))
        dse.load_state_dict(fill_state_dict(M.style_encoder_manifest(), 7))
        torch.manual_seed(11)
        return DurationTrainer(dpm.to(device), dse.to(device), PitchDiscriminator(dim_in=1, kernel=5).to(device), torch.ones(16),
                               **common)
    if stage == "alignment":
        from stylish_tts_amd.alignment import AlignmentTrainer, TrainableTextAligner
        if compute != "fp32":
            raise SystemExit("the alignment stage runs fp32 operands")
        torch.manual_seed(1234)
        m = TrainableTextAligner(80, 178, hidden_dim=80).to(device)
        return AlignmentTrainer(m, lr=lr, w_align=1.0, mean=-4.0, std=4.0, dropout=0.1, seed=0, deterministic=deterministic,
                                log=lambda *_: None)
    raise SystemExit(f"--stage must be one of {STAGES}")


def models_of(stage, tr):
    """The stage's trained models under the reference's keys, in the order their backward runs."""
    if stage == "acoustic":
        m = {"speech_predictor": tr.sp, "speech_style_encoder": tr.se}
        for i, d in enumerate(tr.mrd or []):
            m[f"mrd{i}"] = d
        if tr.disc is not None:
            m["disc"] = tr.disc
        return m
    if stage == "textual":
        return {"pitch_energy_predictor": tr.pep, "pe_style_encoder": tr.pse, "pitch_disc": tr.pitch_disc}
    if stage == "duration":
        return {"duration_predictor": tr.dp, "duration_style_encoder": tr.se, "dur_disc": tr.dur_disc}
    return {"text_aligner": tr.aligner}


def step(stage, tr, batch, i):
    """One optimizer step -> the logged losses as {name: tensor}"""
    if stage == "acoustic":
        kw = dict(disc_index=DISC_PICKS[i % len(DISC_PICKS)]) if tr.mrd is not None else {}
        out = tr.train_batch(seed=i, **kw, **batch)
        losses = {"loss.acoustic": out}
        if tr.mrd is not None:
            losses["loss.gan"] = tr.gan
        return losses
    if stage == "textual":
        return {"loss." + k: v for k, v in tr.train_batch(seed=i, **batch).items()}
    if stage == "duration":
        kw = {k: v for k, v in batch.items() if k != "pitch"}
        return {"loss." + k: v for k, v in tr.train_batch(**kw).items()}
    kw = {k: batch[k] for k in ("audio_gt", "texts", "text_lengths")}
    return {"loss." + k: v for k, v in tr.train_batch(seed=i, **kw).items()}


def state_items(stage, tr, losses=None):
    """[(name, tensor or number)] of everything a step leaves behind, in backward order: the losses, then per model (in the
    order of models_of) the gradients from the last parameter to the first, then parameters, optimizer moments and buffers the
    same way, then the tracked discriminator losses."""
    items = list((losses or {}).items())
    models = models_of(stage, tr)
    for key, m in models.items():
        for n, p in reversed(list(m.named_parameters())):
            if p.grad is not None:
                items.append((f"grad  {key}.{n}", p.grad))
    for key, m in models.items():
        for n, p in reversed(list(m.named_parameters())):
            items.append((f"param {key}.{n}", p.detach()))
    for key, o in tr.opt.items():
        for what, ts in (("exp_avg", o.m), ("exp_avg_sq", o.v)):
            for j, t in reversed(list(enumerate(ts))):
                items.append((f"{what} {key}[{j}]", t))
    for key, m in models.items():
        params = {n for n, _ in m.named_parameters()}
        for n, t in reversed(list(m.state_dict().items())):
            if n not in params:
                items.append((f"buffer {key}.{n}", t))
    helpers = list(getattr(tr, "disc_helpers", []) or []) + ([tr.disc_helper] if getattr(tr, "disc_helper", None) is not None else [])
    for j, h in enumerate(helpers):
        items.append((f"last_loss helper{j}", h.last_loss))
    if stage == "alignment" and tr.priors.log_priors is not None:
        items.append(("label priors", tr.priors.log_priors))
    return items


def differences(a, b):
    """names (with the largest |difference|) of the items that are not equal bit for bit; a and b from state_items"""
    out = []
    assert [n for n, _ in a] == [n for n, _ in b], "the two trainers hold different state"
    for (name, x), (_, y) in zip(a, b):
        if torch.is_tensor(x):
            if not torch.equal(x, y):
                d = (x.double() - y.double()).abs()
                out.append((name, float(d.max()), int((d > 0).sum()), x.numel()))
        elif x != y:
            out.append((name, abs(float(x) - float(y)) if x is not None and y is not None else float("nan"), 1, 1))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--stage", required=True, choices=STAGES)
    ap.add_argument("--compute", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--T", type=int, default=80)
    ap.add_argument("--L", type=int, default=24)
    ap.add_argument("--no-adversarial", action="store_true", help="acoustic stage without the discriminators")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: there is no CPU training path in this package")
    from stylish_tts_amd import lib as L
    device = torch.device("cuda:0")
    batch = batch_of(a.B, a.T, a.L, device, ragged=a.stage == "alignment")
    pair = [build(a.stage, device, compute=a.compute, deterministic=a.deterministic, adversarial=not a.no_adversarial)
            for _ in range(2)]
    print(f"{a.stage}, {a.compute}, B {a.B} T {a.T} L {a.L}, deterministic mode {'on' if L.get_deterministic() else 'off'}")
    total = 0
    for i in range(a.steps):
        losses = [step(a.stage, tr, batch, i) for tr in pair]
        torch.cuda.synchronize()
        diff = differences(state_items(a.stage, pair[0], losses[0]), state_items(a.stage, pair[1], losses[1]))
        total += len(diff)
        print(f"step {i}: {len(diff)} items differ")
        for name, worst, n, numel in diff:
            print(f"  {name:72s} max|diff| {worst:9.3e}  {n} of {numel} elements")
    if a.deterministic and total:
        print("the deterministic mode did not repeat")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
