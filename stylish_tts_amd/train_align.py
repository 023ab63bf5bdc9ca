"""The `train-align` entry point on the reference's unchanged YAML files (train/cli.py:60-108 `train_align`; the `alignment`
stage of train/train.py:76-338, :341-450): config.yml + model.yml + a dataset without alignments -> a trained TextAligner ->
`<dataset.path>/<alignment_model_path>`, the file `python -m stylish_tts_amd.align` starts from.

    python -m stylish_tts_amd.train_align CONFIG.yml --model-config MODEL.yml --out OUT [--checkpoint DIR] [--reset-stage]

or `stylish_tts_amd.train_align.train_align(config_path, model_config_path, out, checkpoint, reset_stage)` -- the reference
command's arguments in the reference command's order.  The stage is its own command, as in the reference; `train --stage`
keeps its three choices.

Per step (stylish_tts_amd/alignment.py): wave -> mel (the `text_aligner` section's n_fft / win_length, normalised) ->
TextAligner in its training graph (batch-statistics BatchNorm, hash dropout) -> CTC loss with label priors from the second
epoch on -> backward -> AdamW.  Every val_interval / save_interval steps the loop also TRAINS one pass over the validation
split (train/train.py:417-423: `align` labels that split too), then validates it: align_loss and the forced alignment's
confidence.  Checkpoints are accelerate-layout directories with the aligner as `pytorch_model.bin` (stage_io.MODEL_ORDER
index 0), every save_interval steps and `checkpoint_final` at the end; the label priors' sums travel in `label_priors.bin`.
One process (the priors' all-gather is not built); no batch-size probe, as in the other stages (train.py's docstring).
"""
import os
import os.path as osp
import random
import shutil
import time

import torch

from . import lib as L

STAGE = "alignment"


def _log(msg):
    print(f"[stylish_tts_amd.train_align] {msg}", flush=True)


class AlignContext:
    """what the loop holds: configs, the two splits, normalization, manifest, the trainer"""


def _dataset(lines, config, model_config):
    from . import data as D
    ds = config.dataset
    return D.SampleDataset(data_list=lines, root_path=osp.join(ds.path, ds.wav_path), pitch_path=None, alignment_path=None,
                           text_cleaner=D.TextCleaner(getattr(model_config, "symbol", None)),
                           sample_rate=model_config.sample_rate, hop_length=model_config.hop_length,
                           coarse_multiplier=model_config.coarse_multiplier)


def train_align_model(config, model_config, out_dir, checkpoint="", reset_stage=False, config_path="", model_config_path="",
                      max_steps=None, device=None, log=_log, deterministic=False):
    """train_model (train/train.py:76-338) for the alignment stage.  `deterministic`: the library's deterministic mode.  `max_steps`: stop after that many optimizer steps of the
    training split (tests; None = the plan's epochs).  Returns the context (.trainer, .manifest, .aligner)."""
    from safetensors.torch import save_file
    from . import data as D
    from . import stage_io as IO
    from .align import ALIGNER_MEL
    from .alignment import AlignmentTrainer, TrainableTextAligner
    if deterministic:  # first of all: nothing is sized, loaded or normalised in the other mode
        L.set_deterministic(True)
    random.seed(1)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise L.StyError("train-align runs in one process: the label priors' all-gather over ranks is not built")
    if STAGE not in config.training_plan:
        raise L.StyError("training_plan.alignment is missing from the config")
    if config.training.device != "cuda":
        raise L.StyError(f"training.device = {config.training.device!r}: this path runs on a HIP device only ('cuda')")
    if not torch.cuda.is_available():
        raise L.StyError("no HIP device: there is no CPU training path in this package")
    ds = config.dataset
    path = lambda p: osp.join(ds.path, p)
    for what in ("train_data", "val_data", "wav_path"):
        if not osp.exists(path(ds[what])):
            raise L.StyError(f"dataset.{what} not found at {path(ds[what])}")
    device = torch.device(device or "cuda:0")
    torch.cuda.set_device(device)
    ctx = AlignContext()
    ctx.config, ctx.model_config, ctx.device = config, model_config, device
    splits = {}
    for what in ("train_data", "val_data"):
        with open(path(ds[what]), encoding="utf-8") as f:
            splits[what] = [ln for ln in f.read().splitlines() if ln.strip()]
    train_set, val_set = _dataset(splits["train_data"], config, model_config), _dataset(splits["val_data"], config, model_config)
    time_bins, _ = train_set.time_bins()
    val_bins, _ = val_set.time_bins()
    plan = config.training_plan[STAGE]
    max_epoch, lr = int(plan["epochs"]), float(plan["lr"])
    stage_dir = osp.join(out_dir, STAGE)
    os.makedirs(stage_dir, exist_ok=True)
    for p in (config_path, model_config_path):
        if p:
            shutil.copy(p, osp.join(stage_dir, osp.basename(p)))
    batch_sizes = IO.BatchSizes(stage_dir, STAGE)  # as train._Stage: no probe, every bin at probe_batch_max
    batch_sizes.load_batch_sizes()
    if not batch_sizes.batch_sizes_exist():
        for b in list(time_bins) + list(val_bins):
            batch_sizes.set_batch_size(b, int(plan["probe_batch_max"]))
        batch_sizes.save_batch_sizes()
    ctx.manifest, ctx.normalization = IO.Manifest(), IO.NormalizationStats()
    m = ctx.manifest
    if checkpoint:
        IO.load_checkpoint(checkpoint, {}, manifest=m, normalization=ctx.normalization)
    how = IO.init_normalization(ctx.normalization, stage_dir, ds.path, splits["train_data"], path(ds.wav_path), model_config,
                                device=str(device), log=log)
    log(f"normalization statistics: {how} (mel log mean {ctx.normalization.mel_log_mean:.4f}, std "
        f"{ctx.normalization.mel_log_std:.4f})")
    ta = getattr(model_config, "text_aligner", None) or {}
    tokens = int(model_config.text_encoder.tokens)
    ctx.aligner = TrainableTextAligner(int(model_config.n_mels), tokens, int(ta.get("hidden_dim", 640))).to(device)
    ctx.trainer = tr = AlignmentTrainer(
        ctx.aligner, lr=lr, w_align=float(config.loss_weight.get("align_loss", 1.0)), mean=ctx.normalization.mel_log_mean,
        std=ctx.normalization.mel_log_std, dropout=float(ta.get("dropout", 0.1)), seed=0,
        hop_length=model_config.hop_length * model_config.coarse_multiplier, n_fft=int(ta.get("n_fft", ALIGNER_MEL["n_fft"])),
        win_length=int(ta.get("win_length", ALIGNER_MEL["win_length"])), log=log, deterministic=deterministic)
    fast_forward = 0
    if checkpoint:
        st = tr.checkpoint_state()
        IO.load_checkpoint(checkpoint, st["models"], optimizers=st["optimizers"], allow_mixed_steps=True)
        pri = osp.join(checkpoint, "label_priors.bin")
        if osp.exists(pri):
            tr.priors.load_state_dict(torch.load(pri, map_location="cpu"), device=device)
        if m.stage == STAGE and not reset_stage:
            fast_forward = m.current_step
        else:
            m.current_epoch, m.current_step = 1, 0
        log(f"loaded checkpoint {checkpoint}")
    else:
        m.current_epoch, m.current_total_step, m.current_step = 1, 0, 0
    m.stage = STAGE
    m.best_loss = float("inf")
    m.steps_per_epoch = batch_sizes.get_steps(time_bins)
    step_limit = max(1, m.steps_per_epoch * max_epoch)
    cfg = config.training
    hop = model_config.hop_length * model_config.coarse_multiplier
    collate = D.Collater(stage=STAGE, hop_length=hop)
    sampler = D.LengthBinSampler(time_bins, batch_sizes.get_batch_size, shuffle=True, seed=0, epoch=m.current_epoch)
    loader = torch.utils.data.DataLoader(train_set, batch_sampler=sampler, num_workers=0, collate_fn=collate)
    val_loader = torch.utils.data.DataLoader(
        val_set, batch_sampler=D.LengthBinSampler(val_bins, batch_sizes.get_batch_size, shuffle=False), num_workers=0,
        collate_fn=collate)

    def inputs(batch):
        waves, texts, text_lengths, paths, _, _ = batch
        return dict(audio_gt=waves.to(device), texts=texts.to(device), text_lengths=text_lengths.to(device), paths=paths)

    def save(prefix, long):
        d = IO.checkpoint_dir(stage_dir, prefix, m, long)
        IO.save_checkpoint(d, manifest=m, normalization=ctx.normalization, **tr.checkpoint_state())
        torch.save(tr.priors.state_dict(), osp.join(d, "label_priors.bin"))

    def validate():
        total, frames, loss_sum, n = 0.0, 0, 0.0, 0
        for batch in val_loader:
            out, (conf, fr) = tr.validate(**inputs(batch))
            total, frames = total + float(conf), frames + fr
            loss_sum, n = loss_sum + float(out["align_loss"]), n + 1
        loss = loss_sum / max(n, 1)
        m.best_loss = min(m.best_loss, loss)
        log(f"validation: align_loss {loss:.4f} confidence {total / max(frames, 1):.4f} ({frames} frames)")

    def finish():
        validate()
        save("checkpoint_final", False)
        out = path(getattr(ds, "alignment_model_path", "alignment_model.safetensors"))
        save_file({k: v.detach().cpu().contiguous() for k, v in ctx.aligner.state_dict().items()}, out)  # train.py:445-450
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
        log(f"{seen} utterances in {dt:.2f} s ({seen / max(dt, 1e-9):.1f} utterances/s, {total} steps, {tr.skipped} skipped); "
            f"wrote {out}")
        return ctx

    log(f"training stage {STAGE}: {max_epoch} epochs, lr {lr:g}, {m.steps_per_epoch} steps per epoch")
    total, seen = 0, 0
    ctx.applied_priors_steps = 0
    t0 = time.perf_counter()
    while m.current_epoch <= max_epoch:
        sampler.set_epoch(m.current_epoch)
        for batch in loader:
            if fast_forward > 0:
                fast_forward -= 1
                continue
            tr.schedule(m.current_step + (m.current_epoch - 1) * m.steps_per_epoch, step_limit)
            ctx.applied_priors_steps += tr.priors.log_priors is not None
            out = tr.train_batch(seed=m.current_total_step, **inputs(batch))
            m.current_total_step += 1
            m.current_step += 1
            total += 1
            seen += batch[0].shape[0]
            m.total_trained_audio_seconds += float(batch[0].shape[0] * batch[0].shape[1]) / model_config.sample_rate
            num = m.current_step + (m.current_epoch - 1) * m.steps_per_epoch
            if num % int(cfg.log_interval) == 0:
                log(f"{STAGE} epoch {m.current_epoch} step {m.current_step}/{m.steps_per_epoch}: align_loss "
                    f"{float(out['align_loss']):.4f}")
            do_val, do_save = num % int(cfg.val_interval) == 0, num % int(cfg.save_interval) == 0
            if do_val or do_save:
                for vb in val_loader:  # train/train.py:417-423: one training pass over the validation split
                    tr.train_batch(seed=m.current_total_step, **inputs(vb))
                    seen += vb[0].shape[0]
                validate()
            if do_save:
                save("checkpoint", True)
            if max_steps is not None and total >= max_steps:
                return finish()
        tr.on_epoch_end()
        m.current_epoch += 1
        m.current_step = 0
        m.training_log.append(f"Completed 1 epoch of {STAGE} training")
    return finish()


def train_align(config_path, model_config_path, out, checkpoint="", reset_stage=False, **kw):
    """train/cli.py:60-108 `train_align`: same arguments, same order."""
    from .config import load_config_yaml
    from .train import get_model_config
    model_config = get_model_config(model_config_path)
    config = load_config_yaml(config_path)
    return train_align_model(config, model_config, out, checkpoint, reset_stage, config_path, model_config_path, **kw)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m stylish_tts_amd.train_align", description=__doc__.split("\n\n")[0])
    ap.add_argument("config_path")
    ap.add_argument("--model-config", dest="model_config_path", default="")
    ap.add_argument("--out", required=True, help="output directory (the stage's sub-directory holds the checkpoints)")
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--reset-stage", dest="reset_stage", action="store_true")
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--deterministic", action="store_true",
                    help="fixed-order sums: a seed reproduces the run to the bit (STY_DETERMINISTIC=1 does the same)")
    a = ap.parse_args(argv)
    train_align(a.config_path, a.model_config_path, a.out, a.checkpoint, a.reset_stage, max_steps=a.max_steps,
                deterministic=a.deterministic)


if __name__ == "__main__":
    main()
