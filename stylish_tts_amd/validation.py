"""The validation pass of the three stages this path trains (train/train.py:399-442, train/stage.py:149-422 `Stage.validate`,
train/loss_log.py:72-124): the val split through the stage trainer's `validate`, the logs combined into one record, `best_loss`,
the reference's log line, listening samples as wav files.

    pass_ = ValidationPass(config, model_config, stage, out_dir, batch_size_of, device, log=log)   # val split + length-bin
                                                                    # sampler at the stage's batch sizes; no device touched
    record = pass_.run(trainer, manifest, loss_weight)              # {"step", "stage", "total", "metrics", "best_before",
                                                                    #  "batches", "skipped", "samples"} (+ "slm" with
                                                                    #  `train --slm`: trainer.slm is set)

What the reference also draws and this does not: mel / attention figures and tensorboard scalars (neither matplotlib's figure
path nor tensorboard is part of this package's dependencies); the record goes to `<out>/<stage>/eval/validation.jsonl` instead.
Everything that decides something -- which steps validate, which rank, which utterances become samples, how logs combine -- is
a small pure function below, testable without a device.
"""
import contextlib
import json
import math
import os
import os.path as osp
import wave

from . import lib as L

SAMPLE_COUNT_DEFAULT = 10  # config/config.yml:61-63 (lib/config_loader.py:245-250: force_samples defaults to [])


# ---- pure rules -------------------------------------------------------------------------------------------------------------
def validation_settings(config):
    """(sample_count, force_samples) of config.yml's `validation` section, the reference's defaults when it is absent"""
    v = config.get("validation") if hasattr(config, "get") else getattr(config, "validation", None)
    v = v or {}
    return int(v.get("sample_count", SAMPLE_COUNT_DEFAULT)), list(v.get("force_samples") or [])


def should_validate(num, val_interval, save_interval, *, stage_end=False, max_steps_exit=False):
    """train/train.py:399-429.  After a step (stage_end=False): a pass runs when the stage's step count `num` is a multiple of
    val_interval or of save_interval (before the save).  Where the loop leaves the stage (stage_end=True): a pass runs at the
    natural end, in front of checkpoint_final, and not on the max_steps early exit (a test hook, which adds no pass)."""
    if stage_end:
        return not max_steps_exit
    return num % int(val_interval) == 0 or num % int(save_interval) == 0


def rank_validates(rank, world=1):
    """Rank 0 alone runs the pass, on the whole val split and without a collective: the ranks' step counts can differ, so a
    collective keyed on the step would mismatch; the other ranks go on to their next step and wait in its gradient exchange."""
    del world
    return int(rank) == 0


def combine(logs):
    """combine_logs (loss_log.py:109-124): the mean of each metric over the batches that logged it"""
    totals, counts = {}, {}
    for log in logs:
        for k, v in log.items():
            totals[k] = totals.get(k, 0.0) + float(v)
            counts[k] = counts.get(k, 0) + 1
    return {k: totals[k] / counts[k] for k in totals}


def total_loss(metrics, loss_weight):
    """LossLog.calculate_metrics (loss_log.py:72-80): sum(metric * loss_weight[key]); an unknown key weighs 1"""
    return sum(v * float(loss_weight.get(k, 1.0)) for k, v in metrics.items())


def update_best(best, total):
    """stage.py:415-420 -> (new best_loss, improved)"""
    return (total, True) if total < best else (best, False)


def select_samples(batch_index, paths, sample_count, force_samples):
    """stage.py:175-197 -> [(index in the batch, sample number)]: with force_samples the listed paths (numbered by their place
    in the list), otherwise utterance 0 of the first sample_count batches"""
    if len(force_samples):
        where = {p: j for j, p in enumerate(force_samples)}
        return [(i, where[p]) for i, p in enumerate(paths) if p in where]
    return [(0, batch_index)] if batch_index < sample_count else []


def log_line(step, total, metrics, best):
    """loss_log.py:31-42"""
    s = f"Validation step {step}: loss: {total:.3f}, " + ", ".join(f"{k}: {v:.3f}" for k, v in metrics.items())
    return s + (f", (best was {best})" if best != float("inf") else "")


def finite_or_none(v):
    """JSON has no Infinity / NaN: a total of a pass whose every batch was skipped, a best_loss nobody has set yet and a
    metric that is not a number are written as null"""
    return v if math.isfinite(v) else None


def record_line(record):
    """the pass's record as one line of strict JSON (what eval/validation.jsonl holds)"""
    return json.dumps(record, allow_nan=False)


def write_wav(path, audio, sample_rate):
    """float audio [samples] (host) -> mono PCM16, saturating (speak.to_int16)"""
    from .speak import to_int16
    os.makedirs(osp.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(to_int16(audio).astype("<i2").tobytes())


# ---- the trainers' side -------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def eval_opts(models, bf16):
    """The inference entry points run the eval-mode graph whatever the train opts say; the one field they read is the compute
    mode.  Inside: every model's compute_bf16 is the stage's.  On exit: every model's train opts are EXACTLY what they were (the
    object and the library's copy) -- train_batch sets its own each step only when train_mode is on, the train_mode=False / bf16
    constructor path sets them once.  A model whose mode had to change is invalidated both ways (its packed weights are the
    other mode's)."""
    import ctypes as C
    lib = L.load()
    touched = []
    for m in models:
        prev = getattr(m, "_train_opts", None)
        if bool(prev.compute_bf16 if prev is not None else False) == bool(bf16):
            continue
        now = L.TrainOpts.from_buffer_copy(prev) if prev is not None else m.set_train_opts()._train_opts
        now.compute_bf16 = int(bool(bf16))
        m._train_opts = now
        touched.append((m, prev))
        if m._handle is not None:
            L.check(lib.sty_model_set_train_opts(m._handle, C.byref(now)))
            L.check(lib.sty_model_invalidate(m._handle))
    try:
        yield
    finally:
        for m, prev in touched:
            if prev is None:
                m.set_train_opts()  # the library's defaults
            m._train_opts = prev
            if m._handle is not None:
                if prev is not None:
                    L.check(lib.sty_model_set_train_opts(m._handle, C.byref(prev)))
                L.check(lib.sty_model_invalidate(m._handle))


def or_refusal(make):
    """make() -- or, when a HOST-SIDE check refused it (lib.refused_on_host), the StyError it raised, handed back as a value:
    one listening sample that cannot be made does not cost the batch its numbers.  A StyDeviceError (the library's STY_EHIP) and
    every other exception propagate: nothing may be launched behind a device fault."""
    try:
        return make()
    except L.StyError as e:
        if not L.refused_on_host(e):
            raise
        return e


# ---- the pass ---------------------------------------------------------------------------------------------------------------
def load_val_lines(config):
    """the non-blank lines of dataset.val_data; a missing list is refused here, before any device work"""
    ds = config.dataset
    path = osp.join(ds.path, ds.val_data)
    if not osp.isfile(path):
        raise L.StyError(f"dataset.val_data not found at {path}")
    with open(path, encoding="utf-8") as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    if not lines:
        raise L.StyError(f"dataset.val_data at {path} lists no utterance")
    return lines


def run_batches(validate, batches, *, sample_count, force_samples, log, on_sample=None):
    """`validate(batch, wanted)` -> (log dict, extra) over `batches` of (paths, batch).  A batch that a HOST-SIDE check refuses
    (lib.refused_on_host: a StyError of a Python shape check or a refusal status of the library) is logged and skipped
    (stage.py:407-413).  Everything else propagates and ends the pass with the next batch never started: any other exception, and
    StyDeviceError -- the library's STY_EHIP, which reaches Python through the same lib.check as the refusals do -- so that nothing
    is launched behind a device fault.  -> (list of float logs, skipped batch indices)"""
    logs, skipped = [], []
    for index, (paths, batch) in enumerate(batches):
        wanted = select_samples(index, paths, sample_count, force_samples)
        try:
            out, extra = validate(batch, wanted)
        except L.StyError as e:
            if not L.refused_on_host(e):
                raise
            log(f"validation batch {index} skipped: {e}")
            skipped.append(index)
            continue
        logs.append({k: float(v) for k, v in out.items()})
        if on_sample is not None:
            for i, j in wanted:
                on_sample(i, j, paths[i], batch, extra)
    return logs, skipped


class ValidationPass:
    """The val split of one stage and what a pass writes under `<out>/<stage>/eval/`."""

    def __init__(self, config, model_config, stage, out_dir, batch_size_of, device, log=print):
        from . import data as D
        self.config, self.model_config, self.stage, self.device, self.log = config, model_config, stage, device, log
        self.lines = load_val_lines(config)  # (first: nothing below runs without the list)
        ds = config.dataset
        path = lambda p: osp.join(ds.path, p)
        self.dataset = D.SampleDataset(data_list=self.lines, root_path=path(ds.wav_path), pitch_path=path(ds.pitch_path),
                                       alignment_path=path(ds.alignment_path), sample_rate=model_config.sample_rate,
                                       hop_length=model_config.hop_length, coarse_multiplier=model_config.coarse_multiplier)
        self.bins, _ = self.dataset.time_bins()
        self.sampler = D.LengthBinSampler(self.bins, batch_size_of, shuffle=False)
        self.collate = D.Collater(stage=stage, hop_length=model_config.hop_length)
        self.sample_count, self.force_samples = validation_settings(config)
        self.eval_dir = osp.join(out_dir, "eval")
        self.gt_written = set()

    def batches(self):
        import torch
        loader = torch.utils.data.DataLoader(self.dataset, batch_sampler=self.sampler, num_workers=0, collate_fn=self.collate)
        for batch in loader:
            yield list(batch[3]), batch

    def run(self, trainer, manifest, loss_weight):
        """One pass: validate every batch, combine, log the reference's line, update manifest.best_loss, write the samples and
        append the record to eval/validation.jsonl.  -> the record"""
        from .data import to_step_inputs
        step = int(manifest.current_total_step)
        sr = int(self.model_config.sample_rate)
        samples, slm_logs = [], []

        def validate(batch, wanted):
            kw = to_step_inputs(batch, self.device)
            if self.stage == "duration":
                kw["samples"] = [i for i, _ in wanted]
            out, extra = trainer.validate(**kw)
            value = extra.get("slm")  # (`train --slm`, acoustic and textual stage)
            if isinstance(value, Exception):  # refused on the host: this batch has no slm value; its metrics stand
                self.log(f"validation batch: slm value skipped: {value}")
            elif value is not None:
                slm_logs.append({"slm": float(value)})
            return out, extra

        def on_sample(i, j, path, batch, extra):
            entry = {"sample": j, "path": path}
            audio = extra["audio"][i] if self.stage == "duration" else extra["audio"][i:i + 1]
            if isinstance(audio, Exception):
                self.log(f"validation sample {j} ({path}) skipped: {audio}")
                entry["skipped"] = str(audio)
            else:
                name = osp.join(self.eval_dir, f"step_{step}", f"sample_{j}.wav")
                write_wav(name, audio.reshape(-1).float().cpu().numpy(), sr)
                entry["file"] = osp.relpath(name, self.eval_dir)
            if j not in self.gt_written:
                gt = osp.join(self.eval_dir, f"sample_{j}_gt.wav")
                if not osp.exists(gt):
                    write_wav(gt, batch[0][i].float().cpu().numpy(), sr)
                self.gt_written.add(j)
            if extra.get("per_item") is not None:  # the sample's own mel error: mean_r sum|t - p| / (sum|t| + 1e-6)
                it = extra["per_item"][i].cpu()
                entry["mel"] = finite_or_none(float((it[:, 0] / (it[:, 1] + 1e-6)).mean()))
            samples.append(entry)

        logs, skipped = run_batches(validate, self.batches(), sample_count=self.sample_count,
                                    force_samples=self.force_samples, log=self.log, on_sample=on_sample)
        metrics = combine(logs)
        total = total_loss(metrics, loss_weight) if logs else float("inf")
        best_before = float(manifest.best_loss)
        self.log(log_line(step, total, metrics, best_before) if logs else
                 f"Validation step {step}: every batch was skipped")
        manifest.best_loss, _ = update_best(best_before, total)
        record = {"step": step, "stage": self.stage, "total": finite_or_none(total),
                  "metrics": {k: finite_or_none(v) for k, v in metrics.items()}, "best_before": finite_or_none(best_before),
                  "batches": len(logs), "skipped": skipped, "samples": samples}
        if slm_logs:
            # The slm value (slm.WavLMLoss, unweighted; the reference's training log shows this term, its validation does not
            # compute it): combined over the batches as the metrics are, one line of its own and one top-level field.  metrics,
            # total, best_before and manifest.best_loss above never see it: best_loss decides which checkpoint is best.
            slm_value = combine(slm_logs)["slm"]
            self.log(f"Validation step {step}: slm: {slm_value:.3f}")
            record["slm"] = finite_or_none(slm_value)
        os.makedirs(self.eval_dir, exist_ok=True)
        with open(osp.join(self.eval_dir, "validation.jsonl"), "a", encoding="utf-8") as f:
            f.write(record_line(record) + "\n")
        return record
