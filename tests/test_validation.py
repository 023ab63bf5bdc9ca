"""The validation pass without a device: the C-ABI surface of the forward-only loss entries, the pure rules of
stylish_tts_amd/validation.py (when, which rank, which samples, how logs combine, best_loss), the skip path on a stub trainer,
and the golden fixture of the duration stage's samples."""
import ctypes as C
import json
import math
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sty_mel_loss_workspace_bytes", "sty_mel_loss_features", "sty_mel_loss_fwd", "sty_pitch_loss_fwd", "sty_duration_loss_fwd")


def _ctype(decl):
    """one parameter of a header declaration -> the ctypes type lib.py must bind it with"""
    decl = decl.strip()
    if "*" in decl:
        base = decl.replace("const", "").split("*")[0].strip()
        return {"size_t": C.POINTER(C.c_size_t), "int": C.POINTER(C.c_int)}.get(base, C.c_void_p)
    base = decl.replace("const", "").split()[0]
    return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}[base]


def test_abi_surface_lists_the_new_symbols_with_the_headers_signatures():
    import __graft_entry__ as ge
    ge.build()
    from stylish_tts_amd import lib as L
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "stylish_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/stylish_hip.h"
        want = [_ctype(a) for a in m.group(1).split(",")]
        res, args = L.SYMBOLS[name]
        assert res is C.c_int and args == want, (name, args, want)
        assert hasattr(lib, name), name


def test_loss_entries_refuse_bad_arguments_on_the_host():
    """NULL outputs, N = 1024 (the 2048-point transform reflect-pads 1024 samples) and a short workspace are refused with
    sty_last_error set, before anything could be launched (no device here)"""
    import __graft_entry__ as ge
    ge.build()
    from stylish_tts_amd import lib as L
    lib = L.load()
    need, off, fr = C.c_size_t(), C.c_size_t(), C.c_int()
    assert lib.sty_mel_loss_workspace_bytes(2, 1024, C.byref(need)) != 0 and b"1024" in lib.sty_last_error()
    assert lib.sty_mel_loss_workspace_bytes(0, 2048, C.byref(need)) != 0
    assert lib.sty_mel_loss_workspace_bytes(2, 1025, None) != 0
    assert lib.sty_mel_loss_workspace_bytes(2, 1025, C.byref(need)) == 0 and need.value > 0
    n1 = need.value
    assert lib.sty_mel_loss_workspace_bytes(2, 1025, C.byref(need)) == 0 and need.value == n1  # a function of the shape
    assert lib.sty_mel_loss_features(2, 1025, 3, 0, C.byref(off), C.byref(fr)) != 0
    assert lib.sty_mel_loss_features(2, 1025, 2, 1, C.byref(off), C.byref(fr)) == 0 and fr.value == 1025 // 512 + 1
    assert off.value + 4 * 128 * 2 * fr.value <= n1
    fake = C.c_void_p(4096)  # never dereferenced: every call below is refused on the host
    assert lib.sty_mel_loss_fwd(2, 1024, fake, fake, fake, None, fake, n1, None) != 0
    assert lib.sty_mel_loss_fwd(2, 1025, fake, fake, None, None, fake, n1, None) != 0
    assert lib.sty_mel_loss_fwd(2, 1025, fake, fake, fake, None, fake, n1 - 1, None) != 0
    assert b"workspace too small" in lib.sty_last_error()
    assert lib.sty_pitch_loss_fwd(2, 8, fake, fake, None, fake, 32, None) != 0
    assert lib.sty_pitch_loss_fwd(2, 8, fake, fake, fake, fake, 31, None) != 0
    assert lib.sty_pitch_loss_fwd(2, 0, fake, fake, fake, fake, 32, None) != 0
    assert lib.sty_duration_loss_fwd(2, 8, 16, fake, fake, fake, fake, fake, fake, None, fake, 32, None) != 0
    assert lib.sty_duration_loss_fwd(2, 8, 33, fake, fake, fake, fake, fake, fake, fake, fake, 32, None) != 0
    assert lib.sty_duration_loss_fwd(2, 8, 16, fake, fake, fake, fake, fake, fake, fake, fake, 31, None) != 0


def test_combine_total_and_best_loss_by_hand():
    from stylish_tts_amd import validation as V
    logs = [{"mel": 1.0, "pitch": 4.0}, {"mel": 2.0}, {"mel": 6.0, "pitch": 2.0}]  # batch 1 logged no pitch
    m = V.combine(logs)
    assert m == {"mel": 3.0, "pitch": 3.0}  # (1 + 2 + 6) / 3, (4 + 2) / 2
    w = {"mel": 5, "pitch": 8}
    assert V.total_loss(m, w) == 5 * 3.0 + 8 * 3.0
    assert V.total_loss({"mel": 2.0, "other": 0.5}, w) == 10.5  # an unknown key weighs 1 (loss_log.py:64-70)
    assert V.combine([]) == {}
    best, improved = V.update_best(float("inf"), 39.0)
    assert (best, improved) == (39.0, True)
    assert V.update_best(39.0, 39.0) == (39.0, False)  # "lower", not "lower or equal" (stage.py:415-420)
    assert V.update_best(39.0, 40.0) == (39.0, False)
    assert V.update_best(39.0, 38.5) == (38.5, True)
    assert V.log_line(7, 39.0, m, float("inf")) == "Validation step 7: loss: 39.000, mel: 3.000, pitch: 3.000"
    assert V.log_line(7, 39.0, m, 41.5).endswith(", (best was 41.5)")


def test_sample_selection_with_and_without_force_samples():
    from stylish_tts_amd import validation as V
    paths = ["a.wav", "b.wav", "c.wav"]
    assert V.select_samples(0, paths, 2, []) == [(0, 0)]
    assert V.select_samples(1, paths, 2, []) == [(0, 1)]
    assert V.select_samples(2, paths, 2, []) == []
    assert V.select_samples(0, paths, 0, []) == []
    force = ["c.wav", "zz.wav", "a.wav"]
    assert V.select_samples(5, paths, 2, force) == [(0, 2), (2, 0)]  # numbered by their place in the list; any batch
    assert V.select_samples(0, ["q.wav"], 2, force) == []           # force_samples switches the first-batches rule off
    cfg = types.SimpleNamespace(validation={"sample_count": 3, "force_samples": ["x.wav"]})
    assert V.validation_settings(cfg) == (3, ["x.wav"])
    assert V.validation_settings(types.SimpleNamespace()) == (10, [])  # the section is absent: the reference's defaults
    assert V.validation_settings({"validation": {"sample_count": 1}}) == (1, [])


def test_when_to_validate_rule():
    from stylish_tts_amd import validation as V
    assert V.should_validate(10, 10, 1000)          # val_interval
    assert V.should_validate(1000, 300, 1000)       # save_interval (the pass runs before the save)
    assert not V.should_validate(7, 10, 1000)
    assert not V.should_validate(3, 1000, 1000)     # the c1 test's config: no pass in three steps
    assert V.should_validate(7, 10, 1000, stage_end=True)                            # the natural end of a stage
    assert not V.should_validate(7, 10, 1000, stage_end=True, max_steps_exit=True)   # the max_steps exit adds none
    assert V.should_validate(4, 2, 1000)            # ... and takes none away: step 4 of max_steps=4 at val_interval=2


def test_rank_rule():
    from stylish_tts_amd import validation as V
    assert V.rank_validates(0, 1) and V.rank_validates(0, 8)
    assert not any(V.rank_validates(r, 8) for r in range(1, 8))
    import inspect
    src = inspect.getsource(V)
    assert "all_reduce" not in src and "torch.distributed" not in src  # no collective of any kind in the pass


class _Stub:
    def __init__(self, fail_on, exc):
        self.fail_on, self.exc, self.seen = fail_on, exc, []

    def validate(self, batch, wanted):
        self.seen.append(batch)
        if batch == self.fail_on:
            raise self.exc
        return {"mel": torch.tensor(float(batch + 1))}, {"wanted": wanted}


def test_a_batch_refused_on_the_host_is_skipped_and_any_other_error_propagates():
    from stylish_tts_amd import validation as V
    from stylish_tts_amd.lib import StyError
    batches = [([f"{i}.wav"], i) for i in range(3)]
    lines, sampled = [], []
    stub = _Stub(1, StyError("texts too long"))
    logs, skipped = V.run_batches(stub.validate, batches, sample_count=3, force_samples=[], log=lines.append,
                                  on_sample=lambda i, j, path, batch, extra: sampled.append((i, j, path)))
    assert stub.seen == [0, 1, 2] and skipped == [1]
    assert logs == [{"mel": 1.0}, {"mel": 3.0}]
    assert len(lines) == 1 and "batch 1 skipped" in lines[0] and "texts too long" in lines[0]
    assert sampled == [(0, 0, "0.wav"), (0, 2, "2.wav")]  # the skipped batch writes no sample
    stub = _Stub(1, RuntimeError("HIP error: an illegal memory access was encountered"))
    with pytest.raises(RuntimeError, match="illegal memory access"):
        V.run_batches(stub.validate, batches, sample_count=0, force_samples=[], log=lines.append)
    assert stub.seen == [0, 1]  # nothing runs behind it


def _raised_by_check(rc):
    """what stylish_tts_amd.lib.check raises for the library status `rc` -- the path every error of the library takes to Python"""
    import __graft_entry__ as ge
    ge.build()
    from stylish_tts_amd import lib as L
    L.load()
    with pytest.raises(L.StyError) as info:
        L.check(rc)
    return info.value


def test_a_device_error_of_the_library_is_never_skipped():
    """The library reports a HIP runtime error (STY_EHIP = -3: a failed launch, a sticky fault) through the same lib.check that
    reports its refusals, as a StyError.  The pass must tell them apart: the refusal statuses are skipped, STY_EHIP ends the
    pass with the next batch never started -- in the batch loop and in the duration stage's per-sample handling alike."""
    from stylish_tts_amd import lib as L
    from stylish_tts_amd import validation as V
    hip = _raised_by_check(-3)
    assert isinstance(hip, L.StyDeviceError) and isinstance(hip, L.StyError) and hip.status == -3 and not L.refused_on_host(hip)
    for rc in (-1, -2, -4, -5):
        e = _raised_by_check(rc)
        assert not isinstance(e, L.StyDeviceError) and e.status == rc and L.refused_on_host(e)
    assert L.refused_on_host(L.StyError("a Python-side shape check")) and not L.refused_on_host(RuntimeError("x"))
    batches = [([f"{i}.wav"], i) for i in range(3)]
    lines = []
    stub = _Stub(1, hip)
    with pytest.raises(L.StyDeviceError):
        V.run_batches(stub.validate, batches, sample_count=3, force_samples=[], log=lines.append)
    assert stub.seen == [0, 1] and not lines  # batch 2 is never seen, and nothing was logged as "skipped"
    stub = _Stub(1, _raised_by_check(-1))  # ... while a refusal of the library is skipped as a Python-side one is
    logs, skipped = V.run_batches(stub.validate, batches, sample_count=0, force_samples=[], log=lines.append)
    assert stub.seen == [0, 1, 2] and skipped == [1] and len(logs) == 2 and "batch 1 skipped" in lines[0]
    # the duration stage's samples: a refusal comes back as a value, a device error does not
    def fail(e):
        raise e
    refusal = _raised_by_check(-1)
    assert V.or_refusal(lambda: 7) == 7 and V.or_refusal(lambda: fail(refusal)) is refusal
    with pytest.raises(L.StyDeviceError):
        V.or_refusal(lambda: fail(hip))
    with pytest.raises(ZeroDivisionError):
        V.or_refusal(lambda: 1 // 0)
    import inspect
    from stylish_tts_amd import duration
    src = inspect.getsource(duration.DurationTrainer.validate)
    assert "or_refusal(" in src and "except" not in src  # the per-sample handling is that helper and nothing else


def test_record_is_strict_json_when_every_batch_was_skipped():
    from stylish_tts_amd import validation as V
    assert V.finite_or_none(float("inf")) is None and V.finite_or_none(float("nan")) is None and V.finite_or_none(2.5) == 2.5
    line = V.record_line({"total": V.finite_or_none(float("inf")), "metrics": {"mel": V.finite_or_none(float("nan"))}})
    assert "Infinity" not in line and "NaN" not in line and json.loads(line) == {"total": None, "metrics": {"mel": None}}
    with pytest.raises(ValueError):
        V.record_line({"total": float("inf")})


def test_missing_val_list_is_refused_before_a_device_is_touched(tmp_path):
    from stylish_tts_amd import validation as V
    from stylish_tts_amd.lib import StyError
    ds = types.SimpleNamespace(path=str(tmp_path), val_data="validation-list.txt", wav_path="wav-dir",
                               pitch_path="pitch.safetensors", alignment_path="alignment.safetensors")
    cfg = types.SimpleNamespace(dataset=ds)
    was = torch.cuda.is_initialized()
    with pytest.raises(StyError, match="val_data not found"):
        V.ValidationPass(cfg, types.SimpleNamespace(), "acoustic", str(tmp_path / "out"), lambda k: 2, "cuda:0")
    (tmp_path / "validation-list.txt").write_text("\n\n")
    with pytest.raises(StyError, match="lists no utterance"):
        V.ValidationPass(cfg, types.SimpleNamespace(), "acoustic", str(tmp_path / "out"), lambda k: 2, "cuda:0")
    assert torch.cuda.is_initialized() == was and not (tmp_path / "out").exists()


def test_wav_writer_saturates_pcm16(tmp_path):
    import wave
    import numpy as np
    from stylish_tts_amd import validation as V
    p = str(tmp_path / "eval" / "step_3" / "sample_0.wav")
    V.write_wav(p, np.array([0.0, 0.5, -0.5, 1.5, -2.0], dtype=np.float32), 24000)
    with wave.open(p, "rb") as f:
        assert (f.getframerate(), f.getsampwidth(), f.getnchannels()) == (24000, 2, 1)
        x = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    assert x.tolist() == [0, 16384, -16384, 32767, -32768]


def test_validate_small_fixture_frame_totals_are_the_rounded_duration_sums():
    from safetensors.torch import load_file
    G = os.path.join(ROOT, "tests", "golden")
    fx = load_file(os.path.join(G, "validate_small.safetensors"))
    stage = load_file(os.path.join(G, "stages_small.safetensors"))
    dur, frames = fx["duration"], fx["frames"]
    assert dur.shape == stage["duration.pred_duration"].shape and frames.shape == (dur.shape[0],)
    assert torch.allclose(dur, stage["duration.pred_duration"], rtol=1e-6, atol=1e-6)  # the same eval-mode forward
    for i in range(dur.shape[0]):
        total = float(dur[i].double().sum())
        assert int(frames[i]) == int(round(total)) and abs(total - math.floor(total) - 0.5) >= 1e-3, (i, total)
        n = int(fx[f"audio_len.{i}"])
        assert n == 300 * int(frames[i]) and fx[f"prior.{i}"].shape == (1, n)
        assert 0 < fx[f"audio_sub.{i}"].numel() <= 16384 and float(fx[f"audio_norm.{i}"]) > 0
    for k in ("duration", "duration_ce"):
        assert abs(float(fx["log." + k]) - float(stage["duration.log." + k])) <= 1e-6 * float(stage["duration.log." + k])
    assert os.path.getsize(os.path.join(G, "validate_small.safetensors")) < os.path.getsize(os.path.join(G, "stages_small.safetensors")) // 2
    json.dumps({"frames": frames.tolist()})
