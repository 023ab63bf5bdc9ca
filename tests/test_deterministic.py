"""The deterministic mode's switch, without a device: the C ABI pair, the Python binding, the environment variable, the
`--deterministic` flags of the two training commands, and the workspace figures of the entry points that size without a model.

The `sty_*_train_workspace_bytes` entry points need a finalized model, which lives on the device: their figures are checked in
tests/test_deterministic_gpu.py.  What sizes without one -- the acoustic losses and the three discriminator families -- is here.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def L():
    from stylish_tts_amd import lib
    lib.load()
    try:
        yield lib
    finally:
        lib.set_deterministic(False)


def test_header_declares_the_switch_and_the_library_exports_it(L):
    text = open(os.path.join(ROOT, "include", "stylish_hip.h")).read()
    assert re.search(r"\bint\s+sty_set_deterministic\s*\(\s*int\s+on\s*\)\s*;", text)
    assert re.search(r"\bint\s+sty_get_deterministic\s*\(\s*void\s*\)\s*;", text)
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "sty_set_deterministic") and hasattr(raw, "sty_get_deterministic")
    assert "sty_set_deterministic" in L.SYMBOLS and "sty_get_deterministic" in L.SYMBOLS


def test_set_and_get_round_trip_without_a_device(L):
    lib = L.load()
    assert lib.sty_get_deterministic() == 0 and L.get_deterministic() is False  # the default
    assert lib.sty_set_deterministic(1) == 0
    assert lib.sty_get_deterministic() == 1 and L.get_deterministic() is True
    assert lib.sty_set_deterministic(7) == 0 and lib.sty_get_deterministic() == 1  # any non-zero value is "on"
    L.set_deterministic(False)
    assert lib.sty_get_deterministic() == 0 and L.get_deterministic() is False
    L.set_deterministic(True)
    assert lib.sty_get_deterministic() == 1


@pytest.mark.parametrize("value,want", [("1", "True"), ("0", "False"), (None, "False")])
def test_environment_variable_turns_the_mode_on_at_load(value, want):
    env = {k: v for k, v in os.environ.items() if k != "STY_DETERMINISTIC"}
    if value is not None:
        env["STY_DETERMINISTIC"] = value
    r = subprocess.run([sys.executable, "-c", "from stylish_tts_amd import lib as L; L.load(); print(L.get_deterministic())"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == want


def test_training_commands_accept_the_flag_and_pass_it_through(L, monkeypatch):
    from stylish_tts_amd import train as T
    from stylish_tts_amd import train_align as TA
    seen = {}
    monkeypatch.setattr(T, "train", lambda *a, **kw: seen.setdefault("train", kw))
    monkeypatch.setattr(TA, "train_align", lambda *a, **kw: seen.setdefault("train_align", kw))
    T.main(["cfg.yml", "--out", "o", "--deterministic"])
    TA.main(["cfg.yml", "--out", "o", "--deterministic"])
    assert seen["train"]["deterministic"] is True and seen["train_align"]["deterministic"] is True
    seen.clear()
    T.main(["cfg.yml", "--out", "o"])
    TA.main(["cfg.yml", "--out", "o"])
    assert seen["train"]["deterministic"] is False and seen["train_align"]["deterministic"] is False


def test_train_functions_hand_the_flag_to_the_stage_and_set_the_switch_first(L, monkeypatch):
    """train / train_align forward the keyword to train_model / train_align_model; those set the switch before anything else
    (observed here at the first refusal, long before a device is needed); TrainContext hands it to every stage's trainer."""
    import inspect
    from stylish_tts_amd import train as T
    from stylish_tts_amd import train_align as TA
    for fn in (T.train_model, TA.train_align_model, T.TrainContext.__init__):
        assert inspect.signature(fn).parameters["deterministic"].default is False
    for mod in ("acoustic.AcousticTrainer", "textual.TextualTrainer", "duration.DurationTrainer", "alignment.AlignmentTrainer"):
        m, cls = mod.split(".")
        klass = getattr(__import__("stylish_tts_amd." + m, fromlist=[cls]), cls)
        assert inspect.signature(klass.__init__).parameters["deterministic"].default is False
    for run in (lambda: T.train_model(None, None, "o", "acoustic", deterministic=True),
                lambda: TA.train_align_model(None, None, "o", deterministic=True)):
        L.set_deterministic(False)
        with pytest.raises(Exception):  # no config: refused on the host
            run()
        assert L.get_deterministic() is True
    L.set_deterministic(False)
    with pytest.raises(Exception):
        T.train_model(None, None, "o", "acoustic")
    assert L.get_deterministic() is False  # the default leaves the switch alone
    # the context hands the flag to the trainer's constructor
    ctx = T.TrainContext.__new__(T.TrainContext)
    ctx.deterministic, ctx.rank, ctx.compute, ctx.adversarial = True, 0, "fp32", False

    class W(dict):
        __getattr__ = dict.__getitem__

    ctx.config = W(loss_weight=W(mel=5.0, multi_phase=8.0, generator=1.0))
    ctx.normalization = W(mel_log_mean=-4.0, mel_log_std=4.0)
    ctx.model_config = W(text_encoder=W(dropout=0.2))
    ctx.model = lambda key: key
    got = {}
    from stylish_tts_amd import acoustic
    monkeypatch.setattr(acoustic, "AcousticTrainer", lambda *a, **kw: got.update(kw))
    ctx.make_trainer("acoustic", 1e-4)
    assert got["deterministic"] is True


SIZERS = {
    "acoustic_loss": lambda lib, n: lib.sty_acoustic_loss_workspace_bytes(5, 24000, n),
    "acoustic_gan": lambda lib, n: lib.sty_acoustic_gan_workspace_bytes(5, 24000, 1, n),
    "specdisc": lambda lib, n: lib.sty_specdisc_workspace_bytes(5, 257, 188, 1, n),
    "pitchdisc_k21": lambda lib, n: lib.sty_pitchdisc_workspace_bytes(5, 2, 21, 80, 1, n),
    "pitchdisc_k5": lambda lib, n: lib.sty_pitchdisc_workspace_bytes(5, 1, 5, 24, 1, n),
    "cfdisc": lambda lib, n: lib.sty_cfdisc_workspace_bytes(5, 24000, 1, n),
}


@pytest.mark.parametrize("name", sorted(SIZERS))
def test_workspace_figures_follow_the_mode(L, name):
    """the figure of mode 1 holds the partial slots (every entry here has an order-dependent sum, so it is strictly larger),
    and the figure of mode 0 is the same before and after a visit to mode 1"""
    lib = L.load()

    def size():
        n = C.c_size_t()
        L.check(SIZERS[name](lib, C.byref(n)))
        return n.value

    L.set_deterministic(False)
    before = size()
    L.set_deterministic(True)
    det = size()
    L.set_deterministic(False)
    after = size()
    print(f"\n  {name}: {before} bytes, deterministic mode {det} (+{det - before})")
    assert before == after
    assert det > before
