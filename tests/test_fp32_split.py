"""The fp32 split mode (bf16x3) at the C-ABI boundary and in the `speak` command's argument layer: who may switch it on, that
it and the bf16 compute mode refuse each other, what the conv dispatch answers for compute mode 4.  Host only (no GPU)."""
import ctypes as C

import pytest

STY_OK, STY_EINVAL = 0, -1
STY_CONV_32P = 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from stylish_tts_amd import lib as L
    return L.load()


def _model(lib, kind):
    h = C.c_void_p()
    assert lib.sty_model_create(kind.encode(), C.byref(h)) == STY_OK
    return h


def _opts(compute_bf16):
    from stylish_tts_amd import lib as L
    return L.TrainOpts(0, 0, 0, 0, 0.1, 0, 0.2, int(compute_bf16), 0, 0.2)


def test_split_then_bf16_is_refused(lib):
    h = _model(lib, "speech_predictor")
    try:
        assert lib.sty_model_set_fp32_split(h, 1) == STY_OK
        assert lib.sty_model_set_train_opts(h, C.byref(_opts(1))) == STY_EINVAL
        assert b"split" in lib.sty_last_error()
        assert lib.sty_model_set_train_opts(h, C.byref(_opts(0))) == STY_OK  # every other option stays settable
        assert lib.sty_model_set_fp32_split(h, 0) == STY_OK
        assert lib.sty_model_set_train_opts(h, C.byref(_opts(1))) == STY_OK  # ... and bf16 again once the split is off
    finally:
        lib.sty_model_destroy(h)


def test_bf16_then_split_is_refused(lib):
    h = _model(lib, "speech_predictor")
    try:
        assert lib.sty_model_set_train_opts(h, C.byref(_opts(1))) == STY_OK
        assert lib.sty_model_set_fp32_split(h, 1) == STY_EINVAL
        assert b"bf16" in lib.sty_last_error()
        assert lib.sty_model_set_fp32_split(h, 0) == STY_OK  # switching it off is never in conflict
    finally:
        lib.sty_model_destroy(h)


@pytest.mark.parametrize("kind", ["text_aligner", "vocoder", "mel_style_encoder"])
def test_other_kinds_are_refused_by_name(lib, kind):
    h = _model(lib, kind)
    try:
        assert lib.sty_model_set_fp32_split(h, 1) == STY_EINVAL
        assert kind.encode() in lib.sty_last_error()
    finally:
        lib.sty_model_destroy(h)


def _route(lib, B, Ci, Co, K, d, T, mode, flags=0):
    k = C.c_int(-2)
    assert lib.sty_conv1d_route(B, Ci, Co, K, d, T, mode, flags, C.byref(k)) == STY_OK
    return k.value


def test_route_of_an_eligible_conv_in_mode_4(lib, monkeypatch):
    monkeypatch.delenv("STY_CONV32P_MIN_TILES", raising=False)
    monkeypatch.delenv("STY_NO_CONV32P", raising=False)
    assert _route(lib, 8, 32, 32, 11, 1, 60000, 4) == STY_CONV_32P


@pytest.mark.parametrize("shape", [(2, 64, 64, 3, 1, 500), (2, 32, 32, 11, 1, 100), (8, 32, 64, 11, 1, 60000), (8, 33, 32, 11, 1, 60000)])
def test_mode_4_answers_what_mode_0_answers_elsewhere(lib, shape, monkeypatch):
    monkeypatch.delenv("STY_CONV32P_MIN_TILES", raising=False)
    monkeypatch.delenv("STY_NO_CONV32P", raising=False)
    for flags in (0, 2):  # plain, with a residual
        assert _route(lib, *shape, 4, flags) == _route(lib, *shape, 0, flags)
    assert _route(lib, *shape, 4) != STY_CONV_32P


def test_unit_workspace_covers_the_fragment_triples(lib):
    """K x 6 KB of bf16 A-fragment triples behind the packed weight of a conv with one 32-channel chunk each way"""
    a, b = C.c_size_t(), C.c_size_t()
    assert lib.sty_conv1d_workspace_bytes(32, 32, 11, C.byref(a)) == STY_OK
    packed = (11 * 32 * 128 + 128) * 4 + 512
    assert a.value >= packed + 11 * 2 * 3 * 64 * 16
    assert lib.sty_conv1d_workspace_bytes(64, 64, 3, C.byref(b)) == STY_OK
    assert b.value == (3 * 64 * 128 + 128) * 4 + 512  # (no triples: the split mode does not take the shape)


def test_speak_parses_the_compute_mode(monkeypatch, capsys):
    """the argparse layer alone: Speaker and speak_document are stand-ins, no device is touched"""
    from stylish_tts_amd import speak as SP
    seen = {}

    class FakeSpeaker:
        def __init__(self, checkpoint, model_config_path, voicepack_path, device=None, compute="fp32"):
            seen.update(checkpoint=checkpoint, compute=compute)

    monkeypatch.setattr(SP, "Speaker", FakeSpeaker)
    monkeypatch.setattr(SP, "speak_document", lambda infile, outfile, speaker, **kw: seen.update(outfile=outfile))
    SP.main(["ckpt", "pack", "in.txt", "out.wav", "--compute", "bf16x3"])
    assert seen == dict(checkpoint="ckpt", compute="bf16x3", outfile="out.wav")
    assert "compute mode bf16x3" in capsys.readouterr().out  # the start-up log line names the mode
    SP.main(["ckpt", "pack", "in.txt", "out.wav"])
    assert seen["compute"] == "fp32"
    with pytest.raises(SystemExit):
        SP.main(["ckpt", "pack", "in.txt", "out.wav", "--compute", "fp16"])
    assert SP.COMPUTE_MODES == ("fp32", "bf16", "bf16x3")


def test_module_shell_carries_the_switch():
    import stylish_tts_amd as S
    sp = S.SpeechPredictor()
    assert sp.set_fp32_split() is sp and sp._fp32_split is True
    assert sp.set_fp32_split(False)._fp32_split is False
    with pytest.raises(S.StyError, match="vocoder"):
        S.MultiGenerator().set_fp32_split()
