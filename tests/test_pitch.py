"""The pitch command without a device: the RMVPE shell's state_dict layout, the host tables of the front end against the
float64 restatements of tests/pitch_cases.py, sanity of those restatements, the decode restatement against the reference
function's recorded outputs (tools/gen_pitch_golden.py), and everything the path refuses before it needs a GPU."""
import ctypes as C
import json
import math
import os

import pytest
import torch
from safetensors.torch import load_file

from tests import pitch_cases as PC

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from stylish_tts_amd import lib as L
    return L.load()


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(G, "pitch_small.safetensors")), json.load(open(os.path.join(G, "pitch_small.json")))


# ---- 1. the module shell -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "full"])
def test_shell_has_the_reference_state_dict_layout(name):
    import stylish_tts_amd as S
    ref = json.load(open(os.path.join(G, "manifest_rmvpe.json")))[name]
    cfg = PC.SMALL if name == "small" else PC.FULL
    m = S.RMVPE(**cfg)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref
    assert list(m.state_dict()) == list(ref), "key order"
    if name == "full":
        assert len(ref) == 741 and m.state_dict().keys() == S.RMVPE().state_dict().keys()  # E2E0(4, 1, (2, 2)) is the default
    # a reference-layout dict loads with strict=True, and from_state_dict reads the configuration off it
    state = {k: torch.zeros(shape, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32)
             for k, shape in ref.items()}
    m.load_state_dict(state, strict=True)
    back = S.RMVPE.from_state_dict(state)
    assert (back.n_blocks, back.inter_layers, back.en_out_channels) == tuple(cfg[k] for k in ("n_blocks", "inter_layers",
                                                                                              "en_out_channels"))


def test_fill_covers_the_gru_keys_and_is_keyed():
    from stylish_tts_amd.synthetic_weights import fill_tensor
    w = fill_tensor("fc.0.gru.weight_hh_l0_reverse", (768, 256), PC.SEED)
    b = fill_tensor("fc.0.gru.bias_ih_l0", (768,), PC.SEED)
    assert w.shape == (768, 256) and abs(w.std().item() * 16 - 1) < 0.05
    assert b.shape == (768,) and abs(b.std().item() * 10 - 1) < 0.15
    assert not torch.equal(w, fill_tensor("fc.0.gru.weight_hh_l0", (768, 256), PC.SEED))
    P = PC.rmvpe_weights(PC.SMALL)
    assert set(P) == set(json.load(open(os.path.join(G, "manifest_rmvpe.json")))["small"])


# ---- 2. the host tables --------------------------------------------------------------------------------------------------
def test_host_tables_are_the_restated_closed_forms(lib):
    """to 2 ulp of fp32 relative to the table's largest entry (the tolerance of test_default_stft_bases_are_the_reference_buffers)"""
    out = (C.c_float * (2 * PC.TAPS))()
    lib.sty_rmvpe_resample_kernel_host(out)
    got = torch.tensor(list(out), dtype=torch.float32).view(2, PC.TAPS)
    ref = PC.resample_kernel()
    assert (got.double() - ref).abs().max().item() <= 2.4e-7 * ref.abs().max().item()
    out = (C.c_float * (PC.N_MELS * 513))()
    lib.sty_rmvpe_mel_basis_host(out)
    got = torch.tensor(list(out), dtype=torch.float32).view(PC.N_MELS, 513)
    ref = PC.mel_basis()
    assert (got.double() - ref).abs().max().item() <= 2.4e-7 * ref.abs().max().item()
    assert bool((got.sum(1) > 0).all()), "no mel row is empty"


# ---- 3. sanity of the restatement itself ---------------------------------------------------------------------------------
def test_resampler_restatement_is_a_resampler():
    k = PC.resample_kernel()
    assert k.shape == (2, PC.TAPS) and (k.sum(1) - 1).abs().max().item() <= 1e-6
    N = 18000
    t24 = torch.arange(N, dtype=torch.float64) / 24000.0
    y = PC.resample(torch.sin(2 * math.pi * 1000.0 * t24)[None])
    assert y.shape == (1, 12000)
    t16 = torch.arange(12000, dtype=torch.float64) / 16000.0
    err = (y[0] - torch.sin(2 * math.pi * 1000.0 * t16))[400:-400].abs().max().item()
    print(f"\n  1 kHz sine through the restated resampler, interior: {err:.2e}")
    assert err <= 2e-3
    assert PC.resample(torch.zeros(2, 18001)).shape == (2, 12001)  # ceil(2 N / 3)


def test_stft_half_of_the_restatement_is_torch_stft():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 12000, generator=g, dtype=torch.float64)
    ref = torch.stft(x, n_fft=1024, hop_length=200, win_length=1024, window=torch.hann_window(1024, dtype=torch.float64),
                     center=True, return_complex=True).abs()
    got = PC.stft_mag(x)
    assert got.shape == ref.shape == (2, 513, 61)
    assert (got - ref).abs().max().item() <= 1e-10 * ref.abs().max().item()


def test_mel_basis_restatement_shape_and_rows():
    fb = PC.mel_basis()
    assert fb.shape == (128, 513) and bool((fb >= 0).all())
    assert bool((fb.sum(1) > 0).all()), "no mel row is empty"
    assert fb[:, 0].abs().max().item() == 0.0 and fb[:, 512].abs().max().item() <= 1e-12  # 0 Hz and 8000 Hz carry no weight
    x = PC.harmonic_audio(18000)
    lm = PC.logmel(x)
    assert lm.shape == (2, 128, 61)
    assert bool((lm[:, :, 0] == math.log(1e-5)).all()), "the leading zeros are silence"


# ---- 4. decode -----------------------------------------------------------------------------------------------------------
def test_decode_restatement_against_the_reference_function(gold):
    fx, meta = gold
    names = meta["decode_cases"]
    cases = PC.decode_cases()
    assert list(cases) == names and torch.equal(torch.stack(list(cases.values())), fx["decode.rows"])
    rows, ref32, ref64 = fx["decode.rows"], fx["decode.f0_f32"].double(), fx["decode.f0_f64"]
    got = PC.decode(rows)
    gated = [i for i, k in enumerate(names) if k != "at_threshold"]
    gate, scale, own = PC.forward_gate(ref64[gated], ref32[gated])
    err = (got[gated] - ref64[gated]).abs().max().item()
    print(f"\n  decode restatement: max|ref| {scale:.3f}  reference fp32-to-f64 {own:.3e}  restatement-to-f64 {err:.3e}  gate {gate:.3e}")
    assert err <= gate
    f0_of = lambda k: 10.0 * 2.0 ** ((20.0 * k + PC.CONST) / 1200.0)
    for k in (4, 100, 355):  # a symmetric bump: exactly the bin's own frequency
        assert got[names.index(f"onehot_{k}")].item() == f0_of(k)
        wide = got[names.index(f"bump_{k}")].item()
        assert abs(wide - f0_of(k)) <= 4e-16 * f0_of(k) * 8 and torch.tensor(wide).float() == torch.tensor(f0_of(k)).float()
    for k in (0, 1, 2, 3, 356, 357, 358, 359):  # clipped window: the missing side pulls the average inwards
        v = got[names.index(f"edge_{k}")].item()
        assert (v > f0_of(k)) if k < 4 else (v < f0_of(k)), k
    # an exact tie: the lowest index wins (its window holds bin 121 = 0.3; the other's would hold bin 199 = 0.4)
    row = cases["tie"].double()
    lo = (row[116:125] * (20.0 * torch.arange(116, 125).double() + PC.CONST)).sum() / row[116:125].sum()
    assert got[names.index("tie")].item() == pytest.approx(10.0 * 2.0 ** (lo.item() / 1200.0), rel=1e-14)
    assert got[names.index("quiet")].item() == 0.0 and ref64[names.index("quiet")].item() == 0.0
    # a maximum equal to the fp32 threshold is voiced, as in the reference's fp32 run (the comparison is `< thred`, in fp32)
    i = names.index("at_threshold")
    assert ref32[i].item() > 0 and got[i].item() == pytest.approx(ref32[i].item(), rel=1e-6)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(lib, tmp_path):
    import stylish_tts_amd as S
    from stylish_tts_amd import lib as L
    from stylish_tts_amd import pitch as P
    with pytest.raises(NotImplementedError, match="pyworld"):
        P.pitch("no_config.yml", "", 8, "pyworld", rmvpe_path="x.safetensors")
    with pytest.raises(NotImplementedError, match="pyworld"):
        P.main(["no_config.yml", "--method", "pyworld", "--rmvpe", "x.safetensors"])
    with pytest.raises(S.StyError, match="--rmvpe is required"):
        P.pitch("no_config.yml", "")
    with pytest.raises(S.StyError, match="--rmvpe is required"):
        P.main(["no_config.yml", "-k", "4", "-bs", "2"])
    with pytest.raises(NotImplementedError):
        S.RMVPE.decode(torch.zeros(1, 1, 360), use_viterbi=True)
    # the library: n < 17 is a shape error ahead of everything else; compute_bf16 and training are refused for the kind
    h = C.c_void_p()
    assert lib.sty_model_create(b"rmvpe", C.byref(h)) == 0
    need = C.c_size_t()
    assert lib.sty_rmvpe_workspace_bytes(h, 2, 16, C.byref(need)) == -2 and b"at least 17" in lib.sty_last_error()
    assert lib.sty_rmvpe_fwd(h, 2, 16, None, None, None, 0, None) == -2
    assert lib.sty_rmvpe_workspace_bytes(h, 2, 17, C.byref(need)) == -5  # not finalized: STY_ESTATE, never a fallback
    opts = L.TrainOpts(0, 0, 0, 0, 0.1, 0, 0.2, 1, 0, 0.2)
    assert lib.sty_model_set_train_opts(h, C.byref(opts)) == -1 and b"fp32 operands" in lib.sty_last_error()
    assert lib.sty_model_enable_training(h) == -1 and b"inference-only" in lib.sty_last_error()
    lib.sty_model_destroy(h)
    m = S.RMVPE(**PC.SMALL)
    with pytest.raises(S.StyError, match="compute_bf16 is refused"):
        m.set_train_opts(compute_bf16=True)
    with pytest.raises(S.StyError, match="inference only"):
        m.enable_training()
    with pytest.raises(S.StyError, match="at least 17"):
        with torch.no_grad():
            m.mel2hidden(torch.zeros(1, 128, 16))
    with pytest.raises(S.StyError):  # no CPU path
        with torch.no_grad():
            m.mel2hidden(torch.zeros(1, 128, 32))
    assert lib.sty_rmvpe_mel_workspace_bytes(1, 600, C.byref(need)) == -1  # 400 samples at 16 kHz cannot be reflected by 512
    assert lib.sty_rmvpe_decode(0, 4, None, 0.03, None, None) == -1
