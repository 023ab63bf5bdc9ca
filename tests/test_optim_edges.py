"""The optimizer side (csrc/optim.hip) at the sizes, regimes and branches where it can go wrong, against float64.

Every training step of every stage ends in adamw_kernel, and in the GAN steps the discriminators' learning rate never leaves the
device: disc_lr_track_kernel keeps the running mean of the tracked loss and the multiplier it sets, adamw_kernel forms its two
rate-dependent scalars from that device double.  tests/test_hip_parity.py runs the kernel on five small tensors with one set of
hyper-parameters and the tracker once, from the state in which the multiplier is exactly 1.  Here (tests/optim_cases.py): bucket
sizes on every edge of launch_adamw (tail-only launches, one and two workgroups, the grid cap and the second trip of the
grid-stride loop), the eps regime, gradients over twelve decades, grad_scale, step counts up to 1e6, the scaled entry point at five
multipliers, all four branches of the tracker on and beside their thresholds, a 200-step sequence through the helper, and the
multiplier arriving in a trainer's parameters.  tests/test_optim_oracle.py pins on the CPU what the gates here assume: they are
twice the distance of float32 torch.optim.AdamW from float64 torch.optim.AdamW, and every restated mistake lands 10 x outside one.

The library is called through ctypes on plain device tensors, so n, step, m and v are set directly.  Runs on the GPU box only (`-m gpu`).
"""
import ctypes as C
import functools
import math
import os

import pytest
import torch

from tests.optim_cases import (ADAMW_REGIME_CASES, ADAMW_SCALED_CASES, ADAMW_SCALED_MULTS as MULTS, ADAMW_SIZE_NAMES, DISC_LR_POINTS, DISC_LR_SEQUENCE, DISC_LR_SUB_COUNTS,
                               adamw_cases, contract_case, disc_lr_fixture, helper_constants, oracle64, restated_multiplier, restated_sequence)
from tests.test_optim_oracle import gate_of, scaled_gates
from tests.test_ragged_lengths import Report

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, SENTINEL = 64, -12345.0  # floats behind every buffer, and what they hold
POW_TOL = 1e-13  # the pow branches, relative: device pow in double is good to a few ulp (2.2e-16 each); two orders of margin


def _lib():
    from stylish_tts_amd import lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _buf(t):
    """a device copy of the float32 vector t with GUARD sentinels behind it"""
    b = torch.full((t.numel() + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    b[:t.numel()].copy_(t)
    assert b.data_ptr() % 16 == 0
    return b


def run_hip(case, mult=None, lr=None):
    """the case's steps through sty_adamw_step (mult None; `lr` replaces the case's rate) or sty_adamw_step_scaled(lr_d = the case's
    rate, *mult) -> (p, m, v) [n] on the CPU.  Only the n elements are returned; the guards behind p, g, m, v must be untouched."""
    L, lib = _lib()
    hp, n = case["hp"], case["n"]
    p, m, v = _buf(case["p0"]), _buf(case["m0"]), _buf(case["v0"])
    mult_d = None if mult is None else torch.tensor([mult], dtype=torch.float64, device=DEV)
    for i, grad in enumerate(case["grads"]):
        g = _buf(grad)
        tail = (hp["betas"][0], hp["betas"][1], hp["eps"], hp["wd"], case["step0"] + i, case["grad_scale"], _stream())
        if mult is None:
            L.check(lib.sty_adamw_step(n, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), hp["lr"] if lr is None else lr, *tail))
        else:
            L.check(lib.sty_adamw_step_scaled(n, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), hp["lr"], L.ptr(mult_d), *tail))
        torch.cuda.synchronize()
        assert bool((g[n:] == SENTINEL).all()) and torch.equal(g[:n].cpu(), grad), "the gradient buffer was written"
    for name, b in (("p", p), ("m", m), ("v", v)):
        assert bool((b[n:] == SENTINEL).all()), f"{name}: written behind element n = {n}"
    return p[:n].cpu(), m[:n].cpu(), v[:n].cpu()


def _table(rep, case, got, ref, gates, tag=""):
    """p of the movement, m and v of their maxima (optim_cases.distances), as rows of the per-tensor table"""
    p0 = case["p0"].double()
    rows = (("p (of max |p_after - p_before|)", got[0].double() - p0, ref[0] - p0), ("m (of max |m|)", got[1].double(), ref[1]),
            ("v (of max |v|)", got[2].double(), ref[2]))
    for (label, a, b), gate in zip(rows, gates):
        norm = b.abs().max().item()
        assert norm > 0
        rep.add(f"{tag}{label}", a / norm, b / norm, gate)


@pytest.mark.parametrize("name", ADAMW_SIZE_NAMES + ADAMW_REGIME_CASES)
def test_adamw_vs_float64_torch(name):
    """(a) sty_adamw_step over the bucket sizes and the regimes against torch.optim.AdamW in float64, at twice the distance of
    torch.optim.AdamW in float32 (test_optim_oracle.GATES).  Elements whose gradient and moments are exact zeros move by weight
    decay alone, and nothing is written behind element n.

    Measured on an MI355X with 1 - beta formed in fp32 from fp32 betas, as the entry points took them before this test: v 6.7e-7 ...
    1.04e-6 in every case against gates of 2e-7 and 3e-7 (1.0f - 0.99f is 0.00999999046, 9.5e-7 off 0.01), m up to 2.3e-7, over its
    gate at d-wide and f-step2 (1.0f - 0.85f is 1.6e-7 off 0.15).  The betas now cross the C ABI as doubles and 1 - beta is formed in double, as
    torch forms it: the figures of profiles/optim_edges_table.txt."""
    case = adamw_cases()[name]
    ref = oracle64(name)
    got = run_hip(case)
    assert all(torch.isfinite(t).all() for t in got)
    rep = Report()
    _table(rep, case, got, ref, gate_of(name))
    print(f"\n  {name}: n = {case['n']}, steps {case['step0']} .. {case['step0'] + len(case['grads']) - 1}")
    rep.done()
    still = (case["grads"] == 0).all(0) & (case["m0"] == 0) & (case["v0"] == 0)
    if name == "c-eps":
        assert int(still.sum()) >= case["n"] // 3
    if bool(still.any()):
        # m / (sqrt(0) / bc2s + eps) = 0 / eps = 0: p is multiplied by fp32(1 - lr wd) once a step and nothing else
        hp = case["hp"]
        decay = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(hp["lr"], dtype=torch.float32) * torch.tensor(hp["wd"], dtype=torch.float32)
        want = case["p0"][still].clone()
        for _ in case["grads"]:
            want = want * decay
        assert torch.equal(got[0][still], want) and not bool(got[1][still].any()) and not bool(got[2][still].any())


@pytest.mark.parametrize("mult", MULTS, ids=[f"x{m:.3g}" for m in MULTS])
@pytest.mark.parametrize("name", ADAMW_SCALED_CASES)
def test_adamw_scaled_vs_float64_torch_at_the_scaled_rate(name, mult):
    """(b) sty_adamw_step_scaled(lr_d, *mult): the lr_mult branch of adamw_kernel with the multiplier in device memory, against
    torch.optim.AdamW in float64 at lr_d * mult.  m and v at the gates of (a); p at twice float32 torch's distance at the same
    rate (test_optim_oracle.GATE_SCALED_P: the gate of (a) at multiplier 1, tighter above it; below it float32 torch itself is
    outside the gate of (a), because the movement shrinks with the rate and the rounding of p does not)."""
    case = adamw_cases()[name]
    ref = oracle64(name, case["hp"]["lr"] * mult)
    got = run_hip(case, mult=mult)
    rep = Report()
    _table(rep, case, got, ref, scaled_gates(name, mult))
    print(f"\n  {name} x {mult!r}")
    rep.done()


def _bits(t):
    return t.contiguous().view(torch.int32)


BIT_CASES = [("b-decay", m) for m in MULTS] + [contract_case()]


@pytest.mark.parametrize("name,mult", BIT_CASES, ids=[f"{n}-x{m:.3g}" for n, m in BIT_CASES])
def test_scaled_entry_equals_the_plain_entry_at_the_rounded_rate(name, mult):
    """(c) What the comment above adamw_kernel claims: decay and step_size formed on the device from lr_d * *lr_mult are the host
    path's.  sty_adamw_step_scaled(lr_d, mult) and sty_adamw_step(lr = float32(lr_d * mult)) leave p, m and v bit-identical, on
    regime (b), where lr * wd is far above one ulp of 1 (1e-3 x mult against 6e-8).

    At regime (b) itself this cannot fail for a reason worth knowing: fp32(1 - lr wd) is the same whether lr wd is rounded first
    (host code) or not (the FMA device code contracts `1.0f - lr * wd` into) at all five multipliers -- the two differ at about one
    (lr, wd) pair in a thousand.  b-contract is regime (b) at the nearest weight decay above 0.1 where they do differ
    (optim_cases.contract_case, multiplier 4): there the kernel as it was left 968 of 1029 parameters with other bits than the plain
    entry (2.9e-7 of max |p| after six steps) while passing the five cases above; it forms the product and the difference apart now."""
    case = adamw_cases()[name]
    lr32 = torch.tensor(case["hp"]["lr"] * mult, dtype=torch.float64).float().item()
    scaled = run_hip(case, mult=mult)
    plain = run_hip(case, lr=lr32)
    diff = [int((_bits(a) != _bits(b)).sum()) for a, b in zip(scaled, plain)]
    worst = (scaled[0].double() - plain[0].double()).abs().max().item() / plain[0].abs().max().item()
    print(f"\n  {name} x {mult!r}: elements whose bits differ (p, m, v) {diff} of {case['n']}, largest |p - p| of max |p| {worst:.3e}")
    assert diff == [0, 0, 0]


@pytest.mark.parametrize("sub_count", DISC_LR_SUB_COUNTS)
def test_disc_lr_track_branch_by_branch(sub_count):
    """(d) sty_disc_lr_track with state[0] preloaded and no loss: state[1] is the multiplier the reference's helper returned for
    that last_loss (tests/golden/disc_lr_small.json) -- exactly on the two constant branches and at pow(., 0), within 1e-13 on the
    pow branches -- and state[0] keeps its bits."""
    L, lib = _lib()
    c = helper_constants(sub_count)
    rows = disc_lr_fixture()["points"][str(sub_count)]
    assert [r[0] for r in rows] == DISC_LR_POINTS[sub_count]
    states = torch.tensor([[last, -1.0] for last, _ in rows], dtype=torch.float64, device=DEV)
    before = states.cpu().clone()
    for i in range(len(rows)):
        L.check(lib.sty_disc_lr_track(L.ptr(states[i]), None, c["ideal_loss"], c["f_max"], c["h_min"], c["x_max"], c["x_min"],
                                      _stream()))
    torch.cuda.synchronize()
    after = states.cpu()
    assert torch.equal(after[:, 0].view(torch.int64), before[:, 0].view(torch.int64)), "state[0] moved without a loss"
    worst = 0.0
    print()
    for (last, want), got in zip(rows, after[:, 1].tolist()):
        branch = restated_multiplier(last, sub_count)[1]
        exact = branch in ("f_max", "h_min") or last == c["ideal_loss"]
        err = abs(got - want) / want
        worst = max(worst, err)
        print(f"  last_loss {last!r:24} {branch:6s} multiplier {got!r:24} fixture {want!r:24} rel {err:.1e}{'  (exact)' if exact else ''}")
        assert (got == want) if exact else (err <= POW_TOL), (last, got, want)
    print(f"  sub_count {sub_count}: worst relative distance {worst:.2e}")


@pytest.mark.parametrize("sub_count", DISC_LR_SUB_COUNTS)
def test_disc_lr_sequence_through_the_helper(sub_count):
    """(d) DISC_LR_SEQUENCE through DiscriminatorLossHelper.track_device, one call per loss, multipliers and running means kept
    on the device and read back once: each multiplier is that of the mean BEFORE the loss is folded in (the order of
    train/stage.py), within 1e-13 of the Python restatement, the mean within 1e-13 after 200 steps.  A second helper on the host
    path (get_disc_lr_multiplier() then track(), as the duration and textual stages use it) gives the restatement's doubles.
    Then the checkpoint-resume path: last_loss set once the device state exists."""
    from stylish_tts_amd.discriminators import DiscriminatorLossHelper
    seq = DISC_LR_SEQUENCE[sub_count]
    want_mults, branches, want_means = restated_sequence(seq, sub_count)
    dev_seq = seq.to(DEV)
    dev_helper, host_helper = DiscriminatorLossHelper(None, sub_count), DiscriminatorLossHelper(None, sub_count)
    mults = torch.zeros(len(seq), dtype=torch.float64, device=DEV)
    means = torch.zeros(len(seq), dtype=torch.float64, device=DEV)
    host_mults = []
    for i in range(len(seq)):
        mults[i:i + 1].copy_(dev_helper.track_device(dev_seq[i:i + 1]))
        means[i:i + 1].copy_(dev_helper._dev[0:1])
        host_mults.append(host_helper.get_disc_lr_multiplier())
        host_helper.track((None, dev_seq[i]))
    torch.cuda.synchronize()
    mults, means = mults.cpu().tolist(), means.cpu().tolist()
    assert host_mults == want_mults and host_helper.last_loss == want_means[-1]
    e_mult = max(abs(a - b) / b for a, b in zip(mults, want_mults))
    e_mean = max(abs(a - b) / b for a, b in zip(means, want_means))
    print(f"\n  sub_count {sub_count}: 200 steps, branches {sorted(set(branches))}: multiplier worst rel {e_mult:.2e}, running mean "
          f"worst rel {e_mean:.2e} (last {abs(means[-1] - want_means[-1]) / want_means[-1]:.2e})")
    assert set(branches) == {"f_max", "h_min", "above", "below"}
    assert e_mult <= POW_TOL and e_mean <= POW_TOL
    assert all(a == b for a, b, br in zip(mults, want_mults, branches) if br in ("f_max", "h_min"))
    assert abs(dev_helper.last_loss - want_means[-1]) <= POW_TOL * want_means[-1]
    # stage_io's resume: the setter reaches the device state, the next multiplier is f_max
    dev_helper.last_loss = 2.9
    got = dev_helper.track_device(None)
    assert got.item() == helper_constants(sub_count)["f_max"] == 4.0
    assert dev_helper.last_loss == 2.9


@functools.lru_cache(maxsize=None)
def _trainer_inputs():
    from oracle.manifest import speech_predictor_manifest, style_encoder_manifest
    from oracle.weights import fill_state_dict
    from safetensors.torch import load_file
    from tests.cases import make_case
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    fx, cfx = load_file(os.path.join(golden, "disc_small.safetensors")), load_file(os.path.join(golden, "cfdisc_small.safetensors"))
    return dict(P=fill_state_dict(speech_predictor_manifest(), 0), Pse=fill_state_dict(style_encoder_manifest(), 0),
                cs=make_case("sp_small"), mrd={k[2:]: v for k, v in fx.items() if k.startswith("w.")},
                wave={k[2:]: v for k, v in cfx.items() if k.startswith("w.")})


def _ulp(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23)


MRD_KEY, WAVE_KEY = "discriminators.1.parametrizations.weight.original1", "last.0.weight"


@pytest.mark.parametrize("mrd2_loss,wave_loss", [(2.6, 0.40), (3.0, 0.48)])
def test_multiplier_reaches_the_trainers_parameters(mrd2_loss, wave_loss):
    """(e) The setup of test_acoustic_train_step_with_spectrogram_discriminators (same inputs and fixtures, disc_index = 2) with
    the helpers' running means preset before the first train_batch.  On the first AdamW step |delta p| = lr x multiplier for every
    element with a gradient well above eps, so the median over a weight tensor is held to lr x the multiplier of the PRESET mean
    (1.741..., 0.01, 4, 0.158... by the fixture's formula), within that test's 2 %: for mrd2's discriminators.1 original1 and the
    waveform discriminator's last.0 weight.  mrd0 and mrd1 do not move; every helper's mean has taken the tracked loss in."""
    import stylish_tts_amd as S
    from stylish_tts_amd.acoustic import AcousticTrainer
    from stylish_tts_amd.discriminators import ContextFreeDiscriminator, SpecDiscriminator
    from tests.test_hip_parity import _test_audio
    fx = _trainer_inputs()
    cs = fx["cs"]
    B, T = cs["pitch"].shape
    audio_gt = _test_audio(B, 300 * T, 21)
    mrd = []
    for r in range(3):
        m = SpecDiscriminator().to(DEV)
        m.load_state_dict(fx["mrd"])
        mrd.append(m)
    sp = S.SpeechPredictor()
    sp.load_state_dict({k: v.clone() for k, v in fx["P"].items()}, strict=False)
    se = S.MelStyleEncoder()
    se.load_state_dict(fx["Pse"])
    wave_disc = ContextFreeDiscriminator()
    wave_disc.load_state_dict(fx["wave"])
    wave_disc = wave_disc.to(DEV)
    lr, wd = 1e-3, 1e-4
    want = {"mrd2": restated_multiplier(mrd2_loss, 5)[0], "wave": restated_multiplier(wave_loss, 1)[0]}
    formula = {2.6: 4.0 ** 0.4, 3.0: 4.0, 0.40: 0.01, 0.48: 0.01 ** 0.4}
    assert abs(want["mrd2"] - formula[mrd2_loss]) <= 1e-12 and abs(want["wave"] - formula[wave_loss]) <= 1e-12
    tr = AcousticTrainer(sp.to(DEV), se.to(DEV), lr=lr, train_mode=False, mrd=mrd, w_gen=1.0, disc=wave_disc)
    tr.disc_helpers[2].last_loss = mrd2_loss
    tr.disc_helper.last_loss = wave_loss
    before = [{k: p.detach().cpu().clone() for k, p in m.named_parameters()} for m in mrd]
    wave_before = {k: p.detach().cpu().clone() for k, p in wave_disc.named_parameters()}
    # premise: the smallest effective rate (multiplier h_min) is at least 100 ulp of the checked tensors' typical magnitude
    for b in (before[2][MRD_KEY], wave_before[WAVE_KEY]):
        assert 0.01 * lr >= 100 * _ulp(b.abs().median().item()), (0.01 * lr, _ulp(b.abs().median().item()))
    tr.train_batch(disc_index=2, audio_gt=audio_gt.to(DEV), texts=cs["texts"].to(DEV), text_lengths=cs["text_lengths"].to(DEV),
                   pitch=cs["pitch"].to(DEV), durations=cs["durations"].to(DEV), noise=cs["noise"].to(DEV), seed=5)
    torch.cuda.synchronize()
    gan, gw = tr.gan.cpu(), tr.gan_wave.cpu()
    assert torch.isfinite(gan).all() and torch.isfinite(gw).all()

    def median_step(after, b, rate):
        return (after.detach().cpu().double() - b.double() * (1 - rate * wd)).abs().median().item()

    print()
    for label, params, b4, key, mult in (("mrd2", dict(mrd[2].named_parameters()), before[2], MRD_KEY, want["mrd2"]),
                                         ("wave", dict(wave_disc.named_parameters()), wave_before, WAVE_KEY, want["wave"])):
        rate = lr * mult
        for k, p in params.items():
            if p.dim() >= 2:
                print(f"  {label} {k:56s} median |delta p| / (lr x multiplier) {median_step(p, b4[k], rate) / rate:.4f}")
        got = median_step(params[key], b4[key], rate)
        assert abs(got - rate) <= 0.02 * rate, (label, key, got, rate)
    for r, m in enumerate(mrd):
        moved = max((p.detach().cpu() - before[r][n]).abs().max().item() for n, p in m.named_parameters())
        assert (moved > 0) == (r == 2), (r, moved)
        preset = mrd2_loss if r == 2 else 2.5
        assert abs(tr.disc_helpers[r].last_loss - (0.95 * preset + 0.05 * gan[2 + 2 * r].item())) <= 1e-5
    assert abs(tr.disc_helper.last_loss - (0.95 * wave_loss + 0.05 * gw[2].item())) <= 1e-5
