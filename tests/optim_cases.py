"""Cases and oracles of the optimizer side (csrc/optim.hip: adamw_kernel, disc_lr_track_kernel), shared by
tests/test_optim_oracle.py (CPU) and tests/test_optim_edges.py (GPU).

AdamW: the oracle is torch.optim.AdamW itself (the reference's optimizer, train/optimizers.py:110-118) on float64 CPU clones, and
on float32 clones for the fp32 anchor the gates are derived from.  The rate multiplier: a plain-Python restatement of
train/losses.py:238-249 and of the running mean of :287, written from the reference's text (nothing of stylish_tts_amd is
imported here), and tests/golden/disc_lr_small.json recorded from the reference's own helper (tools/gen_golden_disc_lr.py).
"""
import functools
import json
import math
import os
from fractions import Fraction

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_HP = dict(lr=1e-4, wd=1e-4, betas=(0.85, 0.99), eps=1e-9)  # train/optimizers.py:110-118

# ---- bucket sizes n --------------------------------------------------------------------------------------------------------
# From launch_adamw / adamw_kernel as they stand: a workgroup is 256 threads of one float4 each (1024 elements), n4 = n / 4,
# blocks = ceil(n4 / 256) capped at 256 * 16 = 4096 (4 194 304 elements a trip of the grid-stride loop) and at least 1; the
# n - 4 n4 tail elements are taken by workgroup 0, thread by thread.
WG = 256 * 4
GRID_CAP = 256 * 16 * WG
ADAMW_SIZE_CASES = [
    1, 3,                                # n4 == 0: one workgroup, the tail loop alone
    4, 5, 7,                             # one float4, and one float4 with a tail of 1 and of 3
    WG - 1, WG, WG + 1,                  # one full workgroup of float4 and its neighbours
    WG + 4, 2 * WG - 1, 2 * WG, 2 * WG + 1, 2 * WG + 5,  # the first float4 of a second workgroup; its end; a third one with a tail
    GRID_CAP,                            # the grid cap exactly: every thread one float4, no second trip
    GRID_CAP + WG + 3,                   # the second trip of the grid-stride loop (workgroup 0 only) and a tail of 3
]
SIZE_STEPS = {n: (2 if n >= GRID_CAP else 6) for n in ADAMW_SIZE_CASES}
N_REGIME = WG + 5  # 1029: two workgroups and a tail of 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _case(family, name, n, hp, p0, grads, step0=1, m0=None, v0=None, grad_scale=1.0):
    """One AdamW case.  p0, m0, v0 [n] and grads [steps, n] are float32 (what the kernel reads); the steps are numbered step0,
    step0 + 1, ...  grad_scale is the float32 value the kernel multiplies the gradient by."""
    if m0 is None:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    gs = float(torch.tensor(grad_scale, dtype=torch.float32).item())
    assert p0.dtype == m0.dtype == v0.dtype == grads.dtype == torch.float32 and grads.shape[1] == n and (v0 >= 0).all()
    return dict(family=family, name=name, n=n, hp=hp, p0=p0, grads=grads, step0=step0, m0=m0, v0=v0, grad_scale=gs)


def _params(n, seed):
    return 0.05 * torch.randn(n, generator=_gen(seed))  # fp32 rounding of p small against the movement


def _size_case(n):
    """the reference's hyper-parameters; the gradient's scale changes from step to step (1e-2, 1e-1, 1, ...)"""
    steps = SIZE_STEPS[n]
    g = _gen(1000 + n % 9973)
    grads = torch.stack([torch.randn(n, generator=g) * 10.0 ** (it % 3 - 2) for it in range(steps)])
    return _case("size", f"n{n}", n, REF_HP, _params(n, 7 + n % 9973), grads)


def _eps_grads(n, steps, seed):
    """exact zeros on every third element (on all steps: m = v = 0 there throughout), magnitudes 10^k, k = -12 .. -8, elsewhere:
    sqrt(v) / bc2s and eps = 1e-9 are of the same order"""
    g = _gen(seed)
    k = torch.randint(-12, -7, (n,), generator=g).float()
    sign = torch.randint(0, 2, (steps, n), generator=g).float() * 2 - 1
    grads = sign * (0.5 + torch.rand(steps, n, generator=g)) * 10.0 ** k
    grads[:, ::3] = 0.0
    return grads


def _wide_grads(n, steps, seed):
    """magnitudes 10^k, k uniform in [-6, 6], drawn anew on every step"""
    g = _gen(seed)
    k = torch.rand(steps, n, generator=g) * 12 - 6
    grads = (torch.randint(0, 2, (steps, n), generator=g).float() * 2 - 1) * 10.0 ** k
    a = grads.abs()
    # fp32 g * g (and (1 - b2) g * g) neither overflows nor goes subnormal: 1e-12 and 1e+12 against 1.2e-38 / 3.4e+38
    assert a.min().item() >= 0.9e-6 and a.max().item() <= 1.1e6
    assert (a.min().item() ** 2) * 0.01 > 1.2e-38 * 1e6 and a.max().item() ** 2 < 3.4e38 / 1e6
    return grads


def _regime_cases():
    n, steps = N_REGIME, 6
    randn = lambda seed, *s: torch.randn(*s, generator=_gen(seed))
    vis = dict(lr=1e-2, wd=0.1, betas=(0.85, 0.99), eps=1e-9)
    out = [_case("a", "a-reference", n, REF_HP, _params(n, 11), randn(12, steps, n)),
           _case("b", "b-decay", n, vis, _params(n, 13), randn(14, steps, n)),
           _case("c", "c-eps", n, REF_HP, _params(n, 15), _eps_grads(n, steps, 16)),
           _case("d", "d-wide", n, REF_HP, _params(n, 17), _wide_grads(n, steps, 18))]
    for label, s in (("1/2", 0.5), ("1/8", 0.125), ("1/3", 1.0 / 3.0)):
        out.append(_case("e", f"e-gscale{label}", n, vis, _params(n, 19), randn(20, steps, n), grad_scale=s))
    for t in (1, 2, 10, 1000, 1000000):  # one step each from preset moments; at 1e6 both beta^t underflow: corrections exactly 1
        m0 = 0.1 * randn(22, n)
        v0 = (0.1 * randn(23, n)) ** 2 + 1e-4
        out.append(_case("f", f"f-step{t}", n, vis, _params(n, 21), randn(24 + t % 7, 1, n), step0=t, m0=m0, v0=v0))
    return out


def decay_roundings(lr32, wd32):
    """fp32(1 - lr wd) from the fp32 values lr, wd -> (the product rounded first: a multiply, then a subtract, what host code does;
    one rounding: what a contracted FMA gives), both as Python floats"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    apart = (f(1.0) - f(lr32) * f(wd32)).item()
    exact = 1 - Fraction(lr32) * Fraction(wd32)
    assert Fraction(1, 2) <= exact < 1  # one ulp is 2^-24 there; round() of a Fraction is to nearest, ties to even
    return apart, float(Fraction(round(exact * 2 ** 24), 2 ** 24))


@functools.lru_cache(maxsize=None)
def _contract_case():
    """Regime (b) with the weight decay moved from 0.1 by a few thousand fp32 steps at most, to the first value at which, for one of
    ADAMW_SCALED_MULTS, fp32(1 - lr wd) depends on whether lr wd is rounded before the subtraction (about one pair in a thousand:
    at regime (b) itself all five multipliers give the same decay either way, so a contracted FMA in the kernel cannot show there)."""
    base = adamw_cases_without_contract()["b-decay"]
    wd0 = torch.tensor(0.1, dtype=torch.float32)
    for k in range(20000):
        wd32 = (wd0.view(torch.int32) + k).view(torch.float32).item()
        for mult in ADAMW_SCALED_MULTS:
            lr32 = torch.tensor(base["hp"]["lr"] * mult, dtype=torch.float64).float().item()
            apart, fused = decay_roundings(lr32, wd32)
            if apart != fused:
                assert abs(apart - fused) == 2.0 ** -24
                hp = dict(base["hp"], wd=wd32)
                return dict(base, family="b", name="b-contract", hp=hp), mult
    raise AssertionError("no weight decay near 0.1 separates the two roundings")


@functools.lru_cache(maxsize=None)
def adamw_cases_without_contract():
    cases = [_size_case(n) for n in ADAMW_SIZE_CASES] + _regime_cases()
    return {c["name"]: c for c in cases}


@functools.lru_cache(maxsize=None)
def adamw_cases():
    """every case, by name"""
    case, _ = _contract_case()
    return dict(adamw_cases_without_contract(), **{case["name"]: case})


def contract_case():
    """-> ('b-contract', the multiplier at which the two roundings of its decay differ)"""
    case, mult = _contract_case()
    return case["name"], mult


ADAMW_SIZE_NAMES = [f"n{n}" for n in ADAMW_SIZE_CASES]
ADAMW_REGIME_CASES = ["a-reference", "b-decay", "c-eps", "d-wide", "e-gscale1/2", "e-gscale1/8", "e-gscale1/3",
                      "f-step1", "f-step2", "f-step10", "f-step1000", "f-step1000000"]
FAMILIES = ("size", "a", "b", "c", "d", "e", "f")
# the scaled entry point (sty_adamw_step_scaled): regimes (a) and (b) at lr_d x these multipliers -- h_min, 0.01^0.4, pow(., 0), 4^0.4, f_max
ADAMW_SCALED_CASES = ("a-reference", "b-decay")
ADAMW_SCALED_MULTS = (0.01, 0.1584893192461111, 1.0, 1.7411011265922491, 4.0)


# ---- AdamW oracle ------------------------------------------------------------------------------------------------------------
def torch_adamw(case, dtype, lr=None):
    """torch.optim.AdamW (single-tensor path) on CPU clones of the case in `dtype` -> (p, m, v) after the case's steps.  The
    state of a case that starts at step0 > 1, or from preset moments, goes in through load_state_dict; grad_scale is applied to
    the gradient, in `dtype`, before torch sees it.  `lr` overrides the case's rate (the scaled entry point: lr_d * multiplier)."""
    hp = case["hp"]
    p = torch.nn.Parameter(case["p0"].to(dtype).clone())
    opt = torch.optim.AdamW([p], lr=hp["lr"] if lr is None else lr, betas=hp["betas"], eps=hp["eps"], weight_decay=hp["wd"],
                            foreach=False)
    if case["step0"] > 1 or bool(case["m0"].any()) or bool(case["v0"].any()):
        sd = opt.state_dict()
        sd["state"] = {0: {"step": torch.tensor(float(case["step0"] - 1)), "exp_avg": case["m0"].to(dtype).clone(),
                           "exp_avg_sq": case["v0"].to(dtype).clone()}}
        opt.load_state_dict(sd)
    for g in case["grads"]:
        p.grad = g.to(dtype) * torch.tensor(case["grad_scale"], dtype=dtype)
        opt.step()
    st = opt.state[p]
    assert int(st["step"].item()) == case["step0"] - 1 + len(case["grads"])
    return p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


@functools.lru_cache(maxsize=None)
def oracle64(name, lr=None):
    """the float64 reference of a case, computed once and shared (read-only)"""
    return torch_adamw(adamw_cases()[name], torch.float64, lr)


def distances(case, got, ref):
    """the metric, per tensor: p as max |got - ref| / max |p_ref_after - p_before|, m and v as max |got - ref| / max |ref|.
    got, ref: (p, m, v); -> (e_p, e_m, e_v)"""
    got = [t.detach().double().cpu() for t in got]
    ref = [t.detach().double().cpu() for t in ref]
    moved = (ref[0] - case["p0"].double()).abs().max().item()
    assert moved > 0
    e_p = (got[0] - ref[0]).abs().max().item() / moved
    return (e_p,) + tuple((g - r).abs().max().item() / r.abs().max().item() for g, r in zip(got[1:], ref[1:]))


def _restated_adamw(case, wrong=None):
    """AdamW step by step in float64, the operation order of torch's single-tensor path; `wrong` names one mistake"""
    hp = case["hp"]
    lr, wd, eps, (b1, b2) = hp["lr"], hp["wd"], hp["eps"], hp["betas"]
    if wrong == "betas_swapped":
        b1, b2 = b2, b1
    p, m, v = case["p0"].double().clone(), case["m0"].double().clone(), case["v0"].double().clone()
    for i, g in enumerate(case["grads"]):
        t = case["step0"] + i
        g = g.double()
        gm = g * case["grad_scale"]
        gv = g if wrong == "grad_scale_not_squared" else gm
        if wrong == "l2_weight_decay":
            gm = gv = gm + wd * p
        else:
            p = p * (1 - lr * wd)
        m = m + (1 - b1) * (gm - m)
        v = v * b2 + (1 - b2) * gv * gv
        tb = t - 1 if (wrong == "bias_correction_t_minus_1" and t >= 2) else t
        bc1, bc2s = 1 - b1 ** tb, math.sqrt(1 - b2 ** tb)
        denom = (v.sqrt() + eps) / bc2s if wrong == "eps_inside_bias_correction" else v.sqrt() / bc2s + eps
        p = p - (lr / bc1) * (m / denom)
    return p, m, v


# float64 restatements of the step, each with one mistake a kernel could make (None: the restatement itself, which must BE the oracle)
WRONG_VARIANTS = {
    "l2_weight_decay": "weight decay added to the gradient (Adam's L2 form) instead of p *= 1 - lr wd",
    "eps_inside_bias_correction": "(sqrt(v) + eps) / bc2s instead of sqrt(v) / bc2s + eps",
    "betas_swapped": "beta1 and beta2 exchanged",
    "grad_scale_not_squared": "grad_scale applied to g in m but not to g * g in v",
    "bias_correction_t_minus_1": "both bias corrections with t - 1 for t >= 2",
}


def wrong_adamw(name, variant):
    return _restated_adamw(adamw_cases()[name], variant)


# ---- the discriminators' rate multiplier ---------------------------------------------------------------------------------------
def helper_constants(sub_count):
    """DiscriminatorLossHelper.__init__ (train/losses.py:231-236), the same double expressions"""
    return dict(ideal_loss=0.5 * sub_count, f_max=4.0, h_min=0.01, x_max=0.05 * sub_count, x_min=0.05 * sub_count)


def restated_multiplier(last_loss, sub_count):
    """train/losses.py:238-249 -> (multiplier, branch); branch: 'f_max', 'h_min' (the constant ones), 'above', 'below' (the pow
    ones; last_loss == ideal takes 'below' with pow(h_min, 0))"""
    c = helper_constants(sub_count)
    x = abs(last_loss - c["ideal_loss"])
    if last_loss > c["ideal_loss"] + c["x_max"]:
        return c["f_max"], "f_max"
    if last_loss < c["ideal_loss"] - c["x_min"]:
        return c["h_min"], "h_min"
    if last_loss > c["ideal_loss"]:
        return min(math.pow(c["f_max"], x / c["x_max"]), c["f_max"]), "above"
    return max(math.pow(c["h_min"], x / c["x_min"]), c["h_min"]), "below"


def restated_track(last_loss, tracked):
    """the running mean of train/losses.py:287; `tracked` is what disc.item() gave"""
    return last_loss * 0.95 + tracked * 0.05


def _disc_lr_points(sub_count):
    """last_loss values on, beside and between every threshold of the four branches; thresholds by the helper's own double
    expressions"""
    n = sub_count
    ideal, hi, lo = 0.5 * n, 0.5 * n + 0.05 * n, 0.5 * n - 0.05 * n
    up, down = (lambda a: math.nextafter(a, math.inf)), (lambda a: math.nextafter(a, -math.inf))
    return [ideal, up(ideal), down(ideal),
            hi, up(hi), down(hi),      # on the upper band edge (still the pow branch), one ulp beyond it, one ulp inside
            lo, down(lo), up(lo),
            0.52 * n, 0.48 * n,        # mid-band: 2.6 and 2.4 at sub_count 5
            0.0, 10.0]


DISC_LR_SUB_COUNTS = (5, 1)  # the spectrogram discriminators' helpers and the waveform discriminator's
DISC_LR_POINTS = {n: _disc_lr_points(n) for n in DISC_LR_SUB_COUNTS}


def _disc_lr_sequence(sub_count):
    """200 seeded tracked losses (float32, what the loss kernels hand over).  Plateaus of 25 steps far above, far below and inside
    the band with a little noise: the running mean crosses the ideal loss and both band edges at least twice and spends steps in
    all four branches (asserted here)."""
    g = _gen(40 + sub_count)
    levels = [0.8, 0.2, 0.8, 0.2, 0.9, 0.1, 0.53, 0.47]
    base = torch.tensor(levels, dtype=torch.float64).repeat_interleave(25) + 0.02 * torch.randn(200, generator=g).double()
    seq = (base * sub_count).float()
    c = helper_constants(sub_count)
    last, means, visits = c["ideal_loss"], [], {"f_max": 0, "h_min": 0, "above": 0, "below": 0}
    for x in seq.tolist():
        visits[restated_multiplier(last, sub_count)[1]] += 1
        last = restated_track(last, x)
        means.append(last)
    crossings = lambda level: sum((a - level) * (b - level) < 0 for a, b in zip(means, means[1:]))
    assert min(visits.values()) >= 8, visits
    assert all(crossings(lv) >= 2 for lv in (c["ideal_loss"], c["ideal_loss"] + c["x_max"], c["ideal_loss"] - c["x_min"]))
    return seq


DISC_LR_SEQUENCE = {n: _disc_lr_sequence(n) for n in DISC_LR_SUB_COUNTS}


def restated_sequence(seq, sub_count, last_loss=None):
    """the order of train/stage.py: the multiplier of the mean BEFORE each loss is folded in -> (multipliers, branches, means)"""
    last = helper_constants(sub_count)["ideal_loss"] if last_loss is None else last_loss
    mults, branches, means = [], [], []
    for x in seq.tolist():
        m, b = restated_multiplier(last, sub_count)
        last = restated_track(last, x)
        mults.append(m)
        branches.append(b)
        means.append(last)
    return mults, branches, means


def disc_lr_fixture():
    """tests/golden/disc_lr_small.json: {"constants": {sub_count: {...}}, "points": {sub_count: [[last_loss, multiplier], ...]}}"""
    with open(os.path.join(GOLDEN, "disc_lr_small.json")) as f:
        return json.load(f)
