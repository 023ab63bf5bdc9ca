"""Shared by tests/test_discriminators.py, tests/test_disc_oracle.py and tests/test_disc_edges.py: the fixtures, the three families'
oracle passes in a chosen precision, the float64-sum loss reference, and the two-part device check.

The two-part scheme.  The relativistic term sends d rel / d m through torch.median's backward, which divides it evenly among the
elements EQUAL to the median: without ties that is a spike on one score element, so score maps that differ in the last bit can
move it to another element.  The comparison is therefore made in two exact halves: (1) the loss kernels against the loss
functions evaluated ON THE DEVICE'S SCORE MAPS (same inputs bit for bit -> same median, same membership); (2) the network
backward against the oracle network's backward fed with those score gradients.  `dtype` chooses the precision of the oracle
network (torch.float32: the pinned oracle as it is; torch.float64: the same code on .double() parameters and inputs), `loss64`
chooses the loss reference (False: the fp32 oracle's value; True: loss_reference64 below).
"""
import os

import torch
import torch.nn.functional as F
from safetensors.torch import load_file

from oracle import discriminator as od

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the gates of test_discriminators.py: scores, d_pred / parameter gradients (x w_factor for original0), loss values
GATES = {"spec": dict(score=2e-5, grad=2e-4, g0=5.0, loss=2e-5), "wave": dict(score=2e-5, grad=5e-4, g0=1.0, loss=5e-5),
         "seq": dict(score=2e-5, grad=2e-4, g0=5.0, loss=2e-5)}


def spec_fixture():
    fx = load_file(os.path.join(G, "disc_small.safetensors"))
    return fx, {k[2:]: v for k, v in fx.items() if k.startswith("w.")}


def cf_fixture():
    fx = load_file(os.path.join(G, "cfdisc_small.safetensors"))
    return fx, {k[2:]: v for k, v in fx.items() if k.startswith("w.")}


def pd_fixture(name):
    fx = load_file(os.path.join(G, "pdisc_small.safetensors"))
    params = {k[len(name) + 3:]: v for k, v in fx.items() if k.startswith(name + ".w.")}
    return {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + ".") and ".w." not in k[:len(name) + 3]}, params


def seq_params(name, dim_in, K):
    from tests.cases import disc_seq_params
    return pd_fixture(name)[1] if name != "seeded" else disc_seq_params(dim_in, K)


def hip_spec_model(params, dev):
    from stylish_tts_amd.discriminators import SpecDiscriminator
    m = SpecDiscriminator().to(dev)
    missing = m.load_state_dict(params, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m


def hip_cf_model(params, dev):
    from stylish_tts_amd.discriminators import ContextFreeDiscriminator
    m = ContextFreeDiscriminator()
    m.load_state_dict(params, strict=True)
    return m.to(dev)


def hip_seq_model(params, dim_in, K, dev):
    from stylish_tts_amd.discriminators import PitchDiscriminator
    m = PitchDiscriminator(dim_in=dim_in, kernel=K)
    m.load_state_dict(params, strict=True)
    return m.to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# which dense kernel family every forward and input-gradient conv of a case takes (sty_conv1d_route; host only)
# ---------------------------------------------------------------------------------------------------------------------
CONV_FAMILIES = ["stem2d", "conv32p", "convsc", "convk1", "convq", "convp16", "tiled"]
_OUT_MASK, _RESIDUAL, _RELU, _FLAT = 4, 2, 8, 256  # STY_ROUTE_* of include/stylish_hip.h


def spec_geometry(W):
    """SdRun::geometry: (valid widths, row pitches) of the five levels"""
    wl = [W]
    for _ in range(3):
        wl.append((wl[-1] + 1) // 2)
    wl.append(wl[-1])
    p3 = (wl[3] + 4 + 3) // 4 * 4
    return wl, [8 * p3, 4 * p3, 2 * p3, p3, p3]


def conv_routes(family, case, bf16=False):
    """[(conv, forward family or None, input-gradient family)] of a case of tests/cases.py, as the runs of disc.hip / cfdisc.hip
    build their ConvArgs (the activation of the bf16-mode forward convs, LeakyReLU in convp16's output stage, is not part of the
    query: it only asks T % 4 == 0 of that family, which every flat image satisfies)."""
    import ctypes as C
    from stylish_tts_amd import lib as L
    lib = L.load()

    def route(B, cin, cout, K, T, flags):
        k = C.c_int()
        L.check(lib.sty_conv1d_route(B, cin, cout, K, 1, T, int(bf16), flags, C.byref(k)))
        return CONV_FAMILIES[k.value]

    out = []
    if family == "spec":
        B, H, W = case
        _, wp = spec_geometry(W)
        out.append(("level 0", None, route(B, 32, 27, 1, H * wp[0], 0)))  # forward: sd_l0_kernel; d_pred only: 32 -> 27 pointwise
        for i in range(1, 5):
            c2d, K = (64, 5) if i < 4 else (32, 3)
            out.append((f"level {i}", route(B, 3 * c2d, 32, K, H * wp[i], _OUT_MASK | _FLAT), route(B, 96, c2d, K, H * wp[i], _FLAT)))
    elif family == "wave":
        B, N = case
        t = (N - 1024) // 512 + 1
        Tl = [t * p for p in (1280, 320, 80, 40, 20)]
        descs = [(1, 64, 11, 4), (64, 128, 11, 4), (128, 256, 7, 2), (256, 256, 5, 2), (256, 256, 7, 1), (256, 256, 3, 1),
                 (256, 768, 1, 1), (768, 256, 1, 1), (256, 256, 1, 1), (256, 256, 1, 1), (256, 256, 1, 1), (256, 512, 1, 1), (512, 1, 1, 1)]
        names = ["conv.0", "conv.1", "conv.2", "conv.3", "temporal.0", "temporal.1", "spectral.0", "spectral.1", "fusion (a)",
                 "fusion (b)", "attn.1", "last.0", "last.2"]
        for i, (cin, cout, K, s) in enumerate(descs):
            pad = K // 2
            qmin, qmax = -((pad + s - 1) // s), (K - 1 - pad) // s
            kp = qmax - qmin + 1
            if kp == 4 and cin * s >= 64 and cout >= 64:
                kp = 5
            T = Tl[i + 1] if i < 4 else (t if i == 10 else Tl[4])
            flags = (0 if i == 10 else _OUT_MASK) | (_RESIDUAL if i == 9 else 0) | (_RELU if i == 11 else 0)
            cinp, coutp = (cin * s + 31) // 32 * 32, (cout + 31) // 32 * 32
            out.append((names[i], route(B, cin * s, cout, kp, T, flags), route(B, coutp, cinp, kp, T, _RESIDUAL if i == 4 else 0)))
    else:
        _, dim_in, K, B, T = case
        for i in range(5):
            cin = dim_in if i == 0 else 64
            out.append((f"layer {i}", route(B, cin, 64, K, T, 0), route(B, 64, (cin + 31) // 32 * 32, K, T, 0)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the families' oracle networks
# ---------------------------------------------------------------------------------------------------------------------
def family_scores(family, p, x):
    """list of score maps [B, n_i] of one input"""
    if family == "spec":
        return od.spec_discriminator(p, x)
    if family == "wave":
        return [od.context_free_discriminator(p, x)]
    return od.pitch_discriminator(p, x)


def grad_keys(family, params):
    if family == "wave":
        return sorted(k for k, v in params.items() if v.is_floating_point() and "running" not in k)
    return sorted(params)


def loss_cotangents(rs, gs):
    """fp32 loss oracle on given score maps -> (gen loss, disc loss, d gen / d gs, d disc / d rs, d disc / d gs)"""
    rs = [x.detach().clone().requires_grad_(True) for x in rs]
    gs = [x.detach().clone().requires_grad_(True) for x in gs]
    gl = od.generator_loss_helper(rs, gs)
    g_gen = torch.autograd.grad(gl, gs)
    dl = od.discriminator_loss_helper(rs, gs)
    g_dr = torch.autograd.grad(dl, rs, retain_graph=True)
    g_dg = torch.autograd.grad(dl, gs)
    return gl.detach(), dl.detach(), list(g_gen), list(g_dr), list(g_dg)


def oracle_pass(family, params, t, q0, cots, dtype=torch.float32):
    """The oracle network in `dtype` with injected score cotangents cots = (g_gen, g_dr, g_dg) (lists per level):
    -> (scores of t, scores of q0, d / d q0 under g_gen, {key: d / d parameter under (g_dr, g_dg)}), all in `dtype`."""
    keys = grad_keys(family, params)
    pp = {k: (v.to(dtype).clone().requires_grad_(True) if k in keys else v) for k, v in params.items()}
    q = q0.to(dtype).clone().requires_grad_(True)
    so_t, so_q = family_scores(family, pp, t.to(dtype)), family_scores(family, pp, q)
    g_gen, g_dr, g_dg = ([c.to(dtype) for c in cs] for cs in cots)
    dq, = torch.autograd.grad(so_q, q, grad_outputs=g_gen, retain_graph=True)
    dw = torch.autograd.grad(so_t + so_q, [pp[k] for k in keys], grad_outputs=g_dr + g_dg)
    return [s.detach() for s in so_t], [s.detach() for s in so_q], dq, dict(zip(keys, dw))


def rel_errors(family, got, ref):
    """got / ref = (scores_t, scores_q, dq, dw): every quantity's error over its gate's norm -- max |ref| with the floor 0.1 for a
    score map and 1e-3 for a parameter gradient, max |d_pred| without a floor -- as {quantity: error}; the parameter gradients
    as "grad" (worst tensor other than original0) and "grad.original0"."""
    out = {"score": 0.0, "grad": 0.0, "grad.original0": 0.0}
    for a, b in zip(got[0] + got[1], ref[0] + ref[1]):
        out["score"] = max(out["score"], (a.double() - b.double()).abs().max().item() / max(b.abs().max().item(), 0.1))
    out["d_pred"] = (got[2].double() - ref[2].double()).abs().max().item() / ref[2].abs().max().item()
    for k, b in ref[3].items():
        e = (got[3][k].double() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-3)
        q = "grad.original0" if k.endswith("original0") else "grad"
        out[q] = max(out[q], e)
    return out


def gate_of(family, quantity):
    g = GATES[family]
    return {"score": g["score"], "d_pred": g["grad"], "grad": g["grad"], "grad.original0": g["grad"] * g["g0"], "loss": g["loss"]}[quantity]


# ---------------------------------------------------------------------------------------------------------------------
# the two loss helpers with a replaceable median, and their float64-sum reference
# ---------------------------------------------------------------------------------------------------------------------
def median_even(d):
    """torch.median of the full reduction: the lower median; its backward divides the gradient evenly among the elements equal to it"""
    return torch.median(d)


def median_first(d):
    """same value, the whole gradient on the FIRST element holding it"""
    f = d.flatten()
    return f[(f == torch.median(f.detach())).nonzero()[0, 0]]


def median_upper(d):
    f = d.flatten()
    return f.sort().values[f.numel() // 2]


def loss_helpers(rs, gs, median=median_even):
    """(generator helper, discriminator helper) as oracle/discriminator.py states them, with the median rule as a parameter"""
    gen = 0
    for g in gs:
        gen = gen + torch.mean((1 - g) ** 2)
    for r, g in zip(rs, gs):
        m = median(g - r)
        gen = gen + (od.TAU - F.relu(od.TAU - torch.mean((((g - r) - m) ** 2)[g < r + m])))
    disc = 0
    for r, g in zip(rs, gs):
        disc = disc + torch.mean((1 - r) ** 2) + torch.mean(g ** 2)
    for r, g in zip(rs, gs):
        m = median(r - g)
        sel = (((r - g) - m) ** 2)[r < g + m]
        disc = disc + (od.TAU - F.relu(od.TAU - torch.sum(sel) / (sel.numel() + 1e-9)))
    return gen, disc


def rel_terms(rs, gs):
    """per level: (ties of the generator form, rel of it, ties of the discriminator form, rel of it), fp32 as the oracle computes"""
    out = []
    for r, g in zip(rs, gs):
        row = []
        for d, a, b in ((g - r, g, r), (r - g, r, g)):
            m = torch.median(d)
            sel = ((d - m) ** 2)[a < b + m]
            row += [int((d == m).sum()), (sel.sum() / max(sel.numel(), 1)).item()]
        out.append(tuple(row))
    return out


def loss_reference64(rs, gs):
    """The float64 reference of the two loss values on given fp32 score maps: the median, the membership mask d < m in its fp32
    form (a < b + m as the helpers write it) and the decision tau - rel > 0 are taken in fp32 -- a float64 predicate would move
    single elements across the kink, which is no error of the sums -- and every sum over that membership is a float64 sum of the
    exactly widened operands."""
    tau32 = torch.tensor(od.TAU, dtype=torch.float32)
    out = []
    for gen in (True, False):
        total = 0.0
        for r, g in zip(rs, gs):
            a, b = (g, r) if gen else (r, g)
            d = a - b
            m = torch.median(d)
            mask = a < b + m
            sel32 = ((d - m) ** 2)[mask]
            rel32 = sel32.mean() if gen else sel32.sum() / (sel32.numel() + 1e-9)
            act = bool(tau32 - rel32 > 0)
            s64 = (((a.double() - b.double()) - m.double()) ** 2)[mask].sum().item()
            rel64 = s64 / (int(mask.sum()) + (0.0 if gen else 1e-9))
            total += rel64 if act else od.TAU
            total += ((1 - g.double()) ** 2).mean().item() if gen else ((1 - r.double()) ** 2).mean().item() + (g.double() ** 2).mean().item()
        out.append(total)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------
# the device check
# ---------------------------------------------------------------------------------------------------------------------
def two_part_check(family, m, params, t, q0, dev, tol_x, tol_w, tol_loss, w0_factor=1.0, dtype=torch.float32, loss64=False,
                   check_scores=True, rec=None):
    """m: the HIP module; asserts the device's score maps, both loss values, d_pred (gen_scale 2) and the parameter gradients
    (disc_scale 3) as the module docstring says.  rec (a dict) receives every measured error over its norm.
    -> (gen, disc, d_pred) of the combined call."""
    td, qd = t.to(dev), q0.to(dev)
    rs_h = [x.cpu().clone() for x in m(td)[0]]
    gs_h = [x.cpu().clone() for x in m(qd)[0]]
    gl, dl, g_gen, g_dr, g_dg = loss_cotangents(rs_h, gs_h)
    if loss64:
        gl, dl = loss_reference64(rs_h, gs_h)
    else:
        gl, dl = gl.item(), dl.item()
    so_t, so_q, dq, dw = oracle_pass(family, params, t, q0, (g_gen, g_dr, g_dg), dtype)
    rec = {} if rec is None else rec
    rec["score"] = 0.0
    if check_scores:
        for a_, b_ in zip(so_t + so_q, rs_h + gs_h):  # the HIP score maps themselves
            err = (a_ - b_.to(dtype)).abs().max().item()
            rec["score"] = max(rec["score"], err / max(a_.abs().max().item(), 0.1))
            assert err <= tol_x * max(a_.abs().max().item(), 0.1), ("score", err)
    for p_ in m.parameters():
        p_.grad = None
    d_pred = torch.zeros(qd.shape[0], *qd.shape[2:], device=dev) if family == "spec" else torch.zeros_like(qd)
    gen, disc = m.losses(td, qd, gen_scale=2.0, d_pred=d_pred, disc_scale=3.0)
    rec["loss.gen"], rec["loss.disc"] = abs(gen[0].item() - gl) / gl, abs(disc[0].item() - dl) / dl
    assert abs(gen[0].item() - gl) <= tol_loss * gl, (gen[0].item(), gl)
    assert abs(disc[0].item() - dl) <= tol_loss * dl, (disc[0].item(), dl)
    dq = dq[:, 0] if family == "spec" else dq
    err = (d_pred.cpu().to(dtype) - 2.0 * dq).abs().max().item()
    rec["d_pred"] = err / (2.0 * dq.abs().max().item())
    assert err <= tol_w * 2.0 * dq.abs().max().item(), ("d_pred", err, dq.abs().max().item())
    got = dict(m.named_parameters())
    rec["grad"] = rec["grad.original0"] = 0.0
    for k, ref in dw.items():
        ref = 3.0 * ref
        err = (got[k].grad.cpu().to(dtype) - ref).abs().max().item()
        is0 = k.endswith("original0")
        lim = tol_w * (w0_factor if is0 else 1.0) * max(ref.abs().max().item(), 1e-3)
        q = "grad.original0" if is0 else "grad"
        rec[q] = max(rec[q], err / max(ref.abs().max().item(), 1e-3))
        assert err <= lim, (k, err, ref.abs().max().item())
    return gen, disc, d_pred


def check_against_oracle(m, params, t, q0, dev, tol_x, tol_w, tol_loss=2e-5, **kw):
    """spectrogram discriminator: original0 at 5 x tol_w"""
    return two_part_check("spec", m, params, t, q0, dev, tol_x, tol_w, tol_loss, w0_factor=5.0, **kw)


def cf_check(m, params, t, q0, dev, tol_x, tol_w, **kw):
    """waveform discriminator: loss values at 5e-5"""
    return two_part_check("wave", m, params, t, q0, dev, tol_x, tol_w, 5e-5, **kw)


def pd_check(m, params, t, q0, dev, **kw):
    """pitch / duration discriminator: d_pred and gradients at 2e-4, original0 at 1e-3, loss values at 2e-5"""
    return two_part_check("seq", m, params, t, q0, dev, 2e-5, 2e-4, 2e-5, w0_factor=5.0, **kw)
