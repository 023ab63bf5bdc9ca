"""Fixtures of the slm gradient tests: autograd of transformers' own WavLMModel on the CPU, on key-filled weights.

    python tools/gen_slm_grad_golden.py            (needs the transformers package; no GPU, no network)

The float64 and fp32 models are built as tools/gen_slm_golden.py builds them, on the waves of tests/slm_cases.py.  Stored per
case (tests/slm_grad_cases.py says which), each file under 1 MiB:

  tests/golden/slm_grad_*.safetensors
      <case>.g_cot     float64 d/d wave1 of sum(h(wave1) * cot) / numel, cot = slm_grad_cases.cot(case) (never stored)
      <case>.e_cot     the same gradient at the encoder's input, [B, H, T] (the feature projection's output)
      <case>.g_l1      float64 d/d wave1 of mean |h(wave0) - h(wave1)|
      <case>.sign      the float64 run's sign(h1 - h0), bit-packed (no exact tie: asserted)
      <grad>.gmax / .gown   max |g64| and max |g32 - g64| of each gradient: the two inputs of its gate
      <case>.mindiff   min |h0 - h1| over the stack
      e2e_<N>.g / .g.gmax / .g.gown / .loss / .mindiff / .fgate
                       at 24 kHz: SC.resample in float64 composed with the float64 small model, autograd through both
  tests/golden/slm_grad.json
      the listing

The reference-alone lines are printed; profiles/slm_grad_table.txt keeps them.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import slm_cases as SC  # noqa: E402
from tests import slm_grad_cases as GC  # noqa: E402
from gen_slm_golden import build  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def run(model, x, want_tap=False):
    """(stack [L + 1, B, T, H] with its graph, the feature projection's output if asked)"""
    tap = []
    hook = model.feature_projection.register_forward_hook(lambda mod, inp, out: tap.append(out[0])) if want_tap else None
    h = torch.stack(model(x, output_hidden_states=True).hidden_states)
    if hook:
        hook.remove()
    return h, (tap[0] if want_tap else None)


def grads(model, name, dtype):
    """the case's gradients of one model: dict of tensors, plus the stacks' difference"""
    cname, n16, B, T, _ = SC.CASES[name]
    want = GC.CASES[name][1]
    x0 = SC.wave(n16, B, 0).to(dtype)
    x1 = SC.wave(n16, B, 1).to(dtype).requires_grad_(True)
    out = {}
    h1, tap = run(model, x1, "e_cot" in want)
    assert tuple(h1.shape) == GC.stack_shape(name), (name, h1.shape)
    obj = (h1 * GC.cot(name, dtype)).sum() / h1.numel()
    gs = torch.autograd.grad(obj, [x1] + ([tap] if tap is not None else []), retain_graph="g_l1" in want)
    out["g_cot"] = gs[0].detach()
    if tap is not None:
        out["e_cot"] = gs[1].detach().transpose(1, 2).contiguous()  # [B, T, H] -> [B, H, T]
    diff = None
    if "g_l1" in want:
        with torch.no_grad():
            h0, _ = run(model, x0)
        out["g_l1"] = torch.autograd.grad((h0 - h1).abs().mean(), x1)[0].detach()
        diff = (h1 - h0).detach()
    return out, diff


def main():
    from safetensors.torch import load_file, save_file
    torch.manual_seed(0)
    fwd = {}
    for f in ("slm_small", "slm_full2", "slm_full12_a", "slm_full12_b"):
        fwd.update(load_file(os.path.join(GOLDEN, f + ".safetensors")))
    files = {f: {} for f in GC.FILES}
    listing, models = {}, {}
    for name, (fname, want) in GC.CASES.items():
        cname, n16, B, T, _ = SC.CASES[name]
        if cname not in models:
            models[cname] = (build(SC.CONFIGS[cname], torch.float64), build(SC.CONFIGS[cname], torch.float32))
        g64, diff = grads(models[cname][0], name, torch.float64)
        g32, _ = grads(models[cname][1], name, torch.float32)
        line = f"slm_grad reference {name}: T {T}"
        for k in want:
            gmax, gown = g64[k].abs().max(), (g32[k].double() - g64[k]).abs().max()
            rel = ((g32[k].double() - g64[k]).norm() / g64[k].norm()).item()
            files[fname][f"{name}.{k}"] = g64[k].contiguous()
            files[fname][f"{name}.{k}.gmax"] = gmax.reshape(1)
            files[fname][f"{name}.{k}.gown"] = gown.reshape(1)
            line += f"  {k}: max|g64| {gmax:.4e} fp32-to-f64 {gown:.3e} (rel L2 {rel:.2e}) gate {GC.grad_gate(gmax.item(), gown.item()):.3e}"
        if diff is not None:
            assert (diff != 0).all(), f"{name}: an exact tie in the float64 stacks"
            mind = diff.abs().min()
            files[fname][f"{name}.sign"] = GC.pack_signs(torch.sign(diff))
            files[fname][f"{name}.mindiff"] = mind.reshape(1)
            fgate = SC.forward_gate(fwd[name + ".max"].item(), fwd[name + ".own"].item())
            line += f"  min|h0 - h1| {mind:.3e} (2 x forward gate {2 * fgate:.3e})"
            if name in GC.OWN_SIGN_CASES:
                assert mind.item() > 2 * fgate, (name, mind.item(), fgate)
            assert torch.equal(GC.unpack_signs(files[fname][f"{name}.sign"], diff.shape, torch.float64), torch.sign(diff))
        if n16 == 7777:
            assert (g64["g_cot"][:, -2:] == 0).all() and (g64["g_cot"][:, -3] != 0).all()
        print(line)
        listing[name] = dict(file=fname, grads=list(want), n16=n16, B=B, T=T)
    # ---- end to end at 24 kHz ----
    m64, m32 = models[GC.E2E_CONFIG]
    e2e = {}
    for N in GC.E2E_N:
        gt, pred = GC.e2e_waves(N)
        res = {}
        for model, dtype in ((m64, torch.float64), (m32, torch.float32)):
            y = pred.to(dtype).requires_grad_(True)
            with torch.no_grad():
                h0, _ = run(model, SC.resample(gt, dtype=dtype))
            h1, _ = run(model, SC.resample(y, dtype=dtype))
            loss = (h0 - h1).abs().mean()
            res[dtype] = (torch.autograd.grad(loss, y)[0].detach(), loss.detach(), (h1 - h0).detach(), h1.detach())
        g, loss, diff, h1 = res[torch.float64]
        gown = (res[torch.float32][0].double() - g).abs().max()
        fgate = SC.forward_gate(h1.abs().max().item(), (res[torch.float32][3].double() - h1).abs().max().item())
        assert (diff != 0).all() and diff.abs().min().item() > 2 * fgate, (N, diff.abs().min().item(), fgate)
        t = files["slm_grad_e2e"]
        t[f"e2e_{N}.g"], t[f"e2e_{N}.g.gmax"], t[f"e2e_{N}.g.gown"] = g.contiguous(), g.abs().max().reshape(1), gown.reshape(1)
        t[f"e2e_{N}.loss"], t[f"e2e_{N}.mindiff"] = loss.reshape(1), diff.abs().min().reshape(1)
        t[f"e2e_{N}.fgate"] = torch.tensor([fgate], dtype=torch.float64)
        print(f"slm_grad reference e2e_{N}: T {h1.shape[2]}  max|g64| {g.abs().max():.4e} fp32-to-f64 {gown:.3e} "
              f"gate {GC.grad_gate(g.abs().max().item(), gown.item()):.3e}  loss {loss:.6f}  min|h0 - h1| {diff.abs().min():.3e} "
              f"(2 x forward gate {2 * fgate:.3e})")
        e2e[str(N)] = dict(B=2, T=int(h1.shape[2]), config=GC.E2E_CONFIG)
    for f, tensors in files.items():
        path = os.path.join(GOLDEN, f + ".safetensors")
        save_file(tensors, path)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    with open(os.path.join(GOLDEN, "slm_grad.json"), "w") as fh:
        json.dump(dict(seed=SC.SEED, cases=listing, e2e=e2e, files=list(GC.FILES)), fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
