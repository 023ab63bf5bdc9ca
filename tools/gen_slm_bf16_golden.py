"""Fixtures of the bf16 operand mode of the slm term: how far the reference's own bf16 mode is from float64.

    python tools/gen_slm_bf16_golden.py            (needs the transformers package; no GPU, no network)

For every case of tests/slm_bf16_cases.py: transformers' WavLMModel on key-filled weights (as tools/gen_slm_golden.py builds it), run
in float64 and again in fp32 under torch.autocast("cpu", dtype=torch.bfloat16) -- autocast is the reference's bf16 mode
(train/train_context.py:94-104) -- on the case's seeded waves.  Stored in tests/golden/slm_bf16.json, per case:

  r_auto.h<i>, r_auto.stack   || autocast - float64 || / || float64 || of every stored hidden state (wave 0) and of the whole stack
  r_auto.g_cot                the same ratio for d/d wave1 of sum(h(wave1) * cot) / numel under autocast autograd
  r_emul.h<i>, r_emul.stack   the same ratio for the float64 model with the two operands of every Conv1d / Linear module but layer
                              0's conv and the gate's Linear rounded to bf16 (forward hooks): rounding operands only, as the device
                              mode does.  (q / k / v run through a functional call inside the class's attention: their weights
                              are rounded, their input is not.  A figure for orientation, printed by the tests, gating nothing.)
  rms.stack                   root mean square of the float64 stack
  loss, loss_auto             float64 mean |h(wave 0) - h(wave 1)| and the same value under autocast

and, for the two cases the older fixtures do not hold, in tests/golden/slm_bf16_*.safetensors (each under 1 MiB):

  <case>.h<i>     the float64 hidden state as float32 on every `frame stride`-th frame
  <case>.g_cot    the float64 gradient as float32 on every `sample stride`-th sample

The ratios of a case are taken on the stored frames / samples, so that the device is compared on exactly what the reference was.
The controls (the float64 reference alone: what a relative L2 gate of this size can and cannot see) are printed;
profiles/slm_bf16_parity_table.txt keeps them.
"""
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import slm_bf16_cases as BC  # noqa: E402
from tests import slm_cases as SC  # noqa: E402
from gen_slm_golden import build  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def run(model, x, cot=None, autocast=False):
    """(stack [L + 1, B, T, H] detached, d/dx of sum(stack * cot) / numel if cot is given)"""
    x = x.clone().requires_grad_(cot is not None)
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if autocast else contextlib.nullcontext()
    with ctx, (contextlib.nullcontext() if cot is not None else torch.no_grad()):
        h = torch.stack([s.float() if autocast else s for s in model(x, output_hidden_states=True).hidden_states])
    g = None
    if cot is not None:
        g = torch.autograd.grad((h.double() * cot).sum() / h.numel(), x)[0].detach()
    return h.detach(), g


def emulated(cfg):
    """the float64 model with bf16-rounded operands on its Conv1d / Linear modules (see the module docstring)"""
    m = build(cfg, torch.float64)
    rnd = lambda t: t.bfloat16().double()
    skip = {"feature_extractor.conv_layers.0.conv"}
    for name, mod in m.named_modules():
        if not isinstance(mod, (torch.nn.Conv1d, torch.nn.Linear)) or name in skip or name.endswith("gru_rel_pos_linear"):
            continue
        if "weight" in mod._parameters:  # (the positional conv's weight is a parametrization: its input alone is rounded)
            with torch.no_grad():
                mod.weight.copy_(rnd(mod.weight))
        mod.register_forward_pre_hook(lambda _m, inp: (rnd(inp[0]),) + tuple(inp[1:]))
    return m


def controls(name, m64, x0, h64):
    last = h64.shape[0] - 1
    sd = {k: v.clone() for k, v in m64.state_dict().items()}
    out = {}
    zero = {k: torch.zeros_like(v) for k, v in sd.items() if k.endswith("rel_attn_embed.weight")}
    m64.load_state_dict({**sd, **zero})
    out["position bias removed"] = BC.rel_l2(run(m64, x0)[0][last], h64[last])
    ones = {k: torch.ones_like(v) for k, v in sd.items() if k.endswith("gru_rel_pos_const")}
    m64.load_state_dict({**sd, **ones})
    out["gru_rel_pos_const = 1"] = BC.rel_l2(run(m64, x0)[0][last], h64[last])
    key = "feature_extractor.conv_layers.2.conv.weight"
    m64.load_state_dict({**sd, key: sd[key] * (1 + 2.0 ** -6)})
    out["conv 2 weight x (1 + 2^-6)"] = BC.rel_l2(run(m64, x0)[0][last], h64[last])
    m64.load_state_dict(sd)
    print(f"  control {name} (last state, relative L2 to float64): " + ", ".join(f"{k}: {v:.2e}" for k, v in out.items()))


def main():
    from safetensors.torch import save_file
    torch.manual_seed(0)
    models, listing = {}, {}
    files = {f: {} for fs in BC.NEW_FILES.values() for f in fs}
    for name, (cname, n16, B, T, keep, fstride, sstride) in BC.CASES.items():
        cfg = SC.CONFIGS[cname]
        if cname not in models:
            models[cname] = (build(cfg, torch.float64), build(cfg, torch.float32), emulated(cfg))
        m64, m32, mem = models[cname]
        x0, x1, cot = SC.wave(n16, B, 0), SC.wave(n16, B, 1), BC.cot(name)
        h64, _ = run(m64, x0.double())
        assert h64.shape[2] == T == SC.frames(n16, cfg), (name, h64.shape)
        h64b, g64 = run(m64, x1.double(), cot)
        ha, _ = run(m32, x0, autocast=True)
        hab, ga = run(m32, x1, cot, autocast=True)
        he, _ = run(mem, x0.double())
        sub = lambda h: h[:, :, ::fstride]
        rec = dict(config=cname, n16=n16, B=B, T=T, states=list(keep), frame_stride=fstride, sample_stride=sstride)
        for i in keep:
            rec[f"r_auto.h{i}"] = BC.rel_l2(sub(ha)[i], sub(h64)[i])
            rec[f"r_emul.h{i}"] = BC.rel_l2(sub(he)[i], sub(h64)[i])
        rec["r_auto.stack"], rec["r_emul.stack"] = BC.rel_l2(sub(ha), sub(h64)), BC.rel_l2(sub(he), sub(h64))
        rec["r_auto.g_cot"] = BC.rel_l2(ga[:, ::sstride], g64[:, ::sstride])
        rec["rms.stack"] = h64.pow(2).mean().sqrt().item()
        rec["loss"] = (h64 - h64b).abs().mean().item()
        rec["loss_auto"] = (ha.double() - hab.double()).abs().mean().item()
        listing[name] = rec
        print(f"slm_bf16 reference {name}: T {T}  r_auto states " + " / ".join(f"{rec[f'r_auto.h{i}']:.2e}" for i in keep)
              + f"  stack {rec['r_auto.stack']:.2e}  g_cot {rec['r_auto.g_cot']:.2e}  operand-rounding emulation "
              + " / ".join(f"{rec[f'r_emul.h{i}']:.2e}" for i in keep)
              + f"  rms {rec['rms.stack']:.4f}  loss {rec['loss']:.6f} autocast {rec['loss_auto']:.6f} "
              f"(rel {abs(rec['loss_auto'] - rec['loss']) / rec['loss']:.1e})")
        if name in BC.NEW_CASES:
            fs = BC.NEW_FILES[name]
            for i in keep:
                files[fs[0]][f"{name}.h{i}"] = h64[i, :, ::fstride].float().contiguous()
            files[fs[-1]][f"{name}.g_cot"] = g64[:, ::sstride].float().contiguous()
        if name in ("small_22800", "full2_8000", "full2_41700"):
            controls(name, m64, x0.double(), h64)
    for f, tensors in files.items():
        path = os.path.join(GOLDEN, f + ".safetensors")
        save_file(tensors, path)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    with open(os.path.join(GOLDEN, BC.LISTING), "w") as fh:
        json.dump(dict(seed=SC.SEED, cases=listing), fh, indent=0)


if __name__ == "__main__":
    main()
