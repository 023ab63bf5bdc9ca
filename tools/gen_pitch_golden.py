"""Golden fixtures of the pitch command by RUNNING THE REFERENCE (build container only): its RMVPE network class E2E0
(train/dataprep/rmvpe/model.py:49-86) and its decode `to_local_average_f0` (rmvpe/utils.py:114-131).

    python tools/gen_pitch_golden.py

The reference's `rmvpe` package is imported directly (its directory goes on sys.path, so that nothing of the training package
around it is pulled in) behind stub `librosa` / `torchaudio` modules, SURVEY.md 8(c): neither is installed, and neither is
reached by what runs here (spec.py's mel basis and inference.py's Resample are only touched by the RMVPE wrapper class, which
is not instantiated).  Only data is written; weights are never committed: both sides regenerate them from the key-named fill
(tests/pitch_cases.rmvpe_weights).

  tests/golden/manifest_rmvpe.json                 key -> shape of E2E0's state_dict, {"full": ..., "small": ...}
  tests/golden/pitch_small.json                    seeds, configurations, the measured numbers printed below
  tests/golden/pitch_small.safetensors             the decode cases with the reference's fp32 and float64 f0; the chained
                                                   check's float64 f0 and top-2 margins (n = 64, both configurations)
  tests/golden/pitch_{small,full}_n{n}.safetensors the network: input [2, 128, n], the reference's salience in fp32 and,
                                                   from a .double() copy, in float64 -- one file per case (size limit)
"""
import importlib.machinery
import json
import os
import sys
import types

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
REF_DATAPREP = "/root/reference/src/stylish_tts/train/dataprep"
EXCLUDED_CAP = 0.10


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def import_reference():
    lib = _stub("librosa")
    lib.filters = _stub("librosa.filters", mel=None)
    lib.sequence = _stub("librosa.sequence", viterbi=None)
    ta = _stub("torchaudio")
    ta.transforms = _stub("torchaudio.transforms", Resample=object)
    sys.path.insert(0, REF_DATAPREP)
    import rmvpe
    return rmvpe


def reference_model(R, PC, cfg):
    m = R.E2E0(cfg["n_blocks"], 1, (2, 2), 5, cfg["inter_layers"], 1, cfg["en_out_channels"])
    miss, unexp = m.load_state_dict(PC.rmvpe_weights(cfg), strict=True)
    assert not miss and not unexp
    return m.eval()


def mel2hidden(model, mel):
    """RMVPE.mel2hidden (inference.py:29-36) without the wrapper class"""
    n = mel.shape[-1]
    with torch.no_grad():
        mel = torch.nn.functional.pad(mel, (0, 32 * ((n - 1) // 32 + 1) - n), mode="reflect")
        return model(mel)[:, :n]


def main():
    from tests import pitch_cases as PC
    torch.set_num_threads(8)
    R = import_reference()
    assert (R.N_CLASS, R.N_MELS, R.CONST) == (PC.N_CLASS, PC.N_MELS, PC.CONST)
    meta = {"seed": PC.SEED, "small": PC.SMALL, "full": PC.FULL, "net": {}, "chain": {}}
    manifest = {}
    for name, cfg in (("full", PC.FULL), ("small", PC.SMALL)):
        model = reference_model(R, PC, cfg)
        sd = model.state_dict()
        manifest[name] = {k: list(v.shape) for k, v in sd.items()}
        params = sum(p.numel() for p in model.parameters())
        print(f"{name}: {len(sd)} keys, {params:,} parameters")
        meta[name + "_parameters"] = params
        double = reference_model(R, PC, cfg).double()
        for n in (PC.NET_FRAMES if name == "small" else (61,)):
            x = PC.net_input(n)
            s32, s64 = mel2hidden(model, x), mel2hidden(double, x.double())
            gate, scale, own = PC.forward_gate(s64, s32)
            meta["net"][f"{name}_n{n}"] = dict(max_ref=scale, ref_f32_to_f64=own, gate=gate)
            print(f"  salience {name} n={n}: max|ref| {scale:.4f}  reference fp32-to-f64 {own:.3e}  gate {gate:.3e}")
            path = os.path.join(OUT, f"pitch_{name}_n{n}.safetensors")
            save_file({"input": x.contiguous(), "salience_f32": s32.contiguous(), "salience_f64": s64.contiguous()}, path)
            assert os.path.getsize(path) < 1 << 20, path
            if n == 33:  # the negative control of the device test must be visible to the gate: zero padding instead of reflection
                with torch.no_grad():
                    z = double(torch.nn.functional.pad(x.double(), (0, 31)))[:, :n]
                meta["net"][f"{name}_n{n}"]["zero_pad_distance"] = (z - s64).abs().max().item()
                print(f"    zero-padded instead of reflected: {meta['net'][f'{name}_n{n}']['zero_pad_distance']:.3e}")
                assert meta["net"][f"{name}_n{n}"]["zero_pad_distance"] > gate
        # the chained check: f0 of the float64 salience at n = 64, and every frame's top-2 margin
        x = PC.net_input(64)
        s32, s64 = mel2hidden(model, x), mel2hidden(double, x.double())
        gate, scale, own = PC.forward_gate(s64, s32)
        top2 = s64.topk(2, dim=2)[0]
        margin = top2[..., 0] - top2[..., 1]
        f64 = torch.from_numpy(R.to_local_average_f0(s64)).double()
        f32 = torch.from_numpy(R.to_local_average_f0(s32)).double()
        out_of = (margin <= 2 * gate).double().mean().item()
        own_share = ((f32 - f64).abs() > 1e-5 * f64.abs().max()).double().mean().item()
        print(f"  chain {name} n=64: salience gate {gate:.3e} (own {own:.3e})  minimum margin {margin.min().item():.3e}  "
              f"frames left out {100 * out_of:.1f} %  voiced {(f64 > 0).double().mean().item():.2f}  "
              f"reference fp32 f0 beyond 1e-5 max {100 * own_share:.1f} %")
        assert out_of <= EXCLUDED_CAP, "change the seed, never the cap"
        meta["chain"][name] = dict(salience_gate=gate, min_margin=margin.min().item(), left_out=out_of,
                                   f0_ref_f32_to_f64=(f32 - f64).abs().max().item())
        manifest_out = {f"chain.{name}.f0_f64": f64.contiguous(), f"chain.{name}.margin_f64": margin.contiguous(),
                        f"chain.{name}.f0_f32": f32.float().contiguous()}
        meta.setdefault("_tensors", {}).update(manifest_out)
    with open(os.path.join(OUT, "manifest_rmvpe.json"), "w") as f:
        json.dump(manifest, f, indent=0)
    out = meta.pop("_tensors")
    # ---- decode: the reference function on the hand-made rows, fp32 and float64 ------------------------------------------
    cases = PC.decode_cases()
    rows = torch.stack(list(cases.values()))[None]  # [1, R, 360]
    out["decode.rows"] = rows[0].contiguous()
    out["decode.f0_f32"] = torch.from_numpy(R.to_local_average_f0(rows)).reshape(-1).float().contiguous()
    out["decode.f0_f64"] = torch.from_numpy(R.to_local_average_f0(rows.double())).reshape(-1).double().contiguous()
    meta["decode_cases"] = list(cases)
    for i, k in enumerate(cases):
        print(f"  decode {k}: reference f0 fp32 {out['decode.f0_f32'][i].item():.6f}  float64 {out['decode.f0_f64'][i].item():.9f}  "
              f"restatement {PC.decode(rows[0, i]).item():.9f}")
    path = os.path.join(OUT, "pitch_small.safetensors")
    save_file(out, path)
    with open(os.path.join(OUT, "pitch_small.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("size KB", os.path.getsize(path) // 1024)


if __name__ == "__main__":
    main()
