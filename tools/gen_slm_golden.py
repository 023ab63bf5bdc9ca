"""Fixtures of the slm tests: runs of transformers' own WavLMModel on the CPU, on key-filled weights.

    python tools/gen_slm_golden.py            (needs the transformers package; no GPU, no network)

For every case of tests/slm_cases.py: WavLMModel(WavLMConfig(**cfg)).eval() with the key-filled weights (masked_spec_embed zero),
run in float64 and in fp32 on the case's seeded wave with output_hidden_states=True.  Stored:

  tests/golden/slm_small.safetensors, slm_full2.safetensors, slm_full12_a / _b.safetensors (each under 1 MiB)
      <case>.h<i>   float64 hidden state i [B, T, H] (all of them for the small cases, 0 / 6 / 12 at full depth)
      <case>.max    max |ref64| over ALL hidden states
      <case>.own    max |fp32 run - float64 run| over ALL hidden states
      <case>.loss   float64 mean |h(wave 0) - h(wave 1)| over the stack of all hidden states (WavLMLoss's value at 16 kHz)
  tests/golden/slm_small.json
      the case list and the class's own _relative_positions_bucket tables
  tests/golden/manifest_wavlm.json
      key -> shape of the class at its default config, without masked_spec_embed

Weights are regenerated from keys on both sides, as for the pitch fixtures; only seeds and outputs are stored.  The negative
controls (the reference alone, float64) are printed; profiles/slm_parity_table.txt keeps them.
"""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import slm_cases as SC  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def build(cfg, dtype):
    from transformers import WavLMConfig, WavLMModel
    model = WavLMModel(WavLMConfig(**cfg)).eval()
    state = dict(SC.wavlm_weights(cfg))
    state["masked_spec_embed"] = torch.zeros(model.config.hidden_size)
    model.load_state_dict(state, strict=True)
    return model.to(dtype)


@torch.no_grad()
def hidden(model, x):
    return torch.stack(model(x.to(next(model.parameters()).dtype), output_hidden_states=True).hidden_states)  # [L + 1, B, T, H]


def main():
    from safetensors.torch import save_file
    from transformers import WavLMConfig, WavLMModel
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    torch.manual_seed(0)
    files = {"slm_small": {}, "slm_full2": {}, "slm_full12_a": {}, "slm_full12_b": {}}
    listing, models = {}, {}
    for name, (cname, n16, B, T, keep) in SC.CASES.items():
        cfg = SC.CONFIGS[cname]
        if cname not in models:
            models[cname] = (build(cfg, torch.float64), build(cfg, torch.float32))
        m64, m32 = models[cname]
        x0, x1 = SC.wave(n16, B, 0), SC.wave(n16, B, 1)
        h64, h32 = hidden(m64, x0), hidden(m32, x0)
        assert h64.shape[2] == T == SC.frames(n16, cfg), (name, h64.shape)
        loss = (h64 - hidden(m64, x1)).abs().mean()
        own = (h32.double() - h64).abs().max()
        print(f"{name}: T {T}  max|ref64| {h64.abs().max():.4f}  fp32-to-f64 {own:.3e}  loss {loss:.6f}")
        for i in keep:
            f = "slm_small" if cname == "small" else "slm_full2" if cname == "full2" else ("slm_full12_a" if i < 12 else "slm_full12_b")
            files[f][f"{name}.h{i}"] = h64[i].contiguous()
        f = "slm_small" if cname == "small" else "slm_full2" if cname == "full2" else "slm_full12_b"
        files[f][f"{name}.max"] = h64.abs().max().reshape(1)
        files[f][f"{name}.own"] = own.reshape(1)
        files[f][f"{name}.loss"] = loss.reshape(1)
        listing[name] = dict(config=cname, n16=n16, B=B, T=T, states=list(keep))
        # ---- negative controls of the reference alone (float64) ----
        if name in ("small_22800", "full2_8000"):
            sd = {k: v.clone() for k, v in m64.state_dict().items()}  # (state_dict() hands out the live tensors)
            ones = {k: torch.ones_like(v) for k, v in sd.items() if k.endswith("gru_rel_pos_const")}
            m64.load_state_dict({**sd, **ones})
            print(f"  control {name}: gru_rel_pos_const set to 1: {(hidden(m64, x0) - h64).abs().max():.3e}")
            zero = {k: torch.zeros_like(v) for k, v in sd.items() if k.endswith("rel_attn_embed.weight")}
            m64.load_state_dict({**sd, **zero})
            print(f"  control {name}: position bias removed: {(hidden(m64, x0) - h64).abs().max():.3e}")
            m64.load_state_dict(sd)
        if name == "small_22800":
            orig = WavLMAttention._relative_positions_bucket

            def unclamped(self, rel):  # the class's function without its torch.min (kept inside the embedding's rows)
                nb = self.num_buckets // 2
                out = (rel > 0).to(torch.long) * nb
                rel = torch.abs(rel)
                max_exact = nb // 2
                large = torch.log(rel.float() / max_exact) / math.log(self.max_distance / max_exact) * (nb - max_exact)
                large = (max_exact + large).to(torch.long)
                return (out + torch.where(rel < max_exact, rel, large)).clamp(0, self.num_buckets - 1)

            WavLMAttention._relative_positions_bucket = unclamped
            print(f"  control {name}: bucket clamp removed: {(hidden(m64, x0) - h64).abs().max():.3e}")
            WavLMAttention._relative_positions_bucket = orig
    for f, tensors in files.items():
        path = os.path.join(GOLDEN, f + ".safetensors")
        save_file(tensors, path)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    tables = {}
    for T, nb, md in SC.BUCKET_TABLES:
        att = WavLMAttention(64, 4, num_buckets=nb, max_distance=md)
        rel = torch.arange(-(T - 1), T, dtype=torch.long)[None, :]
        tables[f"{T}_{nb}_{md}"] = att._relative_positions_bucket(rel)[0].tolist()
    with open(os.path.join(GOLDEN, "slm_small.json"), "w") as fh:
        json.dump(dict(seed=SC.SEED, cases=listing, bucket_tables=tables), fh, separators=(",", ":"))
    sd = WavLMModel(WavLMConfig()).state_dict()
    sd.pop("masked_spec_embed")
    with open(os.path.join(GOLDEN, "manifest_wavlm.json"), "w") as fh:
        json.dump({k: list(v.shape) for k, v in sd.items()}, fh, indent=0)
    print(f"manifest: {len(sd)} keys, {sum(v.numel() for v in sd.values()):,} parameters")


if __name__ == "__main__":
    main()
