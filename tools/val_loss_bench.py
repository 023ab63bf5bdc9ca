"""sty_mel_loss_fwd (the validation pass's forward-only mel term) against sty_acoustic_loss_fwd_bwd (the training entry, which also
builds the phase tensors and runs three STFT backward chains) at the c3 shape, B = 32 x 6.5 s: ms per call from device events around
blocks of calls, the two entries alternating block by block so that both see the same machine.  python tools/val_loss_bench.py
(profiles/validate_pass.txt)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stylish_tts_amd.losses import acoustic_loss, mel_loss

DEV = "cuda:0"
B, T = 32, 520  # bench.py WORKLOADS["c3"]
N = 300 * T
BLOCK, ROUNDS = 20, 15


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    g = torch.Generator().manual_seed(3)
    gt = (0.3 * torch.randn(B, N, generator=g)).to(DEV)
    pr = (0.3 * torch.randn(B, N, generator=g)).to(DEV)
    entries = {"sty_mel_loss_fwd": lambda: mel_loss(gt, pr, per_item=True),
               "sty_acoustic_loss_fwd_bwd": lambda: acoustic_loss(gt, pr)}
    for fn in entries.values():  # warm-up: code objects, front-end tables, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    a, b = mel_loss(gt, pr), acoustic_loss(gt, pr)[0][0]
    torch.cuda.synchronize()
    print(f"shape B={B} N={N}: mel {a.item():.9g} (forward only) vs {b.item():.9g} (training entry)")
    ms = {k: [] for k in entries}
    for _ in range(ROUNDS):
        for k, fn in entries.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BLOCK):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / BLOCK)
    for k, v in ms.items():
        print(f"{k:28s} median {statistics.median(v):.3f} ms per call  (min {min(v):.3f}, max {max(v):.3f}, {ROUNDS} blocks of {BLOCK})")


if __name__ == "__main__":
    main()
