"""A/B record of the fp32 split mode (bf16x3) of the persistent 32-channel conv: writes profiles/fp32_split_table.txt.

    python tools/fp32_split_ab.py [--parent-dir DIR] [--out profiles/fp32_split_table.txt]

Run on the GPU box from the repository root, library built.  The driver starts every GPU step as a child process of its own
under a time limit and stops at the first one that fails or runs out of time:
  shapes   every conv32p shape of the c5 forward (K 7 / 11 / 21, dilation 1 / 3 / 5, B = 8, T = 60 000): us per launch of the
           fp32 kernel and of the split kernel (the library's profiler, one launch per sample: 5 warm-up, 20 timed, median and
           min-max) and max abs error of both against float64 on the same unrounded operands (batch rows 0 and 7)
  forward  the c5 vocoder forward (bench.WORKLOADS["c5"], bench.make_inputs): ms in fp32, split and bf16 (events around each
           of 20 forwards behind 5 warm-up, median and min-max), and the split audio against the fp32 audio on the same inputs
           and the same prior_override (the prior of the fp32 run)
  bench    three runs each of `python bench.py --workload c5` and `--workload c5-bf16` in this tree, and in --parent-dir (a built
           checkout of the parent commit) where given
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(8, 32, 32, 7, 1, 60000), (8, 32, 32, 11, 1, 60000), (8, 32, 32, 11, 3, 60000), (8, 32, 32, 11, 5, 60000),
          (8, 32, 32, 21, 1, 60000)]
WARMUP, TIMED = 5, 20


def _stats(v):
    return dict(median=statistics.median(v), lo=min(v), hi=max(v), n=len(v))


def step_shapes():
    import torch
    from stylish_tts_amd import lib as L
    lib = L.load()
    dev = "cuda:0"
    rows = []
    for shape in SHAPES:
        B, Ci, Co, K, d, T = shape
        g = torch.Generator().manual_seed(sum(shape))
        x, w, b = torch.randn(B, Ci, T, generator=g), torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5, torch.randn(Co, generator=g)
        sub = [0, B - 1]
        ref = torch.nn.functional.conv1d(x[sub].double(), w.double(), b.double(), padding=(K - 1) * d // 2, dilation=d)
        xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
        y = torch.empty(B, Co, T, device=dev)
        need = C.c_size_t()
        L.check(lib.sty_conv1d_workspace_bytes(Co, Ci, K, C.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        row = dict(shape=shape)
        for mode, name in ((0, "conv32p_kernel<false>"), (4, "conv32p_kernel<split>")):
            us = []
            for i in range(WARMUP + TIMED):
                L.prof_report(64)
                lib.sty_prof_enable(1)
                try:
                    L.check(lib.sty_conv1d_fwd(B, Ci, Co, K, d, T, L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(y), L.ptr(ws), ws.numel(),
                                               mode, None))
                    torch.cuda.synchronize()
                finally:
                    lib.sty_prof_enable(0)
                mine = [r for r in L.prof_report(64) if r["name"] == name]
                if len(mine) != 1 or mine[0]["launches"] != 1:
                    raise SystemExit(f"{shape} mode {mode}: expected one launch of {name}, saw {mine}")
                if i >= WARMUP:
                    us.append(1e3 * mine[0]["ms"])
            row["fp32" if mode == 0 else "split"] = dict(us=_stats(us), err=(y[sub].cpu().double() - ref).abs().max().item())
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_forward():
    import torch
    import bench
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["c5"]
    model, _, _ = bench.build_model(dev)
    inp = bench.make_inputs(w, 0, dev)
    B, T = w["B"], w["T"]
    args = dict(mel=inp["mel"], style=inp["style"], pitch=inp["pitch"], voiced=inp["voiced"])

    def timed():
        ms = []
        for i in range(WARMUP + TIMED):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.no_grad():
                model.vocoder_forward(seed=i, **args)
            e1.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms.append(e0.elapsed_time(e1))
        return _stats(ms)

    out = {}
    prior = torch.zeros(B, 300 * T, device=dev)
    with torch.no_grad():
        model.vocoder_forward(seed=0, taps=dict(tap_prior=prior), **args)
        a_fp32 = model.vocoder_forward(seed=0, prior_override=prior, **args).audio.double().cpu()
    out["fp32"] = timed()
    model.set_fp32_split(True)
    with torch.no_grad():
        a_split = model.vocoder_forward(seed=0, prior_override=prior, **args).audio.double().cpu()
    out["split"] = timed()
    model.set_fp32_split(False)
    model.set_train_opts(compute_bf16=True)
    out["bf16"] = timed()
    diff = a_split - a_fp32
    out["audio"] = dict(mse=(diff ** 2).mean().item(), max_abs=diff.abs().max().item(), power=(a_fp32 ** 2).mean().item())
    print(json.dumps(out), flush=True)
    return out


def _child(cmd, limit, cwd=ROOT):
    """one GPU step: a fresh process under its own time limit; its last JSON line"""
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} (in {cwd}) ended with {r.returncode}; nothing further is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return [json.loads(ln) for ln in lines]


def _fmt(s, unit):
    return f"{s['median']:8.2f} {unit} (min {s['lo']:.2f}, max {s['hi']:.2f}, n {s['n']})"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=["shapes", "forward"], default=None, help="(internal) run one GPU step in this process")
    ap.add_argument("--parent-dir", default=None, help="a built checkout of the parent commit for the bench.py comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp32_split_table.txt"))
    ap.add_argument("--bench-runs", type=int, default=3)
    a = ap.parse_args()
    if a.step == "shapes":
        return step_shapes()
    if a.step == "forward":
        return step_forward()
    me = [sys.executable, os.path.abspath(__file__)]
    T = []
    rows = _child(me + ["--step", "shapes"], 400)
    T.append("fp32 split mode (bf16x3) of the persistent 32-channel conv -- tools/fp32_split_ab.py")
    T.append("")
    T.append(f"1. conv32p shapes of the c5 forward, B = 8, T = 60 000, plain conv + bias (sty_conv1d_fwd, compute mode 0 against 4);")
    T.append(f"   kernel time from the library's profiler, one launch per sample, {WARMUP} warm-up, {TIMED} timed; error: max abs against float64")
    T.append("   on the same unrounded operands, batch rows 0 and 7")
    T.append("   K  dil   fp32 kernel us (median, min-max)          split kernel us (median, min-max)         split/fp32  err fp32   err split  eligible")
    for r in rows:
        _, _, _, K, d, _ = r["shape"]
        f, s = r["fp32"], r["split"]
        ratio = s["us"]["median"] / f["us"]["median"]
        T.append(f"  {K:2d}  {d:2d}   {_fmt(f['us'], 'us'):42s}  {_fmt(s['us'], 'us'):42s}  {ratio:6.3f}    {f['err']:.2e}   {s['err']:.2e}  "
                 f"{'yes' if ratio < 1 else 'NO: to be excluded in conv32p_split_eligible'}")
    fw = _child(me + ["--step", "forward"], 400)[-1]
    T.append("")
    T.append(f"2. c5 vocoder forward (bench.WORKLOADS['c5'], bench.make_inputs(seed 0)), events around each forward, {WARMUP} warm-up, {TIMED} timed")
    for k in ("fp32", "split", "bf16"):
        T.append(f"   {k:6s} {_fmt(fw[k], 'ms')}")
    au = fw["audio"]
    T.append(f"   split audio against fp32 audio, same inputs and prior_override: mse {au['mse']:.3e} (gate 1e-8; signal power {au['power']:.3e}), "
             f"max abs {au['max_abs']:.3e}")
    T.append("")
    T.append(f"3. bench.py, {a.bench_runs} runs each, ms_per_step")
    for label, cwd in (("parent", a.parent_dir), ("this tree", ROOT)):
        if not cwd:
            T.append(f"   {label}: not measured (no --parent-dir)")
            continue
        for wl in ("c5", "c5-bf16"):
            ms = []
            for _ in range(a.bench_runs):
                rec = _child([sys.executable, "bench.py", "--workload", wl], 300, cwd=os.path.abspath(cwd))[-1]
                ms.append(rec["ms_per_step"])
            T.append(f"   {label:9s} {wl:8s} " + "  ".join(f"{v:.3f}" for v in ms) + f"   (range {max(ms) - min(ms):.3f})")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(T) + "\n")
    print("\n".join(T))


if __name__ == "__main__":
    main()
