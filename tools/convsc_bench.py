"""convsc_kernel against the families it replaces, over the column count: us per launch from the in-situ event timers, every fused
operand on (input mask, bias, ReLU, out_mask, residual).  python tools/convsc_bench.py  (section 1 of profiles/r10_small_column_convs.txt)"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stylish_tts_amd import lib as L
lib = L.load()
DEV = "cuda:0"
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
def run(B, Ci, Co, K, T, env, n=30):
    for k in ("STY_NO_CONVSC", "STY_CONVSC_MAX_COLS"):
        os.environ.pop(k, None)
    os.environ.update(env)
    torch.manual_seed(B + Ci)
    x = torch.randn(B, Ci, T, device=DEV); w = torch.randn(Co, Ci, K, device=DEV) / (Ci * K) ** 0.5; b = torch.randn(Co, device=DEV)
    r = torch.randn(B, Co, T, device=DEV); m = torch.ones(B, T, device=DEV); y = torch.empty(B, Co, T, device=DEV)
    need = C.c_size_t(); L.check(lib.sty_conv1d_workspace_bytes(Co, Ci, K, C.byref(need)))
    ws = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
    def go():
        L.check(lib.sty_conv1d_fwd_ex(B, Ci, Co, K, 1, T, L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(m), L.ptr(r), L.ptr(m), 0, 1, L.ptr(y), L.ptr(ws), ws.numel(), 1, st))
    for _ in range(5): go()
    torch.cuda.synchronize(); L.prof_report(64); lib.sty_prof_enable(1)
    for _ in range(n): go()
    torch.cuda.synchronize(); lib.sty_prof_enable(0)
    rows = [r_ for r_ in L.prof_report(64) if r_["name"].startswith("conv")]
    return ", ".join("%s %.1f us" % (r_["name"].split("<")[0] + "<" + ",".join(r_["insts"].keys())[:40], 1e3 * r_["ms"] / r_["launches"]) for r_ in rows), y
shapes = [(128, 128, 1), (512, 128, 3), (128, 512, 3), (128, 128, 5)]
for Ci, Co, K in shapes:
    for B in (8, 16, 32, 48, 64, 96, 128, 166):
        on, y1 = run(B, Ci, Co, K, 100, {"STY_CONVSC_MAX_COLS": "100000000"})
        off, y0 = run(B, Ci, Co, K, 100, {"STY_NO_CONVSC": "1"})
        print(f"ci{Ci} co{Co} k{K} cols {B*100:6d}: on [{on}]  off [{off}]  maxdiff {(y1-y0).abs().max().item():.2e}", flush=True)
for Ci, Co, K, T in [(256, 1024, 3, 520), (512, 512, 1, 520), (256, 256, 3, 520)]:
    on, y1 = run(32, Ci, Co, K, T, {"STY_CONVSC_MAX_COLS": "100000000"})
    off, y0 = run(32, Ci, Co, K, T, {"STY_NO_CONVSC": "1"})
    print(f"ci{Ci} co{Co} k{K} cols {32*T:6d}: on [{on}]  off [{off}]  maxdiff {(y1-y0).abs().max().item():.2e}", flush=True)
