"""One WavLMLoss.forward (stylish_tts_amd/slm.py: two resamplings, two WavLM forwards, the L1 reduction) at the c3 wave size:
B = 32 x 156 000 samples at 24 kHz, full width (the class defaults, 12 layers), key-filled weights, fp32 operands.  ms per call from
device events around blocks of calls after a warm-up; then one profiled call for the per-family split (sty_prof_report).
Dense work by the issue's count: 87 GFLOP per utterance and forward, 5.6 TFLOP per call; the fp32 matrix-core figure it is set
against is 157.3 TFLOP/s (v_mfma_f32_32x32x2_f32).  python tools/slm_bench.py [B]

--grad: the gradient path at the same size instead -- WavLM.forward_keep and WavLM.backward timed apart, the whole
WavLMLoss.loss_and_grad, the gradient workspace in bytes and the per-family split of one loss_and_grad call.
python tools/slm_bench.py --grad [B]

--compute fp32|bf16|both (default fp32): the operand mode of the network (slm.py, "Operand mode"); `both` measures the two modes one
after the other in one process, fp32 first, and states the ratios.
--step: the c3-gan training step (bench.py's workload: B 32, T 520, bf16 operands, adversarial terms on) with AcousticTrainer driven
directly, in three settings: without the slm term, with it on fp32 operands, with it on bf16 operands (a full-width key-filled
WavLMLoss(24000 -> 16000), w_slm 0.2).  python tools/slm_bench.py --step"""
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from stylish_tts_amd import lib as L
from stylish_tts_amd import slm
from stylish_tts_amd.manifest import WAVLM_DEFAULT_CFG, wavlm_manifest
from stylish_tts_amd.synthetic_weights import fill_state_dict

DEV = "cuda:0"
N = 300 * 520  # bench.py WORKLOADS["c3"]: 6.5 s at 24 kHz
BLOCK, ROUNDS = 2, 5
PEAK_FP32_MFMA = 157.3e12


def dense_flops(n16, cfg=WAVLM_DEFAULT_CFG):
    """multiply-adds x 2 of the dense contractions of one forward of one utterance"""
    n, cin, fl = n16, 1, 0.0
    for dim, k, s in zip(cfg["conv_dim"], cfg["conv_kernel"], cfg["conv_stride"]):
        n = (n - k) // s + 1
        fl += 2.0 * dim * cin * k * n
        cin = dim
    H, FF, T = cfg["hidden_size"], cfg["intermediate_size"], n
    fl += 2.0 * H * cin * T + 2.0 * H * (H // cfg["num_conv_pos_embedding_groups"]) * cfg["num_conv_pos_embeddings"] * T
    fl += cfg["num_hidden_layers"] * (4 * 2.0 * H * H * T + 2 * 2.0 * H * FF * T + 2 * 2.0 * H * T * T)
    return fl, T


def timed(fn, rounds=ROUNDS, block=BLOCK):
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(block):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / block)
    return statistics.median(ms), min(ms), max(ms)


PEAK_BF16_MFMA = 16 * 157.3e12  # v_mfma_f32_32x32x16_bf16: 16 x the fp32 matrix-core rate per clock


def full_width_loss(compute="fp32"):
    with tempfile.TemporaryDirectory() as d:
        from safetensors.torch import save_file
        json.dump({}, open(os.path.join(d, "config.json"), "w"))
        save_file(fill_state_dict(wavlm_manifest(), 23), os.path.join(d, "model.safetensors"))
        return slm.WavLMLoss(d, 24000, 16000, compute=compute).to(DEV)


def grad_main(B, compute="fp32", loss=None):
    """forward-keep, backward, the whole loss_and_grad and its per-family split at the c3 wave size; returns the medians"""
    loss = loss or full_width_loss()
    loss.compute = compute
    loss.wavlm.set_compute(compute)
    print(f"---- operand mode {compute} ----")
    g = torch.Generator().manual_seed(3)
    gt = (0.3 * torch.randn(B, N, generator=g)).to(DEV)
    pr = gt + (0.03 * torch.randn(B, N, generator=g)).to(DEV)
    net = loss.wavlm
    with torch.no_grad():
        x16 = slm.resample(pr, 24000, 16000)
        n16 = x16.shape[1]
        ws = net.grad_workspace_bytes(B, n16, torch.device(DEV))
        h = net.forward_keep(x16)
        cot = torch.randn_like(h) / h.numel()
        net.backward(cot)
        v, _ = loss.loss_and_grad(gt, pr, 0.2)
        torch.cuda.synchronize()
        fwd = timed(lambda: net.forward_keep(x16))
        plain = timed(lambda: net(x16))

        def both():
            net.forward_keep(x16)
            net.backward(cot)

        fb = timed(both)
        whole = timed(lambda: loss.loss_and_grad(gt, pr, 0.2))
        fl, T = dense_flops(n16)
        print(f"slm gradient B={B} N={N} (N16={n16}, T={T}): value {v.item():.6f}; gradient workspace {ws} bytes ({ws / 2**30:.2f} GiB)")
        print(f"  WavLM.forward {plain[0]:.2f} ms; WavLM.forward_keep {fwd[0]:.2f} ms (min {fwd[1]:.2f}, max {fwd[2]:.2f}); "
              f"forward_keep + backward {fb[0]:.2f} ms -> backward {fb[0] - fwd[0]:.2f} ms (by difference); {ROUNDS} blocks of {BLOCK}")
        print(f"  WavLMLoss.loss_and_grad (two resamplings, forward, forward_keep, L1 + sign, backward, resampler adjoint) {whole[0]:.2f} ms "
              f"(min {whole[1]:.2f}, max {whole[2]:.2f}); backward dense work 2 x {B * fl / 1e12:.2f} TFLOP")
        lib = L.load()
        L.check(lib.sty_prof_enable(1))
        loss.loss_and_grad(gt, pr, 0.2)
        torch.cuda.synchronize()
        rows = sorted(L.prof_report(cap=256), key=lambda r: -r["ms"])
        L.check(lib.sty_prof_enable(0))
        tot = sum(r["ms"] for r in rows)
        print(f"per-family split of one loss_and_grad call under the in-situ timers ({tot:.2f} ms in timed launches; untimed glue kernels are not in it):")
        for r in rows:
            tf = r["flops"] / (r["ms"] * 1e-3) / 1e12 if r["ms"] > 0 else 0.0
            print(f"  {r['name']:44s} {r['launches']:5d} launches {r['ms']:9.3f} ms {100 * r['ms'] / tot:5.1f} %  {tf:6.1f} TFLOP/s")
        if compute == "bf16":
            lead = max((r for r in rows if r["flops"] > 0), key=lambda r: r["ms"])
            tf = lead["flops"] / (lead["ms"] * 1e-3)
            print(f"leading dense family in bf16 mode: {lead['name']} at {tf / 1e12:.1f} TFLOP/s, {100 * tf / PEAK_BF16_MFMA:.1f} % of the "
                  f"bf16 matrix-core figure ({PEAK_BF16_MFMA / 1e12:.1f} TFLOP/s)")
            left = [r["name"] for r in rows if r["name"].startswith("conv1d_mfma_kernel") and r["name"].endswith("false>")]
            print("dense families left on conv1d_mfma_kernel<...,false> in bf16 mode: " + (", ".join(left) if left else "none"))
    return dict(forward=plain, forward_keep=fwd, fwd_bwd=fb, loss_and_grad=whole, workspace=ws)


def both_modes(B):
    loss = full_width_loss()
    res = {c: grad_main(B, c, loss) for c in ("fp32", "bf16")}
    print("---- fp32 operands against bf16 operands (medians of the blocks above) ----")
    for k, label in (("forward", "WavLM.forward"), ("forward_keep", "WavLM.forward_keep"), ("fwd_bwd", "forward_keep + backward"),
                     ("loss_and_grad", "WavLMLoss.loss_and_grad")):
        a, b = res["fp32"][k], res["bf16"][k]
        print(f"  {label:28s} fp32 {a[0]:8.2f} ms (min {a[1]:.2f}, max {a[2]:.2f}; spread {a[2] - a[1]:.2f})   bf16 {b[0]:8.2f} ms "
              f"(min {b[1]:.2f}, max {b[2]:.2f})   ratio {a[0] / b[0]:.2f}x, {a[0] - b[0]:.2f} ms less")
    print(f"  gradient workspace: fp32 {res['fp32']['workspace'] / 2**30:.2f} GiB, bf16 {res['bf16']['workspace'] / 2**30:.2f} GiB")


def step_main():
    """the c3-gan step with the trainer driven directly: without the term, with it on fp32 operands, with it on bf16 operands"""
    import bench
    from stylish_tts_amd.acoustic import AcousticTrainer
    from stylish_tts_amd.discriminators import ContextFreeDiscriminator, SpecDiscriminator
    w = bench.WORKLOADS["c3-gan"]
    inp = bench.make_inputs(w, 1000, DEV)
    loss = full_width_loss()
    res = {}
    for label, kw in (("without the term", {}), ("with slm_train, fp32 operands", dict(slm_train=loss, w_slm=0.2, slm_compute="fp32")),
                      ("with slm_train, bf16 operands", dict(slm_train=loss, w_slm=0.2, slm_compute="bf16"))):
        model, style_enc, _ = bench.build_model(DEV)
        torch.manual_seed(7)
        mrd = [SpecDiscriminator().to(DEV) for _ in range(3)]
        trainer = AcousticTrainer(model, style_enc, lr=1e-4, compute=w["compute"], seed=0, mrd=mrd, disc=ContextFreeDiscriminator().to(DEV), **kw)
        n = [0]

        def step():
            n[0] += 1
            trainer.train_batch(audio_gt=inp["audio_gt"], texts=inp["texts"], text_lengths=inp["text_lengths"], pitch=inp["pitch"],
                                durations=inp["durations"], seed=n[0])

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        res[label] = timed(step, rounds=5, block=3)
        r = res[label]
        sv = f"  slm value {float(trainer.slm_value):.6f}" if kw else ""
        print(f"c3-gan step, trainer directly, {label}: median {r[0]:.2f} ms (min {r[1]:.2f}, max {r[2]:.2f}; 5 blocks of 3){sv}")
        del trainer, model, style_enc, mrd
        torch.cuda.empty_cache()
    base, f32, b16 = (res[k] for k in res)
    print(f"the slm term adds {f32[0] - base[0]:.2f} ms on fp32 operands and {b16[0] - base[0]:.2f} ms on bf16 operands to a c3-gan step of "
          f"{base[0]:.2f} ms; step ratio fp32 / bf16 {f32[0] / b16[0]:.2f}x ({f32[0] - b16[0]:.2f} ms less; the fp32 blocks' own spread "
          f"{f32[2] - f32[1]:.2f} ms)")


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    argv = sys.argv[1:]
    compute = "fp32"
    if "--compute" in argv:
        i = argv.index("--compute")
        compute = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
        if compute not in ("fp32", "bf16", "both"):
            raise SystemExit("--compute fp32|bf16|both")
    if "--step" in argv:
        return step_main()
    args = [a for a in argv if a != "--grad"]
    B = int(args[0]) if args else 32
    if "--grad" in argv:
        return both_modes(B) if compute == "both" else grad_main(B, compute)
    if compute == "both":
        raise SystemExit("--compute both goes with --grad")
    with tempfile.TemporaryDirectory() as d:
        from safetensors.torch import save_file
        json.dump({}, open(os.path.join(d, "config.json"), "w"))  # the class defaults
        save_file(fill_state_dict(wavlm_manifest(), 23), os.path.join(d, "model.safetensors"))
        loss = slm.WavLMLoss(d, 24000, 16000, compute=compute).to(DEV)
    g = torch.Generator().manual_seed(3)
    gt = (0.3 * torch.randn(B, N, generator=g)).to(DEV)
    pr = gt + (0.03 * torch.randn(B, N, generator=g)).to(DEV)
    with torch.no_grad():
        for _ in range(2):  # warm-up: code objects, tables, the workspace, the packed weights
            v = loss(gt, pr)
        torch.cuda.synchronize()
        ms = []
        for _ in range(ROUNDS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BLOCK):
                loss(gt, pr)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / BLOCK)
        fl, T = dense_flops((2 * N + 2) // 3)
        total = 2 * B * fl
        med = statistics.median(ms)
        print(f"WavLMLoss.forward B={B} N={N} (T={T}): value {v.item():.6f}; median {med:.2f} ms per call (min {min(ms):.2f}, max {max(ms):.2f}, "
              f"{ROUNDS} blocks of {BLOCK})")
        print(f"dense work {total / 1e12:.2f} TFLOP per call ({fl / 1e9:.1f} GFLOP per utterance and forward): {total / med / 1e9:.1f} TFLOP/s achieved, "
              f"{100 * total / (med * 1e-3) / PEAK_FP32_MFMA:.1f} % of the fp32 matrix-core figure ({PEAK_FP32_MFMA / 1e12:.1f} TFLOP/s)")
        lib = L.load()
        L.check(lib.sty_prof_enable(1))
        loss(gt, pr)
        torch.cuda.synchronize()
        rows = sorted(L.prof_report(cap=256), key=lambda r: -r["ms"])
        L.check(lib.sty_prof_enable(0))
        tot = sum(r["ms"] for r in rows)
        print(f"per-family split of one call under the in-situ timers ({tot:.2f} ms in timed launches; untimed glue kernels are not in it):")
        for r in rows:
            tf = r["flops"] / (r["ms"] * 1e-3) / 1e12 if r["ms"] > 0 else 0.0
            print(f"  {r['name']:44s} {r['launches']:5d} launches {r['ms']:9.3f} ms {100 * r['ms'] / tot:5.1f} %  {tf:6.1f} TFLOP/s")
    validate_only_pass()


def validate_only_pass():
    """one --validate-only pass of the small set-up (the 8-utterance sample dataset, batch 2, an untrained acoustic checkpoint)
    without and with --slm on a full-width key-filled snapshot: wall seconds of the second of two passes each"""
    import time
    from safetensors.torch import save_file
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_sample_dataset import make
    from stylish_tts_amd import train as T
    from tests.test_boundary import _default_config_yaml, _default_model_yaml
    with tempfile.TemporaryDirectory() as d:
        make(os.path.join(d, "data"), 8, 11)
        cfg, mdl, snap = os.path.join(d, "config.yml"), os.path.join(d, "model.yml"), os.path.join(d, "wavlm")
        open(cfg, "w").write(_default_config_yaml(os.path.join(d, "data"), acoustic=dict(epochs=1)))
        open(mdl, "w").write(_default_model_yaml())
        os.makedirs(snap)
        json.dump({}, open(os.path.join(snap, "config.json"), "w"))
        save_file(fill_state_dict(wavlm_manifest(), 23), os.path.join(snap, "model.safetensors"))
        quiet = lambda s: None
        T.train(cfg, mdl, os.path.join(d, "out"), "acoustic", max_steps=1, log=quiet)
        final = os.path.join(d, "out", "acoustic", "checkpoint_final")
        for label, kw in (("without --slm", {}), ("with --slm", dict(slm_path=snap))):
            secs = []
            for i in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx = T.train(cfg, mdl, os.path.join(d, f"v_{len(kw)}_{i}"), "acoustic", checkpoint=final, validate_only=True, log=quiet, **kw)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
            rec = ctx.validation
            print(f"--validate-only, acoustic, {rec['batches']} batches of the sample val split, {label}: {secs[1]:.2f} s (first pass {secs[0]:.2f} s; "
                  f"model loading included)  total {rec['total']:.6f}  slm {rec.get('slm')}")


if __name__ == "__main__":
    main()
