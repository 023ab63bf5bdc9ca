"""The slm loss value on the HIP path: `WavLMLoss` (train/losses.py:376-394), the last term of the reference's acoustic step
(`step.slm_loss()`, train/stage_type.py:221-225, 363).  Both waves are resampled `model_sr` -> `slm_sr`, both go through a frozen
WavLM (`microsoft/wavlm-base-plus` in the reference's model.yml), and the loss is the L1 distance between the stacks of all
hidden states (13 at full depth); the trainer weights it with `loss_weight.slm`.

What is built: the value -- the network's forward in HIP (csrc/wavlm.hip), logged by the validation pass (`train --slm DIR`) --
and the gradient with respect to the predicted wave: `WavLMLoss.loss_and_grad`, the term inside `AcousticTrainer.train_batch`
(`train --slm DIR --slm-train`).  The network is frozen, so the backward is the input-gradient chain alone: resampler adjoint,
feature-encoder and transformer input gradients, the L1 sign.  It is an explicit call, this package's idiom; there is no
autograd node: `WavLMLoss.forward` still raises in grad mode when the prediction requires a gradient.

Operand mode.  The kind runs fp32 operands by default, whatever the trainer's compute mode is.  `WavLM.set_compute("bf16")`,
`WavLMLoss(..., compute="bf16")` or a per-call `compute="bf16"` of `forward` / `loss_and_grad` (`train --slm DIR --slm-train
--slm-bf16`) put the network's dense contractions -- feature convs 1 .. n - 1, the feature projection, the positional conv,
q / k / v / o, both FFN convs and, at head dim 64, the attention's products -- on the bf16 matrix cores: both operands rounded to
bf16 (RNE), fp32 accumulation, fp32 storage of everything returned or kept.  Layer 0's conv, the norms, GELU, the gate, the
relative bias (added to the logits in fp32), softmax statistics, residual adds, the L1 and the resampler stay fp32 (DESIGN.md
section 4.24 has the list).  The reference runs WavLM under autocast when `mixed_precision` is bf16; the mode is this path's
counterpart and is held to be no further from float64 than autocast is (tests/test_slm_bf16_gpu.py).  The validation value is
always computed on fp32 operands.  `set_train_opts(compute_bf16=True)` keeps refusing the kind: the mode has this door alone.

Nothing is downloaded.  `model` is a local directory in the hub snapshot layout: `config.json` plus `model.safetensors`, or
`pytorch_model.bin` read with `torch.load(weights_only=True)`.  The `transformers` package is not imported: `config.json` is read
as JSON and the network is this package's own.  State-dict keys are those of `WavLMModel.state_dict()` without
`masked_spec_embed` (eval mode never reads it); for the positional conv both spellings of the weight norm load
(`...conv.parametrizations.weight.original0/1` and the older `...conv.weight_g/weight_v` hub files carry); a leading `wavlm.` is
stripped; strict otherwise.

The resampler restates `torchaudio.transforms.Resample(model_sr, slm_sr)` with its defaults (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99) from the documented closed form; torchaudio is not a dependency of this package: PARITY
UNPINNED at that boundary (tests/slm_cases.py has the float64 restatement the kernel is held to).  No test uses trained WavLM
weights: the network is held to the class's own CPU runs on key-filled weights (tests/golden/slm_*); that the value on real
speech is right is not shown by a test.
"""
import ctypes as C
import json
import os.path as osp

import torch

from . import lib as L
from .manifest import WAVLM_DEFAULT_CFG, wavlm_manifest
from .modules import _HipModule, _f32

# config.json fields whose every other value is refused by name (what wavlm-base-plus is by the class defaults)
SUPPORTED = dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False, feat_extract_activation="gelu",
                 hidden_act="gelu")
_SHAPE_FIELDS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "conv_dim", "conv_kernel",
                 "conv_stride", "num_conv_pos_embeddings", "num_conv_pos_embedding_groups", "num_buckets", "max_bucket_distance",
                 "layer_norm_eps")
_WN_OLD = {"weight_g": "parametrizations.weight.original0", "weight_v": "parametrizations.weight.original1"}


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_compute(compute):
    if compute not in ("fp32", "bf16"):
        raise L.StyError(f"WavLM: compute must be 'fp32' or 'bf16', not {compute!r}")
    return compute


def check_wavlm_config(cfg):
    """config.json (a dict) -> the fields wavlm_manifest takes, the class defaults where the file is silent.  A value this path
    does not build is refused by name, as config.check_supported does for model.yml."""
    for name, want in SUPPORTED.items():
        got = cfg.get(name, want)
        if got != want:
            raise L.StyError(f"WavLM config: {name}={got!r} is not built (only {name}={want!r})")
    out = {k: cfg.get(k, WAVLM_DEFAULT_CFG[k]) for k in _SHAPE_FIELDS}
    for k in ("conv_dim", "conv_kernel", "conv_stride"):
        out[k] = tuple(int(v) for v in out[k])
    n = len(out["conv_dim"])
    if not (2 <= n <= 8) or len(out["conv_kernel"]) != n or len(out["conv_stride"]) != n:
        raise L.StyError(f"WavLM config: conv_dim / conv_kernel / conv_stride must have the same length, 2 to 8 (got {n})")
    if out["conv_kernel"][0] > 16:
        raise L.StyError(f"WavLM config: conv_kernel[0]={out['conv_kernel'][0]} is not built (at most 16 taps)")
    if out["num_conv_pos_embeddings"] % 2 or out["num_conv_pos_embeddings"] > 128:
        raise L.StyError(f"WavLM config: num_conv_pos_embeddings={out['num_conv_pos_embeddings']} is not built (even, at most 128)")
    H, heads, G = out["hidden_size"], out["num_attention_heads"], out["num_conv_pos_embedding_groups"]
    if H % heads or H // heads not in (16, 64):
        raise L.StyError(f"WavLM config: hidden_size={H} with num_attention_heads={heads} is not built (head dim 16 or 64)")
    if H % G:
        raise L.StyError(f"WavLM config: num_conv_pos_embedding_groups={G} does not divide hidden_size={H}")
    if out["num_buckets"] < 4 or out["max_bucket_distance"] <= out["num_buckets"] // 4:
        raise L.StyError(f"WavLM config: num_buckets={out['num_buckets']} / max_bucket_distance={out['max_bucket_distance']} "
                         "is not built")
    return out


def wavlm_frames(n16, cfg=None):
    """frames of `n16` samples at the slm rate: floor((n - k) / s) + 1 per feature conv; 0 when a layer is left without one"""
    c = cfg or WAVLM_DEFAULT_CFG
    n = int(n16)
    for k, s in zip(c["conv_kernel"], c["conv_stride"]):
        if n < k:
            return 0
        n = (n - k) // s + 1
    return n


def normalize_state_dict(state):
    """a hub-layout state dict -> the keys of wavlm_manifest: `wavlm.` stripped, the old weight-norm spelling renamed,
    masked_spec_embed dropped"""
    out = {}
    for k, v in state.items():
        if k.startswith("wavlm."):
            k = k[len("wavlm."):]
        if k == "masked_spec_embed":
            continue
        head, _, last = k.rpartition(".")
        if last in _WN_OLD and head.endswith("pos_conv_embed.conv"):
            k = f"{head}.{_WN_OLD[last]}"
        out[k] = v
    return out


class WavLM(_HipModule):
    """transformers' WavLMModel in eval mode with its state_dict keys (manifest.wavlm_manifest).  forward(audio16 [B, N16]) ->
    hidden states [layers + 1, B, T, hidden_size]: what `WavLMModel(x, output_hidden_states=True).hidden_states` stacks to."""
    KIND = "wavlm"

    def __init__(self, **cfg):
        super().__init__()
        self.cfg = check_wavlm_config(cfg)
        self._build(wavlm_manifest(**{k: v for k, v in self.cfg.items() if k != "layer_norm_eps"}))

    def enable_training(self):
        raise L.StyError("WavLM: the network is frozen (no weight gradient is built; forward_keep / backward give the gradient "
                         "with respect to the wave)")

    def set_train_opts(self, **kw):
        if kw.get("compute_bf16"):
            raise L.StyError("WavLM: compute_bf16 is refused: the train options of the kind stay fp32; its bf16 operand mode is "
                             "set with WavLM.set_compute('bf16')")
        return super().set_train_opts(**kw)

    def set_compute(self, compute):
        """the network's operand mode, "fp32" (the default) or "bf16" (see the module docstring); holds until the next call.
        Nothing is re-packed: both weight forms live side by side once each mode has run."""
        self.__dict__["_compute"] = _check_compute(compute)
        if self._handle is not None:
            L.check(L.load().sty_wavlm_set_compute(self._handle, int(compute == "bf16")))
        return self

    @property
    def compute(self):
        return self.__dict__.get("_compute", "fp32")

    def _ensure(self, device):
        if self._handle is None and torch.device(device).type == "cuda":
            lib = L.load()
            h = C.c_void_p()
            L.check(lib.sty_model_create(self.KIND.encode(), C.byref(h)))
            stride = (C.c_int * len(self.cfg["conv_stride"]))(*self.cfg["conv_stride"])
            L.check(lib.sty_wavlm_set_config(h, len(self.cfg["conv_stride"]), stride, int(self.cfg["max_bucket_distance"]),
                                             float(self.cfg["layer_norm_eps"])))
            L.check(lib.sty_wavlm_set_compute(h, int(self.compute == "bf16")))
            self._handle = h
        return super()._ensure(device)

    def forward(self, audio16):
        if torch.is_grad_enabled() and audio16.requires_grad:
            raise L.StyError("WavLM: backward is not built")
        if audio16.dim() != 2 or not audio16.is_cuda:
            raise L.StyError(f"WavLM: audio must be [B, N] on a HIP device (got {tuple(audio16.shape)} on {audio16.device}); "
                             "there is no CPU path")
        B, n16 = audio16.shape
        T = wavlm_frames(n16, self.cfg)
        if T < 1:
            raise L.StyError(f"WavLM: {n16} samples leave no frame behind the feature encoder")
        dev = audio16.device
        lib = self._ensure(dev)
        x = _f32(audio16.detach(), dev)
        out = torch.empty(self.cfg["num_hidden_layers"] + 1, B, T, self.cfg["hidden_size"], dtype=torch.float32, device=dev)
        need = C.c_size_t()
        L.check(lib.sty_wavlm_workspace_bytes(self._handle, B, n16, C.byref(need)))
        ws = self._workspace(need.value, dev)
        L.check(lib.sty_wavlm_fwd(self._handle, B, n16, L.ptr(x), L.ptr(out), L.ptr(ws), ws.numel(), _stream(dev)))
        return out

    def _check_audio(self, audio16):
        if audio16.dim() != 2 or not audio16.is_cuda:
            raise L.StyError(f"WavLM: audio must be [B, N] on a HIP device (got {tuple(audio16.shape)} on {audio16.device}); "
                             "there is no CPU path")
        B, n16 = audio16.shape
        T = wavlm_frames(n16, self.cfg)
        if T < 1:
            raise L.StyError(f"WavLM: {n16} samples leave no frame behind the feature encoder")
        return B, n16, T

    def grad_workspace_bytes(self, B, n16, device):
        lib = self._ensure(device)
        need = C.c_size_t()
        L.check(lib.sty_wavlm_grad_workspace_bytes(self._handle, B, n16, C.byref(need)))
        return need.value

    def forward_keep(self, audio16):
        """forward() -- the same bits -- that keeps in a workspace of its own what backward() reads.  Under no_grad semantics:
        nothing is recorded for autograd."""
        B, n16, T = self._check_audio(audio16)
        dev = audio16.device
        lib = self._ensure(dev)
        x = _f32(audio16.detach(), dev)
        out = torch.empty(self.cfg["num_hidden_layers"] + 1, B, T, self.cfg["hidden_size"], dtype=torch.float32, device=dev)
        need = self.grad_workspace_bytes(B, n16, dev)
        ws = self.__dict__.get("_grad_ws")
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = self.__dict__["_grad_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        self.__dict__["_kept"] = None
        L.check(lib.sty_wavlm_fwd_keep(self._handle, B, n16, L.ptr(x), L.ptr(out), L.ptr(ws), ws.numel(), _stream(dev)))
        self.__dict__["_kept"] = (B, n16, T)
        return out

    def backward(self, d_hidden, tap=False):
        """d_hidden [layers + 1, B, T, H], the cotangent of forward_keep's stack -> d_audio16 [B, N16] (whole: the tail no frame
        reads is zero); tap=True: (d_audio16, d_enc_in [B, H, T]), the gradient at the feature projection's output.  Consumes the
        forward_keep call before it."""
        kept = self.__dict__.get("_kept")
        if kept is None:
            raise L.StyError("WavLM.backward: no forward_keep call precedes it (a backward consumes its forward's workspace)")
        B, n16, T = kept
        want = (self.cfg["num_hidden_layers"] + 1, B, T, self.cfg["hidden_size"])
        if tuple(d_hidden.shape) != want or not d_hidden.is_cuda:
            raise L.StyError(f"WavLM.backward: d_hidden must be {want} on the device of the forward_keep call (got "
                             f"{tuple(d_hidden.shape)} on {d_hidden.device}); the shape belongs to another forward_keep")
        dev = d_hidden.device
        lib = self._ensure(dev)
        g = _f32(d_hidden.detach(), dev)
        ws = self.__dict__["_grad_ws"]
        d_audio = torch.empty(B, n16, dtype=torch.float32, device=dev)
        d_enc = torch.empty(B, self.cfg["hidden_size"], T, dtype=torch.float32, device=dev) if tap else None
        self.__dict__["_kept"] = None
        L.check(lib.sty_wavlm_bwd(self._handle, B, n16, L.ptr(g), L.ptr(d_audio), L.ptr(d_enc), L.ptr(ws), ws.numel(), _stream(dev)))
        return (d_audio, d_enc) if tap else d_audio


def resample(audio, orig, new):
    """torchaudio.transforms.Resample(orig, new) with its defaults, restated (PARITY UNPINNED): [B, N] -> [B, ceil(N new / orig)]"""
    if audio.dim() != 2 or not audio.is_cuda:
        raise L.StyError(f"slm.resample: audio must be [B, N] on a HIP device (got {tuple(audio.shape)} on {audio.device})")
    lib = L.load()
    B, N = audio.shape
    M = lib.sty_slm_resample_len(N, int(orig), int(new))
    if M < 1:
        raise L.StyError(f"slm.resample: {orig} -> {new} on {N} samples is not built")
    x = _f32(audio.detach(), audio.device)
    out = torch.empty(B, M, dtype=torch.float32, device=audio.device)
    L.check(lib.sty_slm_resample_fwd(B, N, int(orig), int(new), L.ptr(x), L.ptr(out), _stream(audio.device)))
    return out


def resample_backward(d_out, n, orig, new, out=None):
    """the adjoint of resample(): d_out [B, ceil(n new / orig)] -> d_audio [B, n]; with `out` given the result is added into it
    (one fp32 add per sample) and `out` is returned"""
    if d_out.dim() != 2 or not d_out.is_cuda:
        raise L.StyError(f"slm.resample_backward: d_out must be [B, M] on a HIP device (got {tuple(d_out.shape)} on {d_out.device})")
    lib = L.load()
    B, M = d_out.shape
    if lib.sty_slm_resample_len(int(n), int(orig), int(new)) != M:
        raise L.StyError(f"slm.resample_backward: {orig} -> {new} on {n} samples gives "
                         f"{lib.sty_slm_resample_len(int(n), int(orig), int(new))} outputs, d_out has {M}")
    if out is not None and (tuple(out.shape) != (B, int(n)) or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.device != d_out.device):
        raise L.StyError(f"slm.resample_backward: out must be a contiguous fp32 [{B}, {n}] on {d_out.device}")
    g = _f32(d_out.detach(), d_out.device)
    res = out if out is not None else torch.empty(B, int(n), dtype=torch.float32, device=d_out.device)
    L.check(lib.sty_slm_resample_bwd(B, int(n), int(orig), int(new), L.ptr(g), L.ptr(res), 1 if out is not None else 0,
                                     _stream(d_out.device)))
    return res


def l1_mean_and_grad(a, b, scale=1.0):
    """(mean |a - b| with the bits of l1_mean, scale * sign(b - a) / n: its gradient with respect to b times `scale`, 0 at a tie)"""
    if a.shape != b.shape or not a.is_cuda:
        raise L.StyError(f"slm.l1_mean_and_grad: shapes {tuple(a.shape)} and {tuple(b.shape)} on {a.device}")
    lib = L.load()
    a, b = _f32(a, a.device), _f32(b, a.device)
    need = C.c_size_t()
    L.check(lib.sty_slm_loss_workspace_bytes(a.numel(), C.byref(need)))
    ws = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=a.device)
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    d_b = torch.empty_like(b)
    L.check(lib.sty_slm_loss_fwd_bwd(a.numel(), L.ptr(a), L.ptr(b), float(scale), L.ptr(loss), L.ptr(d_b), L.ptr(ws), ws.numel() * 8,
                                     _stream(a.device)))
    return loss[0], d_b


def l1_mean(a, b):
    """mean |a - b| of two equally shaped fp32 device tensors, float64 partials in a fixed order: the same inputs, the same bits"""
    if a.shape != b.shape or not a.is_cuda:
        raise L.StyError(f"slm.l1_mean: shapes {tuple(a.shape)} and {tuple(b.shape)} on {a.device}")
    lib = L.load()
    a, b = _f32(a, a.device), _f32(b, a.device)
    need = C.c_size_t()
    L.check(lib.sty_slm_loss_workspace_bytes(a.numel(), C.byref(need)))
    ws = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=a.device)
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    L.check(lib.sty_slm_loss_fwd(a.numel(), L.ptr(a), L.ptr(b), L.ptr(loss), L.ptr(ws), ws.numel() * 8, _stream(a.device)))
    return loss[0]


def load_snapshot(model):
    """(config dict, normalised state dict) of a local hub-layout directory; anything else raises"""
    if not isinstance(model, (str, bytes)) and not hasattr(model, "__fspath__") or not osp.isdir(model):
        raise L.StyError(f"WavLMLoss: {model!r} is not an existing directory.  Nothing is downloaded: pass the local snapshot "
                         "directory of the WavLM model (config.json + model.safetensors or pytorch_model.bin) with --slm")
    cfg_path = osp.join(model, "config.json")
    if not osp.isfile(cfg_path):
        raise L.StyError(f"WavLMLoss: {cfg_path} not found (--slm takes a hub snapshot directory)")
    with open(cfg_path, encoding="utf-8") as f:
        cfg = json.load(f)
    st, pt = osp.join(model, "model.safetensors"), osp.join(model, "pytorch_model.bin")
    if osp.isfile(st):
        from safetensors.torch import load_file
        state = load_file(st)
    elif osp.isfile(pt):
        state = torch.load(pt, map_location="cpu", weights_only=True)
    else:
        raise L.StyError(f"WavLMLoss: neither model.safetensors nor pytorch_model.bin in {model} (--slm)")
    return cfg, normalize_state_dict(state)


class WavLMLoss(torch.nn.Module):
    """WavLMLoss(model, model_sr, slm_sr=16000, compute="fp32") (train/losses.py:376-394): the reference's constructor plus the
    operand mode; `model` is a local snapshot directory.  forward(wav [B, N], y_rec [B, 1, N] or [B, N]) -> scalar, under
    torch.no_grad().  loss_and_grad(wav, y_rec, weight, d_pred) -> (the same scalar, weight * d value / d y_rec [B, N]).  Both take
    `compute=None` ("fp32" / "bf16"): the operand mode of that call alone, so that one object serves the fp32 validation value and
    the bf16 training term; None = the object's own."""

    def __init__(self, model, model_sr, slm_sr=16000, compute="fp32"):
        super().__init__()
        self.compute = _check_compute(compute)
        cfg, state = load_snapshot(model)
        self.wavlm = WavLM(**{k: v for k, v in cfg.items() if k in SUPPORTED or k in _SHAPE_FIELDS})
        self.wavlm.load_state_dict(state, strict=True)
        self.wavlm.eval()
        for p in self.wavlm.parameters():
            p.requires_grad_(False)
        self.model_sr, self.slm_sr = int(model_sr), int(slm_sr)

    def hidden_states(self, wav, compute=None):
        """[B, N] at model_sr -> [layers + 1, B, T, H]"""
        self.wavlm.set_compute(_check_compute(compute or self.compute))
        return self.wavlm(self._to_slm_rate(wav))

    def _to_slm_rate(self, wav):
        # (equal rates: torchaudio's Resample.forward hands the wave back unchanged; the 15-tap table of 1 -> 1 is no identity)
        return wav if self.model_sr == self.slm_sr else resample(wav, self.model_sr, self.slm_sr)

    def forward(self, wav, y_rec, compute=None):
        if torch.is_grad_enabled() and y_rec.requires_grad:
            raise L.StyError("WavLMLoss: backward is not built")
        if y_rec.dim() == 3 and y_rec.shape[1] == 1:
            y_rec = y_rec[:, 0]
        if wav.dim() != 2 or y_rec.dim() != 2:
            raise L.StyError(f"WavLMLoss: wav must be [B, N] and y_rec [B, 1, N] or [B, N] (got {tuple(wav.shape)}, "
                             f"{tuple(y_rec.shape)})")
        if wav.shape != y_rec.shape:
            raise L.StyError(f"WavLMLoss: unequal lengths {tuple(wav.shape)} and {tuple(y_rec.shape)}")
        with torch.no_grad():
            # (the ground-truth stack is kept; the second forward reuses the network's workspace)
            ref = self.hidden_states(wav, compute)
            return l1_mean(ref, self.hidden_states(y_rec, compute))

    def _pair(self, wav, y_rec):
        if y_rec.dim() == 3 and y_rec.shape[1] == 1:
            y_rec = y_rec[:, 0]
        if wav.dim() != 2 or y_rec.dim() != 2:
            raise L.StyError(f"WavLMLoss: wav must be [B, N] and y_rec [B, 1, N] or [B, N] (got {tuple(wav.shape)}, "
                             f"{tuple(y_rec.shape)})")
        if wav.shape != y_rec.shape:
            raise L.StyError(f"WavLMLoss: unequal lengths {tuple(wav.shape)} and {tuple(y_rec.shape)}")
        return y_rec

    @torch.no_grad()
    def loss_and_grad(self, wav, y_rec, weight=1.0, d_pred=None, compute=None):
        """(value, d_audio [B, N]): the unweighted value with the bits forward() gives, and weight * d value / d y_rec -- the weight
        folded into the L1 cotangent.  With `d_pred` (a contiguous fp32 [B, N]) the gradient is accumulated into that tensor, which
        is returned.  Every host-side refusal (shapes, no frame left) is raised before anything is launched."""
        y_rec = self._pair(wav, y_rec)
        B, N = y_rec.shape
        if d_pred is not None and (tuple(d_pred.shape) != (B, N) or d_pred.dtype != torch.float32 or not d_pred.is_contiguous()):
            raise L.StyError(f"WavLMLoss.loss_and_grad: d_pred must be a contiguous fp32 [{B}, {N}] (got {tuple(d_pred.shape)})")
        ref = self.hidden_states(wav, compute)  # (sets the network's mode for the three calls of this step)
        value, d_h = l1_mean_and_grad(ref, self.wavlm.forward_keep(self._to_slm_rate(y_rec)), weight)
        d16 = self.wavlm.backward(d_h)
        if self.model_sr == self.slm_sr:
            if d_pred is None:
                return value, d16
            d_pred.add_(d16)
            return value, d_pred
        return value, resample_backward(d16, N, self.model_sr, self.slm_sr, out=d_pred)
