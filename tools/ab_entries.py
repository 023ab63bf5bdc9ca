"""Do two builds of libstylish_hip.so answer their entry points alike?  The comparison every host-side refactor needs.

    python tools/ab_entries.py OLD.so NEW.so            # host-only entries: runs without a GPU
    python tools/ab_entries.py OLD.so NEW.so --device   # also the model-bound sizing entries, on synthetic weights (needs a GPU)

Each library is loaded in a child process of its own, which calls the entries over a grid of arguments -- invalid ones (zero,
negative, null pointers) and valid ones -- and records (status, output value, sty_last_error text) per call.  The parent prints
every (entry, arguments) whose record differs and exits non-zero if there is one.

Host half: the model-free sizing and table entries, sty_conv1d_route over all flag bits, sty_model_create with good and bad
kinds, and every model-bound entry on a created but un-finalized model of every kind (and on a null model).
Device half: workspace bytes of the model-bound sizing entries, inference and training, default and deterministic mode; every
training entry in front of the same finalized models (its own kind and the others, training enabled or not) with null and zero
arguments, and each *_fwd_train with too small a workspace in deterministic mode.
"""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = ("speech_predictor", "vocoder", "mel_style_encoder", "duration_predictor", "pitch_energy_predictor", "pitch_style_encoder",
         "text_aligner", "text_aligner_train", "rmvpe", "wavlm")
MODEL_BOUND = re.compile(r"^sty_(model_(?!create|destroy|finalize)\w+|vocoder_\w+|speech_\w+|style_\w+|duration_(?!loss)\w+|pitch_energy_\w+|"
                         r"pitch_style_\w+|aligner_\w+|rmvpe_(workspace_bytes|fwd)|wavlm_(set_config|set_compute|frames|workspace_bytes|"
                         r"fwd|grad_workspace_bytes|fwd_keep|bwd)|convnext_fwd|resblock_fwd|block_\w+)$")


def load(path):
    from stylish_tts_amd import lib as L
    L.LIB_PATH = os.path.abspath(path)
    return L, L.load()


class Recorder:
    def __init__(self, lib):
        self.lib, self.rows = lib, []

    def call(self, name, shown, args, out=None):
        """shown: the arguments as they are reported; out: () -> the output value, read after a call that returned 0"""
        rc = getattr(self.lib, name)(*args)
        err = self.lib.sty_last_error().decode() if rc else ""
        self.rows.append([name, list(shown), rc, out() if out is not None and rc == 0 else None, err])

    def sizing(self, name, grids, null_out=True):
        """an entry (ints..., size_t* bytes): the product of the grids, and one call with bytes == NULL"""
        for v in itertools.product(*grids):
            n = C.c_size_t(0)
            self.call(name, v, list(v) + [C.byref(n)], lambda: n.value)
        if null_out:
            v = [g[-1] for g in grids]
            self.call(name, v + ["NULL"], v + [None])


def host_half(L, lib):
    r = Recorder(lib)
    ch = (-1, 0, 1, 31, 32, 33, 80, 128, 130, 512)
    r.sizing("sty_conv1d_workspace_bytes", [ch, ch, (0, 1, 3, 5, 7, 21)])
    r.sizing("sty_conv1d_bwd_workspace_bytes", [(0, 1, 3), (-1, 1, 32, 80, 512), (0, 1, 32, 33, 512), (0, 1, 3, 5, 7), (0, 1, 62, 80, 6000)])
    k = C.c_int(0)
    for v in itertools.product((2,), (3, 32, 96, 512), (32, 512), (1, 3, 7, 21), (1, 3), (7, 600), (0, 1), range(512)):
        r.call("sty_conv1d_route", v, list(v) + [C.byref(k)], lambda: k.value)
    for v in itertools.product((0, 3), (0, 32, 64), (0, 32, 64, 96), (0, 1, 3, 5, 11), (0, 1, 2), (0, 1, 80, 6000), (0, 1, 2), (0,)):
        r.call("sty_conv1d_route", v, list(v) + [C.byref(k)], lambda: k.value)
    r.call("sty_conv1d_route", (2, 32, 32, 3, 1, 80, 0, 0, "NULL"), [2, 32, 32, 3, 1, 80, 0, 0, None])
    dims = (-1, 0, 1, 2, 3, 62, 80)
    r.sizing("sty_attention_workspace_bytes", [dims, (0, 1, 2, 8), (0, 1, 7, 24, 80, 600)])
    r.sizing("sty_source_workspace_bytes", [dims, (0, 1, 2, 62, 80)])
    r.sizing("sty_mel_workspace_bytes", [(0, 1, 3), (0, 512, 1024, 1025, 18600, 24000), (0, 1024, 2048), (0, 256, 300)])
    for name in ("sty_multispec_workspace_bytes", "sty_acoustic_loss_workspace_bytes"):
        r.sizing(name, [(0, 1, 3), (-1, 0, 1024, 1025, 18600, 24000)])
    r.sizing("sty_acoustic_gan_workspace_bytes", [(0, 1, 3), (0, 1024, 1025, 18600, 24000), (0, 1)])
    r.sizing("sty_grn_bwd_workspace_bytes", [(0, 1, 3), (0, 128, 512, 2048), (0, 1, 62, 80, 6000)])
    r.sizing("sty_rmvpe_mel_workspace_bytes", [(0, 1, 3), (0, 700, 768, 769, 800, 24000)])
    r.sizing("sty_wavlm_strided_conv_workspace_bytes", [(0, 2), (0, 8, 512), (0, 8, 512), (0, 1, 2, 3, 10), (0, 1, 2, 5, 16, 17), (0, 1, 9, 10, 400)])
    for n in (0, 1, 255, 256, 257, 1 << 20, (1 << 31) + 5):
        out = C.c_size_t(0)
        r.call("sty_slm_loss_workspace_bytes", (n,), [n, C.byref(out)], lambda: out.value)
    r.call("sty_slm_loss_workspace_bytes", (5, "NULL"), [5, None])
    rates = (-1, 0, 1, 16000, 22050, 24000, 44100, 48000, 16001)
    for v in itertools.product((0, 1, 300, 24000), rates, rates):
        r.rows.append(["sty_slm_resample_len", list(v), lib.sty_slm_resample_len(*v), None, ""])
    for o, n in itertools.product(rates, rates):
        size = lib.sty_slm_resample_kernel_host(o, n, None)
        digest = None
        if 0 < size <= 1 << 22:
            buf = (C.c_float * size)()
            size = lib.sty_slm_resample_kernel_host(o, n, C.cast(buf, C.c_void_p))
            digest = hashlib.sha1(bytes(buf)).hexdigest()
        r.rows.append(["sty_slm_resample_kernel_host", [o, n], size, digest, ""])
    for v in itertools.product((0, 1, 7, 49, 300), (0, 3, 4, 32, 320), (0, 1, 2, 8, 80, 128, 800)):
        buf = (C.c_int32 * max(2 * v[0] - 1, 1))()
        r.call("sty_wavlm_rel_buckets_host", v, list(v) + [C.cast(buf, C.c_void_p)], lambda: hashlib.sha1(bytes(buf)).hexdigest())
    r.call("sty_wavlm_rel_buckets_host", (7, 32, 128, "NULL"), [7, 32, 128, None])
    # ---- models: creation, then every model-bound entry in front of finalize ----
    h = C.c_void_p()
    for kind in (None, b"", b"speech", b"Vocoder", b"wavlm ") + tuple(k.encode() for k in KINDS):
        r.call("sty_model_create", (kind.decode() if kind is not None else "NULL",), [kind, C.byref(h)])
        if kind and kind.decode() in KINDS:
            lib.sty_model_destroy(h)
    r.call("sty_model_create", ("vocoder", "NULL"), [b"vocoder", None])
    scratch = (C.c_char * 4096)()
    entries = sorted(n for n in L.SYMBOLS if MODEL_BOUND.match(n))

    def make(argtypes, model, ival, null_ptrs):
        args, shown = [model], ["model" if model else "NULL"]
        for t in argtypes[1:]:
            if t is C.c_int:
                v = ival
            elif t in (C.c_size_t, C.c_uint, C.c_uint64):
                v = 4096
            elif t is C.c_float:
                v = 0.25
            elif t is C.c_char_p:
                v = None if null_ptrs else b"generator.amp_prior_block"
            else:  # a pointer of some kind: the zeroed scratch (a zeroed io struct, an int to write) or NULL
                v = None if null_ptrs else C.cast(scratch, t)
            args.append(v)
            shown.append("p" if (v is not None and not isinstance(v, (int, float))) else ("NULL" if v is None else v))
        return args, shown

    for kind in KINDS:
        L.check(lib.sty_model_create(kind.encode(), C.byref(h)))
        for name in entries:
            res, argtypes = L.SYMBOLS[name]
            for model, ival, null_ptrs in ((h, 40, False), (h, 0, False), (h, 40, True), (None, 40, False)):
                args, shown = make(argtypes, model, ival, null_ptrs)
                if res is C.c_int:
                    r.call(name, [kind] + shown, args)
                else:
                    v = getattr(lib, name)(*args)
                    r.rows.append([name, [kind] + shown, 0, v.decode() if isinstance(v, bytes) else v, ""])
        lib.sty_model_destroy(h)
    return r.rows


TRAIN_ENTRY = re.compile(r"^sty_\w+(_train_workspace_bytes|_fwd_train|_prepare_train|_bwd|_bwd_pe)$|^sty_block_fwd_bwd$")


def train_checks(L, r, tag, handle, buf):
    """Every training entry in front of a finalized model, of its kind or of another, with training enabled or not: null
    arguments, then zero dimensions over non-null pointers.  Nothing may reach the device with made-up buffers, so the stream
    stays null, a zeroed io struct stands for an io, and a *_bwd gets null gradients only.  A *_prepare_train of the model's
    kind has no argument to refuse: with training enabled it runs for real."""
    for name in sorted(n for n in L.SYMBOLS if TRAIN_ENTRY.match(n) and MODEL_BOUND.match(n)):
        argtypes = L.SYMBOLS[name][1]
        io = (C.c_char * 1024)()
        for nulls in (True, False):
            if not nulls and (name.endswith(("_bwd", "_bwd_pe", "_prepare_train"))):
                continue
            args, shown = [handle], []
            for i, t in enumerate(argtypes[1:], 1):
                stream = t is C.c_void_p and i == len(argtypes) - 1 and not name.endswith("_workspace_bytes")
                if t is C.c_int:
                    v = 40 if nulls else 0
                elif t in (C.c_size_t, C.c_uint, C.c_uint64):
                    v = 4096
                elif t is C.c_float:
                    v = 0.25
                elif nulls or stream:
                    v = None
                elif t is C.c_char_p:
                    v = b"generator.amp_prior_block"
                elif t is C.c_void_p:
                    v = buf
                else:  # an io struct, all null, or the size_t a sizing entry writes
                    v = C.cast(io, t)
                args.append(v)
                shown.append(v if t in (C.c_int, C.c_float) else ("NULL" if v is None else "p"))
            r.call(name, tag + shown, args)


def small_workspace(L, r, tag, name, handle, ints, buf):
    """a *_fwd_train with every buffer in place and 256 bytes of workspace, in deterministic mode: refused with the bytes the
    mode needs before anything is launched"""
    args, ints = [handle], list(ints)
    argtypes = L.SYMBOLS[name][1]
    keep = []
    for i, t in enumerate(argtypes[1:], 1):
        if t is C.c_int:
            args.append(ints.pop(0))
        elif t is C.c_size_t:
            args.append(256)
        elif t is C.c_uint:
            args.append(0)
        elif t is C.c_float:
            args.append(0.1)
        elif t is C.c_void_p:
            args.append(None if i == len(argtypes) - 1 else buf)
        else:  # the io struct: its dimensions, and every input and output on the buffer (taps and the style stream stay null)
            io = t._type_()
            for f, ft in io._fields_:
                if f in "BLT":
                    setattr(io, f, ints.pop(0))
                elif ft is C.c_void_p and not f.startswith("tap_") and f != "style_stream":
                    setattr(io, f, buf)
            keep.append(io)
            args.append(C.byref(io))
    r.call(name, tag + ["256 bytes"], args)


def device_half(L, lib):
    """workspace bytes of the model-bound sizing entries on finalized models with synthetic weights, and the checks in front of
    the training entries on the same models"""
    import torch
    import stylish_tts_amd as S
    from stylish_tts_amd import manifest as M
    from stylish_tts_amd.alignment import TrainableTextAligner
    from stylish_tts_amd.synthetic_weights import fill_state_dict
    dev = torch.device("cuda:0")
    r = Recorder(lib)
    shapes = [(B, T, Lt) for B in (2, 3) for T, Lt in ((62, 7), (80, 24))]

    def model(cls, manifest, train):
        m = cls()
        m.load_state_dict(fill_state_dict(manifest, 0), strict=False)
        m = m.to(dev)
        if train:
            m.enable_training()
        m._ensure(dev)
        return m

    n_ = C.c_size_t(0)
    zeros = torch.zeros(1 << 20, device=dev)
    buf = zeros.data_ptr()
    for det in (0, 1):
        L.set_deterministic(det)
        for train in (False, True):
            sfx = "_train_workspace_bytes" if train else "_workspace_bytes"
            plan = [(S.SpeechPredictor, M.speech_predictor_manifest(), ("sty_speech", "BLT"), ("sty_vocoder", "BT")),
                    (S.MelStyleEncoder, M.style_encoder_manifest(), ("sty_style", "BT")),
                    (S.PitchStyleEncoder, M.pitch_style_encoder_manifest(), ("sty_pitch_style", "BT")),
                    (S.DurationPredictor, M.duration_predictor_manifest(), ("sty_duration", "BL")),
                    (S.PitchEnergyPredictor, M.pitch_energy_predictor_manifest(), ("sty_pitch_energy", "BLT"))]
            for cls, man, *entries in plan:
                m = model(cls, man, train)
                for (stem, sig), (B, T, Lt) in itertools.product(entries, shapes):
                    v = [dict(B=B, L=Lt, T=T)[c] for c in sig]
                    r.call(stem + sfx, [cls.__name__, "det" if det else "default"] + v, [m._handle] + v + [C.byref(n_)], lambda: n_.value)
                if train and cls is S.SpeechPredictor:
                    for (B, T, Lt), (kind, prefix, Cc) in itertools.product(shapes, ((b"resblock", b"generator.amp_prior_block", 32),)):
                        v = [kind, prefix, B, Cc, 75 * T]
                        r.call("sty_block_train_workspace_bytes", ["SpeechPredictor", "det" if det else "default", kind.decode(), B, Cc, 75 * T],
                               [m._handle] + v + [C.byref(n_)], lambda: n_.value)
                tag = [cls.__name__, "det" if det else "default", "train" if train else "inference"]
                if det and train:
                    for stem, sig in entries:
                        small_workspace(L, r, tag, stem + "_fwd_train", m._handle, [dict(B=3, L=24, T=80)[c] for c in sig], buf)
                train_checks(L, r, tag, m._handle, buf)
                del m
            torch.manual_seed(1234)
            a = TrainableTextAligner(80, 178, hidden_dim=80).to(dev)
            if train:
                a.enable_training()
            a._ensure(dev)
            for B, T, _ in shapes:
                r.call("sty_aligner" + sfx, ["TrainableTextAligner", "det" if det else "default", B, T], [a._handle, B, T, C.byref(n_)],
                       lambda: n_.value)
            tag = ["TrainableTextAligner", "det" if det else "default", "train" if train else "inference"]
            if det and train:
                small_workspace(L, r, tag, "sty_aligner_fwd_train", a._handle, [3, 80], buf)
            train_checks(L, r, tag, a._handle, buf)
            del a
    L.set_deterministic(0)
    return r.rows


def child(path, device):
    L, lib = load(path)
    rows = host_half(L, lib)
    if device:
        rows += device_half(L, lib)
    json.dump(rows, sys.stdout)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new", nargs="?")
    ap.add_argument("--device", action="store_true", help="also size the model-bound entries on synthetic weights (needs a GPU)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        return child(a.old, a.device)
    if not a.new:
        ap.error("two libraries are compared")
    runs = []
    for path in (a.old, a.new):
        cmd = [sys.executable, os.path.abspath(__file__), path, "--child"] + (["--device"] if a.device else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode:
            print(f"{path}: the child process ended with status {p.returncode}")
            return 2
        runs.append(json.loads(p.stdout))
    old, new = runs
    print(f"{len(old)} calls of {len({r[0] for r in old})} entries per library")
    bad = 0
    if len(old) != len(new):
        print(f"the two libraries made {len(old)} and {len(new)} calls")
        bad += 1
    for x, y in zip(old, new):
        if x != y:
            bad += 1
            if bad <= 50:
                print(f"DIFFERS {x[0]}{tuple(x[1])}\n  old: status {x[2]}, value {x[3]}, error {x[4]!r}\n  new: status {y[2]}, value {y[3]}, error {y[4]!r}")
    print(f"records that differ: {bad if bad else 'none'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
