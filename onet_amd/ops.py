"""Tensor-level wrappers over the C ABI (include/onet_hip.h).

PyTorch-ROCm tensors are used for STORAGE ONLY: every function here takes
tensors, checks them, and hands raw device pointers + sizes + the current HIP
stream to libonet_hip.so.  No torch compute op is called on the data path.
There is no CPU fallback: CPU tensors raise."""
from __future__ import annotations

import torch

from . import _lib

F32 = torch.float32


# ----------------------------------------------------------------------------- per-model settings
import os as _os
from collections import namedtuple as _namedtuple


def _flags_from_env():
    """ONET_FLAGS="NAME=VALUE,NAME=VALUE": diagnostic overrides of the module switches below (the values a fresh process starts with;
    tests and tools may also set the attributes directly).  The product has three environment switches of its own -- ONET_HIP_LIB
    (another build of the library), ONET_CONV_ALGO (the default algorithm) and this one; models carry their switches in `Settings`."""
    out = {}
    for item in _os.environ.get("ONET_FLAGS", "").split(","):
        if "=" in item:
            k, v = item.split("=", 1)
            out[k.strip()] = v.strip()
    return out


_FLAGS = _flags_from_env()


def _flag(name, default):
    """Process default of on/off switch `name`: ONET_FLAGS' value if given ("0" = off)."""
    v = _FLAGS.get(name)
    return default if v is None else v != "0"


class Settings:
    """Switches a MODEL carries (`Onet.settings`); a field left at None falls back to the process default (the module
    attribute of the same purpose below, initialised from the environment).  The active record is thread-local: `Onet.forward`
    / `compute_loss` activate their model's record for the calls they make, and every autograd Function of
    onet_amd.functional captures the record active in its forward and re-activates it in its backward (which autograd runs
    on another thread, possibly after another model has run) -- so two models with different settings in one process, or on
    two streams / threads, never see each other's.

      conv          3x3 convolution algorithm: "auto" | "split" | "winograd4" | "direct" | "bf16"         (default CONV_ALGO)
      twin          weight-shared Onet: X and 1-X as ONE batch of 2B                                        (default TWIN)
      convt_bf16    under conv == "bf16": the ConvTranspose2d GEMMs take bf16 operands too                  (default CONVT_BF16)
      lazy_nan      OV:234's NaN assertion deferred to FlatAdam.step()                                      (default LAZY_NAN_CHECK)
      split         under conv == "auto": fp32 3x3 convolutions on the bf16 matrix pipe by operand splitting   (default SPLIT_AUTO)
      bn_on_load    the second convolution of a DoubleConv applies the first unit's BatchNorm + ReLU on load     (default BN_ON_LOAD)
      split_f16     split forward convolution on fp16 parts (22-bit operands); False: bf16 parts (16-bit)         (default SPLIT_F16)
      grad_f16      split input / weight gradients on fp16 parts of power-of-two-scaled operands; False: bf16      (default SPLIT_GRAD_F16)
      split_dgrad   input gradients may take the split kernels (False: diagnostic, fp32-MFMA kernels)             (default SPLIT_DGRAD)
      stem_fused    the stem convolution + its BatchNorm statistics in one streaming pass                          (default STEM_FUSED)
      sync_bn       BatchNorm statistics all-gathered over the process group                                       (default SYNC_BN)
      presplit      the split kernels' operands are written pre-split (fp16 hi | mid slots) by their producers     (default PRESPLIT)
      z_bf16        under conv == "bf16" with pre-split operands: the convolution outputs z are STORED as bf16          (default Z_BF16)
      fused_eval    eval-mode forward under no_grad as a straight-line plan on the pre-split kernels: BatchNorm(eval) + ReLU in
                    the convolution's epilogue, activations kept as slots (onet_amd/inference.py); opt-in                (default FUSED_EVAL)
                    True: fp16 (hi | mid) slots, fp32-level results (needs the fp16-split convolution path: under conv == "bf16" the
                    forward falls back to the default path); "bf16": ONE part of plain bf16 per slot -- the arithmetic conv == "bf16"
                    trains with, a third of the matrix instructions and half the slot bytes -- under any conv with pre-split storage
                    (fused_eval_operands()); "fp16x2+pool" / "bf16+pool": the plan of True / "bf16" with the four encoder units in front
                    of a max-pool in ONE launch each, the pooling in the convolution's epilogue (fused_eval_pool()) -- the same bits;
                    "bf16+pool+ragged": the plan of "bf16+pool" that also takes levels whose maps are not made of full 16 x 32 tiles
                    (fused_eval_ragged(), eval_layer_ok_ragged: even H, W % 4 == 0 -- the data sets' 224 x 224 down to its 28-pixel
                    level); on levels made of full tiles the launches and the bits of "bf16+pool".
                    "fp16x2+ragged": the plan of "fp16x2+pool" ("+pool" implied) that also takes such levels, at fp32 level
                    (eval_layer_ok_ragged_fp16; the exact maxima its bounds start from are taken over the map's own pixels); on
                    levels made of full tiles the launches and the bits of "fp16x2+pool".
                    "bf16+pool+anymap": the plan of "bf16+pool+ragged" whose levels below the first also take maps of ANY H and W, odd
                    included (fused_eval_anymap(), eval_layer_ok_anymap: 200 x 200 down to its 25-pixel level; floor pooling, the
                    reference's F.pad); on every map "bf16+pool+ragged" takes, its launches and bits.
                    "bf16+pool+anymap+pairs": the plan of "bf16+pool+anymap" whose BOTTOM level (level 4: down4 and the ConvTranspose2d
                    of up1) is fused too where its map is 16 pixels wide or narrower (fused_eval_pairs(), eval_layer_ok_pairs: 256 x 256,
                    224 x 224 and 200 x 200 at full depth), two images per tile (include/onet_hip_pairs.h); elsewhere the launches
                    and bits of "bf16+pool+anymap".
                    "bf16+pool+anymap+pairs+up": the plan of "bf16+pool+anymap+pairs" whose ConvTranspose2d edges with an odd-w input map
                    or an output padded into an odd concat map (200 x 200: 12 -> 25 and 25 -> 50) run the slot-operand GEMM too
                    (fused_eval_upmap(), convt_slots_ok_anymap; include/onet_hip_upmap.h): one launch that writes the pad strip itself
                    where "bf16+pool+anymap+pairs" takes the general kernel and a conversion pass, and the level below stops writing
                    fp32.  Such an edge then reads the bf16 slots of the level below, not its unrounded fp32 activation: other bits
                    there; on every input without such an edge (224 x 224, 256 x 256) the launches and bits of "bf16+pool+anymap+pairs".
                    "fp16x2+ragged+pairs": the plan of "fp16x2+ragged" whose BOTTOM level (level 4: down4 and the ConvTranspose2d of
                    up1) is fused too where its map is PAIRS_MIN_W .. 16 pixels wide (fused_eval_pairs_fp16(), eval_layer_ok_pairs_fp16:
                    224 x 224 and 256 x 256 at full depth, at fp32 level), two images per tile (include/onet_hip_split_pairs.h);
                    elsewhere -- 200 x 200 included -- the launches and bits of "fp16x2+ragged".
                    Any other string is a ValueError where the setting is read"""
    __slots__ = ("conv", "twin", "convt_bf16", "lazy_nan", "split", "bn_on_load", "split_f16", "grad_f16", "split_dgrad",
                 "stem_fused", "sync_bn", "presplit", "z_bf16", "fused_eval")

    def __init__(self, conv=None, twin=None, convt_bf16=None, lazy_nan=None, split=None, bn_on_load=None,
                 split_f16=None, grad_f16=None, split_dgrad=None, stem_fused=None, sync_bn=None, presplit=None, z_bf16=None,
                 fused_eval=None):
        self.presplit = presplit
        self.z_bf16 = z_bf16
        self.fused_eval = fused_eval
        self.conv, self.twin, self.convt_bf16, self.lazy_nan = conv, twin, convt_bf16, lazy_nan
        self.split, self.bn_on_load = split, bn_on_load
        self.split_f16, self.grad_f16, self.split_dgrad, self.stem_fused, self.sync_bn = split_f16, grad_f16, split_dgrad, stem_fused, sync_bn

    def replace(self, **kw):
        out = Settings(*(getattr(self, k) for k in self.__slots__))
        for k, v in kw.items():
            setattr(out, k, v)
        return out

    def __repr__(self):
        return "Settings(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


import threading as _threading
_TLS = _threading.local()


def active_settings():
    return getattr(_TLS, "cur", None)


class using:
    """`with ops.using(settings):` -- make `settings` the active record of this thread (None: leave the current one)."""

    def __init__(self, settings):
        self.settings = settings

    def __enter__(self):
        self.prev = getattr(_TLS, "cur", None)
        if self.settings is not None:
            _TLS.cur = self.settings
        return self.settings

    def __exit__(self, *exc):
        _TLS.cur = self.prev
        return False


def _setting(field, default):
    cur = getattr(_TLS, "cur", None)
    v = None if cur is None else getattr(cur, field)
    return default if v is None else v


def conv_algo():
    return _setting("conv", CONV_ALGO)


def twin_enabled():
    return bool(_setting("twin", TWIN))


def lazy_nan_check():
    return bool(_setting("lazy_nan", LAZY_NAN_CHECK))


def split_f16():
    return bool(_setting("split_f16", SPLIT_F16))


def grad_f16():
    return bool(_setting("grad_f16", SPLIT_GRAD_F16))


def split_dgrad():
    return bool(_setting("split_dgrad", SPLIT_DGRAD))


def stem_fused():
    return bool(_setting("stem_fused", STEM_FUSED))


def sync_bn():
    return bool(_setting("sync_bn", SYNC_BN))


def presplit():
    """Pre-split storage (round 4): activations and BatchNorm-backward gradients whose consumers are the split convolution kernels
    are written by their producers as fp16 (hi, mid) parts in the kernels' slot layout; the MFMA kernels' staging is an LDS-DMA copy."""
    if not bool(_setting("presplit", PRESPLIT)) or sync_bn() or not (FUSE_BN_REDUCE and FUSE_POOL):
        return False
    if conv_algo() == "bf16":           # BASELINE configs[2]: the same machinery with ONE part of plain bf16 operands (p16_parts() == 1)
        return True
    return split_enabled() and conv_algo() in ("auto", "split") and split_f16() and split_dgrad()


# One value of Settings.fused_eval.  format: the slot format ("fp16x2": fp16 hi | mid parts, "bf16": one part of plain bf16, None: off);
# pool: the pooled units run as one launch; modes: the level modes the plan takes -- "full" (maps made of full 16 x 32 tiles), "ragged"
# (even H, W % 4 == 0), "anymap" (any H and W, levels below the first), "pairs" (level 4 on image-pair tiles where its map is 16 pixels
# wide or narrower); upmap: ConvTranspose2d edges with an odd-w input or a padded output take the any-map slot GEMM
_FusedEval = _namedtuple("_FusedEval", "format pool modes upmap", defaults=(False, frozenset(("full",)), False))


def _modes(*more):
    return frozenset(("full",) + more)


# The string values of Settings.fused_eval; True is _FusedEval("fp16x2")
_FUSED_EVAL_VALUES = {"bf16": _FusedEval("bf16"), "fp16x2+pool": _FusedEval("fp16x2", True), "bf16+pool": _FusedEval("bf16", True),
                      "bf16+pool+ragged": _FusedEval("bf16", True, _modes("ragged")), "fp16x2+ragged": _FusedEval("fp16x2", True, _modes("ragged")),
                      "bf16+pool+anymap": _FusedEval("bf16", True, _modes("ragged", "anymap")),
                      "bf16+pool+anymap+pairs": _FusedEval("bf16", True, _modes("ragged", "anymap", "pairs")),
                      "bf16+pool+anymap+pairs+up": _FusedEval("bf16", True, _modes("ragged", "anymap", "pairs"), True),
                      "fp16x2+ragged+pairs": _FusedEval("fp16x2", True, _modes("ragged", "pairs"))}
# 1: eval forwards under no_grad take the fused inference plan (Settings.fused_eval); bf16: its one-part plain-bf16 form; either with
# "+pool" ("fp16x2+pool", "bf16+pool"): the pooled units in one launch; "bf16+pool+ragged" / "fp16x2+ragged" ("+pool" implied): ... on
# maps not made of full tiles too; "bf16+pool+anymap": the plan of "bf16+pool+ragged" whose levels below the first take maps of any H and W;
# "bf16+pool+anymap+pairs": the plan of "bf16+pool+anymap" with level 4 fused on image-pair tiles where its map is at most 16 pixels wide
# "bf16+pool+anymap+pairs+up": ... whose ConvTranspose2d edges with an odd-w input or a padded output take the slot-operand GEMM too
#   value                format    pooled units    ragged levels    layer predicate
#   True                 fp16x2    two passes      no               eval_layer_ok
#   "fp16x2+pool"        fp16x2    one launch      no               eval_layer_ok
#   "fp16x2+ragged"      fp16x2    one launch      yes              eval_layer_ok_ragged_fp16
#   "bf16"               bf16      two passes      no               eval_layer_ok_bf16
#   "bf16+pool"          bf16      one launch      no               eval_layer_ok_bf16
#   "bf16+pool+ragged"   bf16      one launch      yes              eval_layer_ok_ragged
#   "bf16+pool+anymap"   bf16      one launch      yes, any map     eval_layer_ok_ragged (level 0), eval_layer_ok_anymap (below)
#   "bf16+pool+anymap+pairs"  bf16  one launch     yes, any map     ... and eval_layer_ok_pairs (level 4)
#   "bf16+pool+anymap+pairs+up"  bf16  one launch  yes, any map     ... and convt_slots_ok_anymap (ConvTranspose2d edges)
#   "fp16x2+ragged+pairs"  fp16x2  one launch      yes              eval_layer_ok_ragged_fp16, eval_layer_ok_pairs_fp16 (level 4)
FUSED_EVAL = _FLAGS["FUSED_EVAL"] if _FLAGS.get("FUSED_EVAL") in _FUSED_EVAL_VALUES else _flag("FUSED_EVAL", False)


def _fused_eval_value():
    """-> the _FusedEval record of the active Settings.fused_eval (format None: off)"""
    v = _setting("fused_eval", FUSED_EVAL)
    if isinstance(v, str):
        if v not in _FUSED_EVAL_VALUES:
            raise ValueError(f"onet_amd: Settings.fused_eval must be None, a bool or one of {sorted(_FUSED_EVAL_VALUES)}, not {v!r}")
        return _FUSED_EVAL_VALUES[v]
    return _FusedEval("fp16x2" if v else None)


def fused_eval():
    return _fused_eval_value().format is not None


def fused_eval_operands():
    """The slot format of the fused eval plan: "fp16x2" (Settings.fused_eval = True, "fp16x2+pool" or "fp16x2+ragged": fp16 hi | mid
    parts), "bf16" (= "bf16", "bf16+pool" or "bf16+pool+ragged": one part of plain bf16), None (off)."""
    return _fused_eval_value().format


def fused_eval_pool():
    """Does the fused eval plan run a unit in front of a max-pool as ONE launch, the pooling in the convolution's epilogue
    (Settings.fused_eval = "fp16x2+pool" | "bf16+pool" and the two ragged values: conv3x3_*_pre_act_pool)?"""
    return _fused_eval_value().pool


def fused_eval_ragged():
    """Does the fused eval plan take levels whose maps are not made of full 16 x 32 tiles (Settings.fused_eval = "bf16+pool+ragged":
    the *_ragged entry points of include/onet_hip_ragged.h, layer predicate eval_layer_ok_ragged; "fp16x2+ragged": those of
    include/onet_hip_ragged_split.h, eval_layer_ok_ragged_fp16)?"""
    return "ragged" in _fused_eval_value().modes


def fused_eval_anymap():
    """Does the fused eval plan take, at its levels below the first, maps of ANY H and W above the width floor (Settings.fused_eval =
    "bf16+pool+anymap": the entry points of include/onet_hip_anymap.h, layer predicate eval_layer_ok_anymap)?  Implies
    fused_eval_ragged(): level 0 and every map of even H and W % 4 == 0 run what "bf16+pool+ragged" runs."""
    return "anymap" in _fused_eval_value().modes


def fused_eval_pairs():
    """Does the fused eval plan take its bottom level (level 4) on image-pair tiles where that level's map is 16 pixels wide or narrower
    (Settings.fused_eval = "bf16+pool+anymap+pairs": the entry point of include/onet_hip_pairs.h, layer predicate eval_layer_ok_pairs)?
    Implies fused_eval_anymap(): every other level runs what "bf16+pool+anymap" runs."""
    v = _fused_eval_value()
    return v.format == "bf16" and "pairs" in v.modes


def fused_eval_upmap():
    """Do the fused eval plan's ConvTranspose2d edges whose input map has odd w or whose output is padded into an odd concat map take the
    slot-operand GEMM (Settings.fused_eval = "bf16+pool+anymap+pairs+up": the entry point of include/onet_hip_upmap.h, predicate
    convt_slots_ok_anymap)?  Implies fused_eval_pairs(): every other launch is what "bf16+pool+anymap+pairs" runs."""
    return _fused_eval_value().upmap


def fused_eval_pairs_fp16():
    """Does the fp32-level (fp16 hi | mid) fused eval plan take its bottom level (level 4) on image-pair tiles where that level's map is
    16 pixels wide or narrower (Settings.fused_eval = "fp16x2+ragged+pairs": the entry point of include/onet_hip_split_pairs.h, layer
    predicate eval_layer_ok_pairs_fp16)?  Implies fused_eval_ragged() on fp16x2 operands: every other level runs what "fp16x2+ragged"
    runs.  The one-part plan's queries (fused_eval_anymap(), fused_eval_pairs(), fused_eval_upmap()) answer False under it."""
    v = _fused_eval_value()
    return v.format == "fp16x2" and "pairs" in v.modes


Z_BF16 = _flag("Z_BF16", True)       # BASELINE configs[2] (conv == "bf16", pre-split operands): conv outputs stored as bf16 (Settings.z_bf16)


def z16_storage():
    """Round 5: under conv == "bf16" with pre-split (plain bf16) operands the 3x3 convolutions STORE their output z as bf16 -- rounded
    once, to nearest even, in the epilogue; the BatchNorm statistics still come from the fp32 accumulators -- and every pass that
    reads z (normalise + ReLU, both backward passes, the pooling backward) moves half the bytes.  z is an internal tensor: nothing
    the reference's callers can see changes type."""
    return conv_algo() == "bf16" and bool(_setting("z_bf16", Z_BF16)) and presplit() and p16_parts() == 1


def p16_parts():
    """Parts per pre-split operand: 2 = fp16 (hi | mid) of the split kernels (fp32-level results), 1 = plain bf16 (conv == "bf16")."""
    return 1 if conv_algo() == "bf16" else 2


def split_enabled():
    return bool(_setting("split", SPLIT_AUTO))


def convt_operand_bf16(B, h, w, Ct):
    """operand_bf16 argument of the onet_convT2x2_* entry points for the calling model and layer: 1 = bf16 operands (the bf16
    conv path), 2 = split bf16 operands (fp32-level results; with the split 3x3 kernels under "auto", on layers whose forward
    GEMM has at least CONVT_SPLIT_MIN_BLOCKS 128 x 128 tiles -- half the CUs by default: like conv3x3_algo, small problems
    keep the fp32 kernels, where there is nothing to gain), 0 = fp32 MFMA"""
    algo = conv_algo()
    if algo == "bf16":
        return int(bool(_setting("convt_bf16", CONVT_BF16)))
    if not (algo in ("auto", "split") and split_enabled() and CONVT_SPLIT):
        return 0
    min_blocks = CONVT_SPLIT_MIN_BLOCKS if CONVT_SPLIT_MIN_BLOCKS is not None else n_cu() // 2
    return 2 if (B * h * w // 128) * (4 * Ct // 128) >= min_blocks else 0


_CU_COUNT = {}


def n_cu(device=None):
    """compute units of the current device (onet_device_info; 256 on MI355X)"""
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    n = _CU_COUNT.get(idx)
    if n is None:
        import ctypes
        cu, lds, wave = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        arch = ctypes.create_string_buffer(64)
        rc = _lib.load().onet_device_info(ctypes.byref(cu), ctypes.byref(lds), ctypes.byref(wave), arch, 64)
        n = int(cu.value) if rc == 0 and cu.value > 0 else 256
        _CU_COUNT[idx] = n
    return n


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def require_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("onet_amd: the HIP path needs tensors on a ROCm GPU (got a CPU tensor); "
                               "there is no CPU fallback -- move the module and inputs to 'cuda'")
        if t is not None and t.dtype != F32 and t.is_floating_point():
            raise TypeError(f"onet_amd: fp32 tensors expected, got {t.dtype}")


def plane(t):
    """-> (tensor, batch_stride) with the (C,H,W) block of every image contiguous.
    Channel-slices of a concat buffer qualify as they are; anything else is copied."""
    B, C, H, W = t.shape
    if is_placeholder(t) and getattr(t, "_onet_twin_src", None) is not None:
        t = twin_materialize(t)          # a reader other than the stem kernels: the twin batch as a real tensor
    if is_placeholder(t):
        raise RuntimeError("onet_amd: an fp32 placeholder (bf16 storage: tensor kept in bf16 only) reached a kernel that reads fp32")
    ok = (W == 1 or t.stride(3) == 1) and (H == 1 or t.stride(2) == W) and (C == 1 or t.stride(1) == H * W)
    if ok and B > 1 and t.stride(0) < C * H * W:
        ok = False
    if not ok:
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else C * H * W)


# Optional in-process kernel timing (bench.py): PROFILE = {} enables HIP-event brackets around the
# MFMA launches, on the stream they are launched on; entries: kind -> [(flops, ev_start, ev_end)].
PROFILE = None
# PROFILE_ALL = {} additionally brackets EVERY other launch of the library (streaming kernels: BatchNorm, pooling, head,
# loss, Adam, packs): entry point -> [(algorithmic HBM bytes | None, ev_start, ev_end)].
PROFILE_ALL = None
_IN_MFMA_BRACKET = False


class _AllHook:
    """_lib.PROFILE_HOOK while PROFILE_ALL is collected; launches inside an MFMA bracket are already timed."""

    @staticmethod
    def begin():
        if PROFILE_ALL is None or _IN_MFMA_BRACKET:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return e0

    @staticmethod
    def end(name, nbytes, e0):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        PROFILE_ALL.setdefault(name, []).append((nbytes, e0, e1))


PROFILE_ONLY = None


def profile_start(everything=True, only=None):
    """everything: bracket every launch of the library (MFMA kernels -> PROFILE, all others -> PROFILE_ALL); else the MFMA kernels
    only -- or, with `only` = a set of kinds, those kinds alone (bench.py's timed region: the dominant kernel)."""
    global PROFILE, PROFILE_ALL, PROFILE_ONLY
    PROFILE = {}
    PROFILE_ALL = {} if everything else None
    PROFILE_ONLY = None if (everything or only is None) else frozenset(only)
    _lib.PROFILE_HOOK = _AllHook if everything else None


def profile_stop():
    """-> (mfma records, all-other records); timing is off afterwards."""
    global PROFILE, PROFILE_ALL
    out = (PROFILE, PROFILE_ALL or {})
    PROFILE = PROFILE_ALL = None
    _lib.PROFILE_HOOK = None
    return out


def _prof_begin(kind=None):
    global _IN_MFMA_BRACKET
    if PROFILE is None or (PROFILE_ONLY is not None and kind not in PROFILE_ONLY):
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    _IN_MFMA_BRACKET = True
    return e0


def _prof_end(kind, flops, e0, nbytes=0.0):
    """flops: direct-algorithm FLOPs of the launch; nbytes: its compulsory HBM bytes (operands read once + result written
    once, fp32)."""
    global _IN_MFMA_BRACKET
    if e0 is None:
        return
    _IN_MFMA_BRACKET = False
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    PROFILE.setdefault(kind, []).append((flops, e0, e1, nbytes))


# OV:234 asserts "jsd is not NaN" inside the loss, which costs a device synchronisation in the MIDDLE of a step (forward
# drained, backward not yet launched: ~1 ms of idle GPU per step at B=32).  A training loop that owns the optimizer
# step (trainer.FlatAdam / trainer.fit, bench.py) may defer the verdict: the flag is copied to pinned host memory behind an
# event, and `check_deferred_nan()` -- called by FlatAdam.step() BEFORE the update is applied, and by the next
# compute_loss -- raises the same AssertionError without draining the queue.  Default: strict (assert in place).
import os as _os

LAZY_NAN_CHECK = _flag("LAZY_NAN_CHECK", False)
_NAN_PENDING = []
_NAN_POOL = []


def defer_nan_check(flag, what="jsd is NaN"):
    host = _NAN_POOL.pop() if _NAN_POOL else torch.empty(1, dtype=torch.bool, pin_memory=True)
    host.copy_(flag.reshape(1), non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _NAN_PENDING.append((host, ev, what))


def check_deferred_nan():
    while _NAN_PENDING:
        host, ev, what = _NAN_PENDING.pop(0)
        ev.synchronize()
        bad = bool(host.item())
        _NAN_POOL.append(host)
        assert not bad, what


_WS = {}


def workspace(nbytes, device):
    """Grow-only scratch buffer per device (wgrad split-K slabs)."""
    key = (device.type, device.index)
    cur = _WS.get(key)
    if cur is None or cur.numel() * 4 < nbytes:
        cur = None
        _WS.pop(key, None)
        cur = torch.empty((int(nbytes) + 3) // 4, dtype=F32, device=device)
        _WS[key] = cur
    return cur


# ----------------------------------------------------------------------------- conv
def pack3x3(w):
    require_gpu(w)
    w = w.detach().contiguous()
    Cout, Cin = w.shape[0], w.shape[1]
    wf = torch.empty(Cin * 9 * Cout, dtype=F32, device=w.device)
    wd = torch.empty(Cout * 9 * Cin, dtype=F32, device=w.device)
    _lib.call("onet_conv3x3_pack_weights", _p(w), _p(wf), _p(wd), Cout, Cin, _stream())
    return wf, wd


def packT2x2(w):
    require_gpu(w)
    w = w.detach().contiguous()
    Cin, Cout = w.shape[0], w.shape[1]
    wf = torch.empty(Cin * 4 * Cout, dtype=F32, device=w.device)
    wd = torch.empty(4 * Cout * Cin, dtype=F32, device=w.device)
    _lib.call("onet_convT2x2_pack_weights", _p(w), _p(wf), _p(wd), Cin, Cout, _stream())
    return wf, wd


def packT2x2_fused(w):
    """[Cin][4*Ct] with column c*4 + sub-pixel: the layout of convT2x2_fwd's shuffle epilogue."""
    require_gpu(w)
    w = w.detach().contiguous()
    Cin, Cout = w.shape[0], w.shape[1]
    wq = torch.empty(Cin * 4 * Cout, dtype=F32, device=w.device)
    _lib.call("onet_convT2x2_pack_weights_fused", _p(w), _p(wq), Cin, Cout, _stream())
    return wq


# BASELINE configs[2]: under the bf16 conv path the ConvTranspose2d GEMMs take bf16 MFMA operands too (what torch.autocast does to
# nn.ConvTranspose2d); CONVT_BF16=0 (ONET_FLAGS) keeps them fp32.  Passed to the library per call (`operand_bf16`).
CONVT_BF16 = _flag("CONVT_BF16", True)


def convT2x2_fwd(x, wq, bias, out, Ct, pt, pl):
    """out[:, c, pt + 2i + di, pl + 2j + dj] = sum_ci x[:, ci, i, j] * W[ci, c, di, dj] + bias[c]: ConvTranspose2d(k=2, s=2)
    written straight into `out`, a plane-contiguous [B, Ct, Ho, Wo] view (e.g. the second half of a concat buffer)."""
    require_gpu(x, wq, out)
    x, xbs = plane(x)
    B, Cin, h, w = x.shape
    Ho, Wo = out.shape[2], out.shape[3]
    obs = out.stride(0) if B > 1 else Ct * Ho * Wo
    e0 = _prof_begin("convt_gemm_kernel")
    _lib.call("onet_convT2x2_fwd", _p(x), xbs, _p(wq), _p(bias), _p(out), obs, B, Cin, Ct, h, w, Ho, Wo, pt, pl,
              convt_operand_bf16(B, h, w, Ct), _stream())
    _prof_end("convt_gemm_kernel", 2.0 * B * h * w * Cin * 4 * Ct, e0, 4.0 * (B * h * w * (Cin + 4 * Ct) + 4 * Cin * Ct))


def convT2x2_out_bound(weight, bias, x_amax):
    """Magnitude slots bounding |ConvTranspose2d(x) + bias| from the layer's weights and the exact max |x| its producer recorded."""
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    slots = new_amax(w.device)
    _lib.call("onet_convT2x2_out_bound", _p(w), _p(bias), w.shape[0], w.shape[1], _p(x_amax), _p(slots), _stream())
    return slots


def packT2x2_slots(w, parts=2, dgrad=False):
    """nn.ConvTranspose2d weight [Cin, Ct, 2, 2] -> the slot pack of the slot-operand forward GEMM: [Cin/8, parts, 4 Ct, 8] fp16 (hi | mid)
    parts of 2^k w (+ (2^k, 2^-k) behind the pack), or one part of bf16(w).  dgrad: -> (that, the K-slot pack of the input gradient
    [(Ct/8) 4, parts, Cin, 8]) from the same launch."""
    require_gpu(w)
    w = w.detach().contiguous()
    Cin, Ct = w.shape[0], w.shape[1]
    dt = torch.float16 if parts == 2 else BF
    wP = torch.empty(Cin * 4 * Ct * parts + 4, dtype=dt, device=w.device)
    wdP = torch.empty(Cin * 4 * Ct * parts + 4, dtype=dt, device=w.device) if dgrad else None
    ws = torch.empty(2048, dtype=torch.int32, device=w.device) if parts == 2 else None
    _lib.call("onet_convT2x2_pack_weights_slots", _p(w), _p(wP), _p(wdP), _p(ws), Cin, Ct, parts, _stream())
    return (wP, wdP) if dgrad else wP


def convT2x2_dgrad_slots(dyP, wdP, Cin, dy_slots=None):
    """dx1 [B, Cin, h, w] fp32 = input gradient of ConvTranspose2d(k=2, s=2) from the pre-split up-sampled gradient dyP [B, Ct/8, 2h, parts,
    2w, 8] and the K-slot pack wdP; None where the kernel does not take the shape."""
    B, C8, Ho, parts, Wo, _ = dyP.shape
    Ct, h, w = C8 * 8, Ho // 2, Wo // 2
    dx = torch.empty((B, Cin, h, w), dtype=F32, device=dyP.device)
    e0 = _prof_begin("convt_gemm_kernel")
    rc = _lib.load().onet_convT2x2_dgrad_slots(_p(dyP), _pbs(dyP), _p(dy_slots), _p(wdP), _p(dx), Cin * h * w, parts, B, Cin, Ct, h, w, _stream())
    flops, nb = 2.0 * B * h * w * Cin * 4 * Ct, B * h * w * (4.0 * Cin + 2.0 * parts * 4 * Ct)
    _prof_end("convt_gemm_kernel", flops if rc == 0 else 0.0, e0, nb if rc == 0 else 0.0)
    if rc < 0:
        raise _lib.OnetHipError(f"onet_convT2x2_dgrad_slots failed ({rc}): {_lib.last_error()}")
    return dx if rc == 0 else None


def convT2x2_wgrad_slots(xP, dyP, dw_shape, x_slots=None, dy_slots=None, want_dbias=False, out=None, db_out=None):
    """(dw [Cin, Ct, 2, 2], dbias | None) from the pre-split input xP and the pre-split up-sampled gradient dyP; None where the kernel does
    not take the shape."""
    B, C8, h, parts, w, _ = xP.shape
    Cin, Ct = C8 * 8, dyP.shape[1] * 8
    assert tuple(dw_shape) == (Cin, Ct, 2, 2) and dyP.shape[3] == parts and dyP.shape[2] == 2 * h and xP.dtype == dyP.dtype
    need = int(_lib.load().onet_convT2x2_wgrad_slots_ws_bytes(B, Cin, Ct, h, w))
    if need <= 0:
        return None
    ws = workspace(need, xP.device)
    dw = out if out is not None else torch.empty(dw_shape, dtype=F32, device=xP.device)
    db = (db_out if db_out is not None else torch.empty(Ct, dtype=F32, device=xP.device)) if want_dbias else None
    e0 = _prof_begin("convt_wgrad_gemm_kernel")
    rc = _lib.load().onet_convT2x2_wgrad_slots(_p(xP), _pbs(xP), _p(x_slots), _p(dyP), _pbs(dyP), _p(dy_slots), _p(dw), _p(db), _p(ws),
                                               ws.numel() * 4, parts, B, Cin, Ct, h, w, _stream())
    flops, nb = 2.0 * B * h * w * Cin * 4 * Ct, 2.0 * parts * B * h * w * (Cin + 4 * Ct)
    _prof_end("convt_wgrad_gemm_kernel", flops if rc == 0 else 0.0, e0, nb if rc == 0 else 0.0)
    if rc < 0:
        raise _lib.OnetHipError(f"onet_convT2x2_wgrad_slots failed ({rc}): {_lib.last_error()}")
    return (dw, db) if rc == 0 else None


def conv3x3_dgrad_bound(weight, dz_slots, ci0):
    """Magnitude slots bounding the channels >= ci0 of a 3x3 convolution's input gradient: max |dz| (dz_slots) x the largest L1 norm of
    the weights feeding one input channel."""
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    slots = new_amax(w.device)
    _lib.call("onet_conv3x3_dgrad_bound", _p(w), w.shape[0], w.shape[1], int(ci0), _p(dz_slots), _p(slots), _stream())
    return slots


def conv3x3_split_dgrad_pre_slots(dzP, wq, Cout, ch0, daP_slots, slots=None, always=False):
    """Input gradient of a decoder block's first convolution from pre-split dz: -> (da [B, Cout, H, W] fp32 whose channels >= ch0 are NOT
    written, daP [B, (Cout - ch0)/8, H, parts, W, 8] = those channels pre-split: fp16 (hi | mid) parts scaled by daP_slots' `always` rule,
    or -- plain bf16 operands -- one part of bf16(da))."""
    B, C8, H, parts, W, _ = dzP.shape
    assert wq.dtype == dzP.dtype == (torch.float16 if parts == 2 else BF)
    da = torch.empty((B, Cout, H, W), dtype=F32, device=dzP.device)
    daP = torch.empty((B, (Cout - ch0) // 8, H, parts, W, 8), dtype=dzP.dtype, device=dzP.device)
    e0 = _prof_begin("conv3x3_split_pre_kernel")
    _lib.call("onet_conv3x3_split_dgrad_pre_slots", _p(dzP), _pbs(dzP), _p(slots), int(always), _p(wq), 2 if parts == 1 else 1, _p(da), Cout * H * W,
              _p(daP), _pbs(daP), int(ch0), _p(daP_slots), B, C8 * 8, Cout, H, W, _stream())
    eb = 2.0 * parts
    _prof_end("conv3x3_split_pre_kernel", 2.0 * B * H * W * C8 * 8 * Cout * 9, e0,
              B * H * W * (eb * C8 * 8 + 4.0 * ch0 + eb * (Cout - ch0)) + eb * 9 * C8 * 8 * Cout)
    return da, daP


CONVT_SLOTS = _flag("CONVT_SLOTS", True)     # 0: the ConvTranspose2d forward reads the fp32 activation (round 4's kernels)


def _convt_domain(parts, mode, B, Cin, Ct, h, w, Ho=None, Wo=None):
    """Does the slot-operand ConvTranspose2d forward of edge mode `mode` (CONVT_ENTRIES) take a layer Cin -> Ct on B maps of h x w with
    `parts` parts per slot, and do the switches want it there?  The convt_slots_ok* predicates are its bindings."""
    # switches; channels and the buffer-resource range
    if not (CONVT_SLOTS and presplit() and (parts == 2 or CONVT_BF16)) or Cin % 32 or Cin < 128 or Ct % 32 or Cin * h * w * 2 * parts >= 2 ** 31:
        return False
    # the mode's maps: any w into the concat map of a floor-pooled level ("anymap"); even w ("ragged") and whole 128-pixel tiles ("full")
    if mode == "anymap":
        return h > 0 and w > 0 and Ho - 2 * h in (0, 1) and Wo - 2 * w in (0, 1)
    return w % 2 == 0 and (mode == "ragged" or (h * w) % 128 == 0)


def convt_slots_ok(B, Cin, Ct, h, w, parts=None):
    """Does the slot-operand ConvTranspose2d forward take this layer (onet_convT2x2_fwd_slots' predicate)?  The block below then writes
    its output pre-split for it (UNet._forward).  parts: parts per slot operand (None: p16_parts(), what the active `conv` trains with)."""
    return _convt_domain(p16_parts() if parts is None else parts, "full", B, Cin, Ct, h, w)


def convt_slots_ok_ragged(B, Cin, Ct, h, w, parts=1):
    """convt_slots_ok(parts) without h w % 128 == 0: the predicate of onet_convT2x2_fwd_slots_ragged (parts = 1, the default) /
    onet_convT2x2_fwd_slots_split_ragged (parts = 2: fp16 hi | mid operands)."""
    return _convt_domain(parts, "ragged", B, Cin, Ct, h, w)


def convt_slots_ok_anymap(B, Cin, Ct, h, w, Ho, Wo):
    """convt_slots_ok_ragged (one part) without even w, into an output map of Ho x Wo: the predicate of onet_convT2x2_fwd_slots_anymap"""
    return _convt_domain(1, "anymap", B, Cin, Ct, h, w, Ho, Wo)


CONVT_BWD_SLOTS = _flag("CONVT_BWD_SLOTS", True)     # 0: the ConvTranspose2d backward GEMMs read fp32 operands (round 4's kernels)


def convt_bwd_slots_ok(B, Cin, Ct, C2, h, w):
    """Do the slot-operand ConvTranspose2d BACKWARD GEMMs take this layer -- and the input gradient of the decoder block's first
    convolution (C2 skip + Ct up-sampled channels on a 2h x 2w map) the slot-writing form that feeds them?"""
    return bool(CONVT_BWD_SLOTS and convt_slots_ok(B, Cin, Ct, h, w) and Cin % 128 == 0 and (w & (w - 1)) == 0
                and C2 % 64 == 0 and (C2 + Ct) % 64 == 0 and (2 * h) % 16 == 0 and (2 * w) % 32 == 0 and Ct * 4 * h * w * 4 < 2 ** 31)


class _LazyPack:
    """One of PackedT's two classic packs, packed when something actually touches the tensor (get())."""

    def __init__(self, owner, i):
        self.owner, self.i = owner, i

    def get(self):
        return self.owner[self.i]


def pack_of(p):
    """The tensor behind a pack handed through autograd as a non-tensor argument: a tensor, or a lazy handle of PackedT."""
    return p.get() if isinstance(p, _LazyPack) else p


class PackedT:
    """Packed forms of one ConvTranspose2d weight: (fused forward pack, input-gradient pack) -- unpacks like that tuple -- plus the slot
    packs of the slot-operand forward, built on first use per number of parts."""

    def __init__(self, w):
        self.w = w.detach()             # (aliases the live parameter, version counter included)
        self._v = self.w._version
        self._t = [None, None]          # built on first use: a step on the slot-operand forward never asks for the fused fp32 pack
        self._s = {}

    def _same_weight(self):
        """A pack made lazily -- at backward time, for the input gradient -- must be of the weight the forward used."""
        if self.w._version != self._v:
            raise RuntimeError("onet_amd: one of the variables needed for gradient computation has been modified by an inplace operation: "
                               f"a ConvTranspose2d weight of shape {list(self.w.shape)} is at version {self.w._version}; expected version "
                               f"{self._v} instead")

    def __getitem__(self, i):
        if self._t[i] is None:
            self._same_weight()
            self._t[i] = packT2x2_fused(self.w) if i == 0 else packT2x2(self.w)[1]
        return self._t[i]

    def __iter__(self):
        return iter((_LazyPack(self, 0), _LazyPack(self, 1)))

    def __len__(self):
        return 2

    def slots(self, parts):
        if parts not in self._s:       # (the backward GEMMs' pack comes out of the same launch -- a training step wants both)
            self._same_weight()
            self._s[parts] = packT2x2_slots(self.w, parts, dgrad=bool(CONVT_BWD_SLOTS))
        v = self._s[parts]
        return v[0] if isinstance(v, tuple) else v

    def dgrad_slots(self, parts):
        v = self._s.get(parts)
        if not isinstance(v, tuple):
            self._same_weight()
            self._s[parts] = v = packT2x2_slots(self.w, parts, dgrad=True)
        return v[1]


# The slot-operand ConvTranspose2d forward (the training forward's launch and the fused eval plan's edges, inference._conv_t): (slot
# format as EVAL_ENTRIES', edge mode) -> (C entry, its binding by name below).  Edge mode: "full" (h w % 128 == 0, even w) | "ragged" (even
# w) | "anymap" (any w, into a map of up to one row and one column more).  A combination that is not a row does not exist.
CONVT_ENTRIES = {
    ("fp16x2", "full"): ("onet_convT2x2_fwd_slots", "convT2x2_fwd_slots"),
    ("bf16", "full"): ("onet_convT2x2_fwd_slots", "convT2x2_fwd_slots"),
    ("bf16", "ragged"): ("onet_convT2x2_fwd_slots_ragged", "convT2x2_fwd_slots_ragged"),
    ("fp16x2", "ragged"): ("onet_convT2x2_fwd_slots_split_ragged", "convT2x2_fwd_slots_split_ragged"),
    ("bf16", "anymap"): ("onet_convT2x2_fwd_slots_anymap", "convT2x2_fwd_slots_anymap"),
}


def eval_convt_name(fmt, mode):
    """The name in this module of the binding of CONVT_ENTRIES[fmt, mode] -- None: no row"""
    return CONVT_ENTRIES.get((fmt, mode), (None, None))[1]


def eval_convt(fmt, mode, xP, wP, bias, outP, Ct, x_slots=None, slots=None, kind="convt_slot_fwd_kernel"):
    """The launch of CONVT_ENTRIES[fmt, mode], what the convT2x2_fwd_slots* functions below are bindings of: ConvTranspose2d(k=2, s=2) +
    bias from the PRE-SPLIT input xP [B, Cin/8, h, parts, w, 8] and the slot pack wP (packT2x2_slots), written pre-split into outP
    [B, Ct/8, Ho, parts, Wo, 8] -- both GEMM operands are LDS-DMA copies.  x_slots / slots: the magnitude slots of input / output.
    -> False where the kernel does not take the shape (nothing written)."""
    (entry, _), two = CONVT_ENTRIES[fmt, mode], fmt == "fp16x2"
    B, C8, h, parts, w, _ = xP.shape
    Cin, Ho, Wo = C8 * 8, outP.shape[2], outP.shape[4]
    assert parts == outP.shape[3] == 1 + two and xP.dtype == wP.dtype == outP.dtype == (torch.float16 if two else BF)
    assert outP.shape[1] * 8 == Ct if mode == "anymap" else (Ho, Wo) == (2 * h, 2 * w)
    with_slots = two or mode == "full"        # (the one-part ragged and any-map entries take neither magnitude slots nor nparts)
    args = (_p(xP), _pbs(xP), *((_p(x_slots),) if with_slots else ()), _p(wP), _p(bias), _p(outP), _pbs(outP),
            *((_p(slots), parts) if with_slots else ()), B, Cin, Ct, h, w, *((Ho, Wo) if mode == "anymap" else ()), _stream())
    e0 = _prof_begin(kind)
    rc = getattr(_lib.load(), entry)(*args)
    flops, nb = 2.0 * B * h * w * Cin * 4 * Ct, 2.0 * parts * (B * (h * w * Cin + Ho * Wo * Ct) + 4 * Cin * Ct)
    _prof_end(kind, flops if rc == 0 else 0.0, e0, nb if rc == 0 else 0.0)
    if rc < 0:
        raise _lib.OnetHipError(f"{entry} failed ({rc}): {_lib.last_error()}")
    return rc == 0


# ---- the table's rows by name
def convT2x2_fwd_slots(xP, wP, bias, outP, Ct, x_slots=None, slots=None, kind="convt_gemm_kernel"):
    """The "full" rows, either format (parts from xP): the training forward's launch too, whose profile kind is the default here (the
    fused eval plan records its launches under the device kernel's own name)"""
    return eval_convt("fp16x2" if xP.shape[3] == 2 else "bf16", "full", xP, wP, bias, outP, Ct, x_slots, slots, kind)


def convT2x2_fwd_slots_ragged(xP, wP, bias, outP, Ct, kind="convt_slot_fwd_kernel"):
    """convT2x2_fwd_slots on one-part bf16 slots whose map has h w % 128 != 0 (any map of even w qualifies): the pixels of the map,
    value for value, as convT2x2_fwd_slots writes them on the map with zero rows appended."""
    return eval_convt("bf16", "ragged", xP, wP, bias, outP, Ct, kind=kind)


def convT2x2_fwd_slots_anymap(xP, wP, bias, outP, Ct, kind="convt_slot_fwd_kernel"):
    """convT2x2_fwd_slots_ragged on a map of ANY w, into outP [B, Ct/8, Ho, 1, Wo, 8] with Ho - 2h, Wo - 2w in {0, 1}: the 2h x 2w block
    in the top-left corner, value for value what that function writes, and the pad strip (row 2h, column 2w) as zero slots, in one launch"""
    return eval_convt("bf16", "anymap", xP, wP, bias, outP, Ct, kind=kind)


def convT2x2_fwd_slots_split_ragged(xP, wP, bias, outP, Ct, x_slots=None, slots=None, kind="convt_slot_fwd_kernel"):
    """convT2x2_fwd_slots_ragged on fp16 (hi | mid) slots (x_slots / slots: the magnitude slots of input / output)"""
    return eval_convt("fp16x2", "ragged", xP, wP, bias, outP, Ct, x_slots, slots, kind)


def convT2x2_fwd_p(x, wq, bias, outP, Ct, pt, pl, slots=None):
    """ConvTranspose2d(k=2, s=2) + bias written PRE-SPLIT into outP [B, Ct/8, Ho, 2, Wo, 8] (the up-sampled channel groups of a pre-split
    concat buffer): no fp32 tensor.  -> False where the GEMM fast path does not take the shape (nothing written)."""
    require_gpu(x, wq)
    x, xbs = plane(x)
    B, Cin, h, w = x.shape
    Ho, Wo = outP.shape[2], outP.shape[4]
    e0 = _prof_begin("convt_gemm_kernel")
    rc = _lib.load().onet_convT2x2_fwd_p(_p(x), xbs, _p(wq), _p(bias), _p(outP), _pbs(outP), _p(slots), outP.shape[3], B, Cin, Ct, h, w, Ho, Wo, pt, pl,
                                         convt_operand_bf16(B, h, w, Ct), _stream())
    flops, nb = 2.0 * B * h * w * Cin * 4 * Ct, 4.0 * (B * h * w * (Cin + 4 * Ct) + 4 * Cin * Ct)
    _prof_end("convt_gemm_kernel", flops if rc == 0 else 0.0, e0, nb if rc == 0 else 0.0)
    if rc < 0:
        raise _lib.OnetHipError(f"onet_convT2x2_fwd_p failed ({rc}): {_lib.last_error()}")
    return rc == 0


# 3x3 convolution algorithm for fwd/dgrad, chosen per call from the layer shape (ONET_CONV_ALGO overrides):
#   "auto" (default)  the split kernels (fp32-level results on the 16-bit matrix cores, conv_split.hip) on maps at least 32 pixels wide
#                     with Cin % 16 == 0 and enough tiles to fill the chip (pre-split operands: also the 16-pixel level at batches that
#                     fill it, pre_layer_ok); else Winograd F(4x4,3x3) where its 64-channel x 32-tile blocks fill the chip, else the
#                     direct implicit-GEMM kernel
#   "split"           the split kernels on every legal layer (parity tests)
#   "winograd4"       F(4x4,3x3) on every legal layer with maps >= 8x8 (parity tests; the fp32-MFMA reference dispatch of bench.py)
#   "direct"          implicit GEMM only
#   "bf16"            BASELINE configs[2]: ONE part of plain bf16 operands through the pre-split kernels (forward, input gradient,
#                     weight gradient) on every layer pre_layer_ok takes -- 32-channel chunks, maps made of full 16 x 32 tiles; "auto"
#                     (fp32 results) elsewhere (round 5 dropped the round-2 bf16 kernels that served the other shapes)
# Layers no Winograd kernel takes (stem Cin < 16, channel counts not multiples of 4) always run direct.
import os as _os
CONV_ALGO = _os.environ.get("ONET_CONV_ALGO", "auto")
# Weight-shared Onet (dwnu is topu): run the X and the 1-X pass as ONE batch of 2B through every convolution
# (BatchNorm keeps the two halves as separate statistics groups).  TWIN=0 (ONET_FLAGS) runs the two passes one after the
# other, as the reference does.
TWIN = _flag("TWIN", True)


BF = torch.bfloat16


_SENTINEL = {}


def _sentinel(device):
    """The 4-byte storage every fp32 placeholder of `device` points at: what identifies one (an expanded gradient or a user's
    `.expand()`ed input has zero strides too, but its own storage -- those are ordinary tensors and are copied by `plane`)."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    s = _SENTINEL.get(key)
    if s is None:
        s = _SENTINEL[key] = torch.zeros(1, dtype=F32, device=device)
    return s


def is_placeholder(t):
    return bool(_SENTINEL) and t.is_cuda and t.dtype == F32 and \
        t.untyped_storage().data_ptr() == _sentinel(t.device).untyped_storage().data_ptr()


def fp32_placeholder(shape, device):
    """A zero-stride fp32 tensor of the given shape over the device's sentinel storage (4 bytes): what autograd passes around
    in place of an activation that exists only in its consumers' operand form (pre-split slots).  Never read by a kernel (`plane` raises).
    Not a view: it has its own version counter, which is what validates the bf16 copy riding on it."""
    t = torch.empty(0, dtype=F32, device=device)
    t.set_(_sentinel(t.device).untyped_storage(), 0, tuple(shape), (0,) * len(shape))
    return t


def twin_virtual(x, bias):
    """The twin batch [X ; clip(1 - X + bias, 0, 1)] (OV:178-180 as one batch of 2B) WITHOUT its tensor: a placeholder of that shape
    carrying (X, bias).  The stem kernels (forward + statistics, weight gradient) form the complement half while they load X
    (clip(1 - X + bias) fused into the stem's load); any other reader gets the real tensor from `plane`, which
    materialises it once (twin_materialize)."""
    t = fp32_placeholder((2 * x.shape[0],) + tuple(x.shape[1:]), x.device)
    t._onet_twin_src = [x, float(bias), None]
    return t


def twin_src_of(t):
    """(X, bias) if `t` is a virtual twin batch whose tensor does not exist, else None."""
    tag = getattr(t, "_onet_twin_src", None)
    return None if tag is None else (tag[0], tag[1])


def twin_materialize(t=None, src=None):
    """The real [2B, C, H, W] tensor of a virtual twin batch (made once per forward, cached on the tag)."""
    tag = getattr(t, "_onet_twin_src", None) if t is not None else None
    if tag is not None and tag[2] is not None:
        return tag[2]
    x, bias = (tag[0], tag[1]) if tag is not None else src
    B = x.shape[0]
    xx = torch.empty((2 * B,) + tuple(x.shape[1:]), dtype=F32, device=x.device)
    xx[:B].copy_(x)
    complement_clip(x, bias, out=xx[B:])
    if tag is not None:
        tag[2] = xx
    return xx


def _z16(z):
    """1 if the convolution output z is stored as bf16 (BASELINE configs[2] with Settings.z_bf16), else 0 (fp32): what the entry points
    that read z take as `z_bf16`; batch strides stay in elements."""
    return int(z.dtype == torch.bfloat16)


def _wino_legal(Cin, Cout):
    return Cin >= 16 and Cin % 4 == 0 and Cout % 4 == 0


def _in_buffer_range(Cin, Cout, H, W):
    """The F(4x4) and bf16 kernels address ONE image (inside a concat buffer of up to twice its channels) through a
    32-bit buffer resource: their entry points reject operands beyond 2 GiB, so the dispatch does not select them there."""
    return (2 * max(Cin, Cout) + 16) * H * W * 4 < 2 ** 31 and (max(Cin, Cout) + 16) * 36 * (max(Cin, Cout) + 63) * 4 < 2 ** 31


def _direct_in_range(Cin, Cout, H, W):
    """The direct fp32-MFMA kernels also stage one image and the packed weight through a 32-bit buffer resource with 32-bit byte
    offsets.  This is the range of ONE launch, the convolution Cin -> Cout that the dispatch is asked about (launch_fwd of
    conv_mfma.hip, the same arithmetic; the input gradient asks with the channels swapped).  The weight gradient's range is narrower --
    (max(Cin, Cout) + 64) H W 4 bytes, a whole 64-channel tile of look-ahead -- and is not checked here, because inference never
    runs it: a layer between the two is dispatched, and its backward is refused by onet_conv_wgrad's own check (OnetHipError)."""
    return (Cin + 16) * H * W * 4 < 2 ** 31 and (Cin + 16) * 9 * Cout * 4 < 2 ** 31


def _split_legal(Cin, Cout, H, W):
    return Cin % 16 == 0 and W > 16 and W % 4 == 0 and H >= 8


def conv3x3_algo(B, Cin, Cout, H, W):
    """-> "split" | "winograd4" | "direct" | "bf16" for a conv with Cin inputs and Cout outputs on B maps of H x W."""
    algo = conv_algo()
    if not _direct_in_range(Cin, Cout, H, W):
        raise ValueError("conv3x3: one image of %d channels on a %d x %d map (or its packed weight) exceeds the 2 GiB buffer-resource "
                         "range of every convolution kernel; tile the map" % (Cin, H, W))
    if algo in ("bf16", "winograd4", "auto", "split") and not _in_buffer_range(Cin, Cout, H, W):
        # between the two ranges: _in_buffer_range allows for a concat buffer of twice the channels, the direct kernel
        # (onet_conv_fwd / onet_conv_wgrad, which check their own range) addresses one image of exactly Cin channels
        algo = "direct"
    if algo == "split":
        if _split_legal(Cin, Cout, H, W):
            return "split"
        algo = "auto_nosplit"
    if algo == "auto" and split_enabled() and _split_legal(Cin, Cout, H, W):
        # persistent 8-wave blocks, one per CU, tiles of 64 channels x 16 rows x 32 pixels: worth it once every CU gets a tile
        if B * -(-H // 16) * -(-W // 32) * -(-Cout // 64) >= (n_cu() * 3) // 4:
            return "split"
    if algo == "auto_nosplit":
        algo = "auto"
    if algo == "bf16":
        if Cin % 16 == 0 and Cout % 4 == 0 and W >= 16 and H >= 8:
            return "bf16"
        algo = "auto"
    if algo == "direct" or not _wino_legal(Cin, Cout):
        return "direct"
    # on maps smaller than 8x8 the tile quantisation wastes most of an MFMA tile and the direct kernel's
    # two-level accumulation is the more accurate one (the 1x1 .. 4x4 bottleneck maps of small inputs feed
    # BatchNorm batches of a few values per channel, which amplify any rounding difference)
    if min(H, W) < 8:
        return "direct"
    if algo == "winograd4":
        return "winograd4"
    if min(H, W) >= 16:
        img = 1 if W > 16 else 2                       # conv_wino4.hip block: 32 tiles of 4x4 px, 64 channels
        blocks = -(-B // img) * -(-W // (32 if W > 16 else 16)) * -(-H // 16) * -(-Cout // 64)
        if blocks >= (n_cu() * 7) // 8:
            return "winograd4"
    return "direct"                   # (round 5: the F(2x2,3x3) kernels that used to take the layers too small to fill the chip are gone)


def use_winograd(Cin, Cout, H, W):
    """May a Winograd weight-gradient kernel (F(3x3,4x4)) take this layer?"""
    return conv_algo() != "direct" and _wino_legal(Cin, Cout) and min(H, W) >= 8


class Packed3x3(dict):
    """Packed forms of one 3x3 weight, built on first use per algorithm: [algo] -> (fwd, dgrad)."""

    def __init__(self, w):
        super().__init__(Cin=w.shape[1], Cout=w.shape[0])
        self.w = w.detach()

    def get_pack(self, algo):
        if algo not in self:
            self[algo] = {"direct": pack3x3, "winograd4": pack3x3_winograd4, "split": pack3x3_split, "plain16": pack3x3_plain16}[algo](self.w)
        return self[algo]


def pack3x3_auto(w):
    """-> lazily packed weights for conv3x3_auto: each algorithm's transform runs on first use after a weight
    update, so a layer only pays for the packs its shapes actually select."""
    return Packed3x3(w)


def _fp32_algo(B, Cin, Cout, H, W):
    """conv3x3_algo for a layer that runs on fp32 tensors whatever the model's setting: under conv == "bf16" the layers outside the
    pre-split plain-bf16 kernels' reach (the stem, the smallest maps, odd shapes) take the fp32 dispatch -- round 5 dropped the
    round-2 bf16 kernels that used to serve them."""
    algo = conv3x3_algo(B, Cin, Cout, H, W)
    if algo != "bf16":
        return algo
    cur = active_settings()
    with using(cur.replace(conv="auto") if cur is not None else Settings(conv="auto")):
        return conv3x3_algo(B, Cin, Cout, H, W)


def conv3x3_auto(x, pk, direction, out=None, amax=None):
    """direction 0: forward (Cin -> Cout); 1: dgrad (Cout -> Cin) with the flipped/transposed pack.
    amax: the 64 magnitude slots of x (int32 [64], written by its producer): what the fp16 split kernels scale x by -- computed here
    (one pass over x) where the fp16-split kernel takes the layer and the caller has none: without them an element >= 65520 is fp16 inf."""
    Ci, Co = (pk["Cin"], pk["Cout"]) if direction == 0 else (pk["Cout"], pk["Cin"])
    shp = x.shape
    algo = _fp32_algo(shp[0], Ci, Co, shp[2], shp[3])
    if algo == "split" and direction == 1 and not split_dgrad():     # diagnostic: input gradients on the fp32-MFMA kernels
        with using(active_settings().replace(split=False) if active_settings() is not None else Settings(split=False)):
            algo = _fp32_algo(shp[0], Ci, Co, shp[2], shp[3])
    wq = pk.get_pack(algo)[direction]
    if algo == "winograd4":
        return conv3x3_winograd4(x, wq, Co, out=out)
    if algo == "split":
        if direction == 0 and amax is None and wq.dtype == torch.float16:
            amax = absmax_slots(x)
        return conv3x3_split(x, wq, Co, out=out, amax=amax, always=direction == 1)
    return conv_fwd(x, wq, Co, 3, out=out)


BN_ON_LOAD = _flag("BN_ON_LOAD", True)        # 0: every BatchNorm + ReLU output is materialised
# every 64-channel output tile of the forward kernel normalises the input tile again: the extra staging work grows with
# Cout / 64 while the saved pass does not -- measured worth it up to two output tiles (the 256- and 128-pixel levels)
BN_ON_LOAD_MAX_COUT = 128
CONVT_SPLIT_MIN_BLOCKS = None                 # tests may set a tile count; None: half the CUs (convt_operand_bf16)
CONVT_SPLIT = _flag("CONVT_SPLIT", True)     # 0: the ConvTranspose2d GEMMs stay on the fp32 MFMA pipe
SPLIT_F16 = _flag("SPLIT_F16", True)         # 0: the forward split kernel takes bf16 parts like the gradients
SPLIT_DGRAD = _flag("SPLIT_DGRAD", True)     # 0 (diagnostic): input gradients stay on the fp32-MFMA kernels
PRESPLIT = _flag("PRESPLIT", True)           # 1: pre-split operand storage (Settings.presplit)
PRESPLIT_W16 = _flag("PRESPLIT_W16", True)    # ... also the 16-pixel level (0: fp32 Winograd F(4x4) there, as in round 3)
# diagnostic / tests: every activation written pre-split ALSO leaves its fp32 tensor (same values: the parts are split from them), so
# that a harness can read each unit's output; the kernels that consume the pre-split forms are unchanged
PRESPLIT_KEEP_FP32 = _flag("PRESPLIT_KEEP_FP32", False)
# 1: split input / weight gradients on fp16 parts of power-of-two-scaled operands (22-bit operands; 15x lower per-layer error than
# the bf16 parts, but no change in the model-level worst gradient error -- 9.4e-5 either way on b4_c1_256 -- and +1.3 ms/step: the
# fp16 MFMAs hold a lower clock); default 0: bf16 parts, as in round 3
SPLIT_GRAD_F16 = _flag("SPLIT_GRAD_F16", False)
SPLIT_WGRAD_MINW = 16                        # the split weight gradient covers the 32- and 16-pixel levels too
SPLIT_AUTO = _flag("SPLIT", True)          # 0: "auto" never selects the split-bf16 kernel (round-2 dispatch)
STEM_FUSED = _flag("STEM_FUSED", True)      # 0: the stem takes the direct MFMA kernel + a statistics pass


def conv3x3_fwd_bn_partials(x, pk, norm=None, amax=None):
    """Forward 3x3 convolution of a Conv-BatchNorm pair (OV:47-48, 51-52): -> (z, cm).  cm = the channel-major
    BatchNorm records [Cout, nparts, 3] the F(4x4) kernel's epilogue emits (image-major: nparts / B per image), or None
    where the selected kernel does not emit them (then `bn_train_coeffs` runs its own statistics pass).
    norm = (z_prev, save [G, 4, Cin], slots): normalise on load -- x is NOT read; the input is relu(bn(z_prev)) of the unit below,
    applied in the split kernel's staging (the caller has checked norm_on_load_ok); slots: magnitude slots bounding that activation
    (its BatchNorm bound, bn_train_coeffs' act_slots), the fp16 parts' range guard, or None.
    amax: the magnitude slots of x; where the fp16-split kernel takes the layer and x has none, they are computed here (one pass)."""
    Ci, Co = pk["Cin"], pk["Cout"]
    if norm is not None:
        z_prev, save, slots = norm
        require_gpu(z_prev, save)
        zs, zbs = plane(z_prev)
        B, _, H, W = zs.shape
        nparts = int(_lib.load().onet_conv3x3_split_nparts(B, H, W)) if not sync_bn() else 0
        out = torch.empty((B, Co, H, W), dtype=F32, device=zs.device)
        cm = torch.empty((Co, nparts, 3), dtype=F32, device=zs.device) if nparts > 0 else None
        e0 = _prof_begin("conv3x3_split_kernel")
        wq = pk.get_pack("split")[0]
        f16 = wq.dtype == torch.float16
        _lib.call("onet_conv3x3_split_fwd_norm", _p(zs), zbs, _p(save), save.shape[0], _p(wq), int(f16), _p(slots) if f16 else None,
                  _p(out), Co * H * W, _p(cm), B, Ci, Co, H, W, _stream())
        _prof_end("conv3x3_split_kernel", 2.0 * B * H * W * Ci * Co * 9, e0, 4.0 * (B * H * W * (Ci + Co) + 9 * Ci * Co))
        return out, cm
    B, _, H, W = x.shape
    if Ci <= 4 and stem_fused() and not sync_bn() and hasattr(pk, "w"):
        # the stem (Cin = n_channels): one streaming pass writes z and its statistics records (stem.hip)
        nparts = int(_lib.load().onet_conv3x3_stem_nparts(B, Ci, Co, H, W))
        if nparts > 0:
            require_gpu(x)
            tw = twin_src_of(x)          # virtual twin batch: the kernel reads X and forms the complement half on load (K7)
            xs, xbs = plane(tw[0] if tw is not None else x)
            w = pk.w if pk.w.is_contiguous() else pk.w.contiguous()
            out = torch.empty((B, Co, H, W), dtype=F32, device=x.device)
            cm = torch.empty((Co, nparts, 3), dtype=F32, device=x.device)
            e0 = _prof_begin("stem_conv_stats_kernel")
            _lib.call("onet_conv3x3_stem_fwd_stats", _p(xs), xbs, _p(w), _p(out), Co * H * W, _p(cm), B, Ci, Co, H, W,
                      B // 2 if tw is not None else 0, tw[1] if tw is not None else 0.0, _stream())
            _prof_end("stem_conv_stats_kernel", 2.0 * B * H * W * Ci * Co * 9, e0, 4.0 * (B * H * W * (Ci + Co) + 9 * Ci * Co))
            return out, cm
    algo = _fp32_algo(B, Ci, Co, H, W)
    nparts = 0
    if algo == "winograd4" and not sync_bn():
        nparts = int(_lib.load().onet_conv3x3_winograd4_nparts(B, H, W))
    if algo == "split" and not sync_bn():
        nparts = int(_lib.load().onet_conv3x3_split_nparts(B, H, W))
        if nparts > 0:
            wq = pk.get_pack(algo)[0]
            require_gpu(x)
            xs, xbs = plane(x)
            if xs.data_ptr() % 16 or xbs % 4:
                xs = xs.contiguous()
                xbs = xs.stride(0) if B > 1 else xs[0].numel()
            out = torch.empty((B, Co, H, W), dtype=F32, device=x.device)
            cm = torch.empty((Co, nparts, 3), dtype=F32, device=x.device)
            if wq.dtype == torch.float16 and amax is None:
                amax = absmax_slots(xs)
            e0 = _prof_begin("conv3x3_split_kernel")
            if wq.dtype == torch.float16:
                _lib.call("onet_conv3x3_split_conv_amax", _p(xs), xbs, _p(amax), 0, _p(wq), _p(out), Co * H * W, _p(cm), B, Ci, Co, H, W,
                          _stream())
            else:
                _lib.call("onet_conv3x3_split_fwd_stats", _p(xs), xbs, _p(wq), 0, _p(out), Co * H * W, _p(cm), B, Ci, Co, H, W, _stream())
            _prof_end("conv3x3_split_kernel", 2.0 * B * H * W * Ci * Co * 9, e0, 4.0 * (B * H * W * (Ci + Co) + 9 * Ci * Co))
            return out, cm
    if nparts <= 0:
        return conv3x3_auto(x, pk, 0, amax=amax), None
    wq = pk.get_pack(algo)[0]
    require_gpu(x, wq)
    x, xbs = plane(x)
    out = torch.empty((B, Co, H, W), dtype=F32, device=x.device)
    cm = torch.empty((Co, nparts, 3), dtype=F32, device=x.device)
    e0 = _prof_begin("conv_wino4_kernel")
    _lib.call("onet_conv3x3_winograd4_fwd_stats", _p(x), xbs, _p(wq), _p(out), Co * H * W, _p(cm), B, Ci, Co, H, W,
              _stream())
    _prof_end("conv_wino4_kernel", 2.0 * B * H * W * Ci * Co * 9, e0, 4.0 * (B * H * W * (Ci + Co) + 9 * Ci * Co))
    return out, cm


FUSE_BN_REDUCE = _flag("FUSE_BN_REDUCE", True)


def conv3x3_dgrad_bnreduce(dz, pk, z_prev, save_prev):
    """Input gradient of the second convolution of a Conv-BN-ReLU-Conv chain (OV:47-53) with the first BatchNorm-backward
    pass of the layer BELOW folded into the epilogue: -> (da, records [Cin, nparts, 2]) or None where the F(4x4) kernel
    is not the one selected / the map is not made of full blocks.  save_prev: [G, 4, Cin] coefficients of the G
    statistics groups (consecutive batch slices) of the layer below; z_prev its pre-activation."""
    if not FUSE_BN_REDUCE or sync_bn():
        return None
    Ci, Co = pk["Cout"], pk["Cin"]                       # dgrad: Cout -> Cin
    B, _, H, W = dz.shape
    if conv3x3_algo(B, Ci, Co, H, W) != "winograd4":
        return None
    nparts = int(_lib.load().onet_conv3x3_winograd4_nparts(B, H, W))
    G = save_prev.shape[0]
    if nparts <= 0 or B % G or tuple(z_prev.shape) != (B, Co, H, W) or not save_prev.is_contiguous():
        return None
    z_prev, zbs = plane(z_prev)
    if (zbs & 3) or (z_prev.data_ptr() & 15):
        return None
    wq = pk.get_pack("winograd4")[1]
    require_gpu(dz, wq, z_prev, save_prev)
    dz, dbs = plane(dz)
    da = torch.empty((B, Co, H, W), dtype=F32, device=dz.device)
    rec = torch.empty((Co, nparts, 2), dtype=F32, device=dz.device)
    e0 = _prof_begin("conv_wino4_kernel")
    _lib.call("onet_conv3x3_winograd4_dgrad_bnreduce", _p(dz), dbs, _p(wq), _p(da), Co * H * W, _p(z_prev), zbs,
              _p(save_prev), B // G, _p(rec), B, Ci, Co, H, W, _stream())
    _prof_end("conv_wino4_kernel", 2.0 * B * H * W * Ci * Co * 9, e0, 4.0 * (B * H * W * (Ci + Co) + 9 * Ci * Co))
    return da, rec






def pack3x3_winograd4(w):
    """F(4x4,3x3) transformed weights: (fwd [Cin][36][CoutP], dgrad [Cout][36][CinP]) with the row's channel dimension padded to
    a multiple of 64 and permuted inside 64-blocks as conv_wino4.hip's A operand wants it (written in full by the pack kernel)."""
    require_gpu(w)
    w = w.detach().contiguous()
    Cout, Cin = w.shape[0], w.shape[1]
    wf = torch.empty(Cin * 36 * ((Cout + 63) // 64 * 64), dtype=F32, device=w.device)
    wd = torch.empty(Cout * 36 * ((Cin + 63) // 64 * 64), dtype=F32, device=w.device)
    _lib.call("onet_conv3x3_pack_weights_winograd4", _p(w), _p(wf), _p(wd), Cout, Cin, _stream())
    return wf, wd


def conv3x3_winograd4(x, wq, Cout, out=None):
    """z = conv3x3(x) by Winograd F(4x4,3x3) with transformed weights wq ([Cin][36][Cout]); fwd and dgrad."""
    require_gpu(x, wq)
    x, xbs = plane(x)
    B, Cin, H, W = x.shape
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=F32, device=x.device)
    zbs = out.stride(0) if B > 1 else Cout * H * W
    e0 = _prof_begin("conv_wino4_kernel")
    _lib.call("onet_conv3x3_winograd4_fwd", _p(x), xbs, _p(wq), _p(out), zbs, B, Cin, Cout, H, W, _stream())
    _prof_end("conv_wino4_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0, 4.0 * (B * H * W * (Cin + Cout) + 9 * Cin * Cout))
    return out


def pack3x3_plain16(w):
    """Plain bf16 packs (ONE part, bf16(w)) in the split kernels' slot order, for the pre-split kernels under conv == "bf16":
    (fwd [Cin/16][9][2][Cout][8], dgrad [ceil(Cout/16)][9][2][Cin][8])."""
    require_gpu(w)
    w = w.detach().contiguous()
    Cout, Cin = w.shape[0], w.shape[1]
    wf = torch.empty(Cin * 9 * Cout + 8, dtype=BF, device=w.device) if Cin % 16 == 0 else None
    wd = torch.empty((-(-Cout // 16) * 16) * 9 * Cin + 8, dtype=BF, device=w.device)
    _lib.call("onet_conv3x3_split_pack_weights", _p(w), _p(wf), _p(wd), None, Cout, Cin, 2, 2, _stream())
    return wf, wd


def pack3x3_split(w):
    """bf16 (hi, mid) packs of a 3x3 weight for conv_split.hip: (fwd [Cin/16][2][9][2][Cout][8], dgrad [ceil(Cout/16)][2][9][2][Cin][8]);
    a pack whose reduction dimension is not a multiple of 16 on the forward side is None."""
    require_gpu(w)
    w = w.detach().contiguous()
    Cout, Cin = w.shape[0], w.shape[1]
    # a pack's parts are fp16 (of 2^k w, k from the tensor's largest magnitude; (2^k, 2^-k) stored behind the pack: + 8 elements)
    # or bf16 -- its dtype tells conv3x3_split which arithmetic the pack is for
    f_fwd, f_dg = split_f16(), grad_f16() or presplit()
    wf = torch.empty(2 * Cin * 9 * Cout + 8, dtype=torch.float16 if f_fwd else BF, device=w.device) if Cin % 16 == 0 else None
    wd = torch.empty(2 * (-(-Cout // 16) * 16) * 9 * Cin + 8, dtype=torch.float16 if f_dg else BF, device=w.device)
    ws = torch.empty(AMAX_SLOTS, dtype=torch.int32, device=w.device) if (f_fwd or f_dg) else None
    _lib.call("onet_conv3x3_split_pack_weights", _p(w), _p(wf), _p(wd), _p(ws), Cout, Cin, int(f_fwd), int(f_dg), _stream())
    return wf, wd


class counting_batches:
    """Within the block BatchNorm's num_batches_tracked increments (count_batches) are collected and applied in ONE multi-tensor launch
    at the end (also when the block raises: the units that ran have updated their running statistics)."""

    def __enter__(self):
        self.outer = getattr(_TLS, "counters", None)
        _TLS.counters = []
        return self

    def __exit__(self, *exc):
        pending, _TLS.counters = _TLS.counters, self.outer
        by_inc = {}
        for t, n in pending:
            by_inc.setdefault(n, []).append(t)
        for n, ts in by_inc.items():
            if len(ts) > 1 and all(t.is_cuda for t in ts):
                torch._foreach_add_(ts, n)
            else:
                for t in ts:
                    t.add_(n)
        return False


def count_batches(counter, n):
    pending = getattr(_TLS, "counters", None)
    if pending is None:
        counter.add_(n)
    else:
        pending.append((counter, n))


AMAX_SLOTS = 64 * 32       # 64 magnitude slots, one per 128-byte line (bn.hip: amax_commit)


_AMAX_ARENA = {}            # device -> [tensor [N, AMAX_SLOTS] int32, next free row]
AMAX_ARENA_ROWS = 192


def amax_arena_reset(device):
    """One fill zeroes a step's worth of magnitude slots (Onet.forward calls this; ~70 sets per training step): new_amax then hands
    out rows instead of launching a fill each."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    # a FRESH block per forward (1.5 MB from the caching allocator: no device malloc in steady state): the rows a forward handed out are
    # read again by its backward (ctx.x_slots: the weight gradient undoes the activation's scale), so a second forward before that backward
    # -- gradient accumulation, another model on the device, an eval pass -- must not zero or re-issue them; the rows keep their block alive
    ar = _AMAX_ARENA[key] = [torch.empty((AMAX_ARENA_ROWS, AMAX_SLOTS), dtype=torch.int32, device=device), 0]
    fill(ar[0].view(torch.float32), 0.0)


def new_amax(device):
    """64 zeroed magnitude slots (8 KB: a cache line each; conv_split.hip: amax_read / amax_scale) for a tensor its producer is
    about to write."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    ar = _AMAX_ARENA.get(key)
    if ar is not None and ar[1] < AMAX_ARENA_ROWS:
        ar[1] += 1
        return ar[0][ar[1] - 1]
    return torch.zeros(AMAX_SLOTS, dtype=torch.int32, device=device)


def absmax_slots(x):
    """Magnitude slots of an existing tensor (one extra pass over it: for callers whose producer did not record them)."""
    require_gpu(x)
    xc = x.contiguous()
    slots = new_amax(x.device)
    _lib.call("onet_absmax_slots", _p(xc), xc.numel(), _p(slots), _stream())
    return slots


def conv3x3_split(x, wq, Cout, out=None, norm=None, amax=None, always=False):
    """z = conv3x3(x) in fp32 accuracy on the 16-bit matrix cores (operands split into two fp16 / bf16 parts, three MFMAs per term).
    norm = save [G, 4, Cin]: x is a pre-activation; the kernel convolves relu(bn(x)), applied in its staging (amax: slots bounding
    that activation, or None).
    fp16 pack: amax = the magnitude slots of x; always = True (input gradients): x is scaled so that its amax lands in [2^13, 2^14)
    -- the slots are then REQUIRED and computed here when the caller has none; always = False: overflow guard only."""
    if wq is None or not wq.is_cuda or wq.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError("conv3x3_split: wq must be a split pack on the GPU (pack3x3_split)")
    f16 = int(wq.dtype == torch.float16)
    require_gpu(x)
    if norm is not None:
        require_gpu(norm)
        x, xbs = plane(x)
        B, Cin, H, W = x.shape
        if out is None:
            out = torch.empty((B, Cout, H, W), dtype=F32, device=x.device)
        e0 = _prof_begin("conv3x3_split_kernel")
        _lib.call("onet_conv3x3_split_fwd_norm", _p(x), xbs, _p(norm), norm.shape[0], _p(wq), f16, _p(amax) if f16 else None, _p(out),
                  out.stride(0) if B > 1 else Cout * H * W, None, B, Cin, Cout, H, W, _stream())
        _prof_end("conv3x3_split_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0, 4.0 * (B * H * W * (Cin + Cout) + 9 * Cin * Cout))
        return out
    x, xbs = plane(x)
    if x.data_ptr() % 16 or xbs % 4:                 # the kernel stages whole float4s: 16-byte aligned image rows
        x = x.contiguous()
        xbs = x.stride(0) if x.shape[0] > 1 else x[0].numel()
    B, Cin, H, W = x.shape
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=F32, device=x.device)
    zbs = out.stride(0) if B > 1 else Cout * H * W
    if f16 and always and amax is None:
        amax = absmax_slots(x)
    e0 = _prof_begin("conv3x3_split_kernel")
    if f16:
        _lib.call("onet_conv3x3_split_conv_amax", _p(x), xbs, _p(amax), int(always), _p(wq), _p(out), zbs, None, B, Cin, Cout, H, W, _stream())
    else:
        _lib.call("onet_conv3x3_split_fwd", _p(x), xbs, _p(wq), 0, _p(out), zbs, B, Cin, Cout, H, W, _stream())
    _prof_end("conv3x3_split_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0, 4.0 * (B * H * W * (Cin + Cout) + 9 * Cin * Cout))
    return out


def split_pack_act(x, f16=True, scale=1.0, out=None, parts=2, slots=None):
    """fp32 NCHW -> the pre-split slot layout of conv_split.hip: [B, C/8, H, 2 (hi | mid), W, 8] fp16 (or bf16) parts of
    scale * x; 4 bytes per element, the fp32 tensor's footprint.  parts = 1: plain bf16, [B, C/8, H, 1, W, 8].
    slots: the tensor's magnitude slots -- x is additionally scaled by their guard scale (2^0 unless the bound reaches 2^15), which
    the consumer undoes from the same slots (what the fused producers do)."""
    require_gpu(x)
    x, xbs = plane(x)
    B, C, H, W = x.shape
    if out is not None:
        parts = out.shape[3]
    if out is None:
        out = torch.empty((B, C // 8, H, parts, W, 8), dtype=torch.float16 if (f16 and parts == 2) else BF, device=x.device)
    _lib.call("onet_split_pack_act", _p(x), xbs, _p(out), _pbs(out), B, C, H, W, 2 if parts == 1 else int(f16), float(scale), _p(slots),
              _stream())
    return out


def conv3x3_split_pre(xs, wq, Cout, out=None, slots=None, always=False, stats=None, slots2=None, split_ch=0, z16=False):
    """z = conv3x3 of a PRE-SPLIT activation xs [B, Cin/8, H, 2, W, 8] (split_pack_act / the producers' fused variants) with the split
    weight pack wq: the arithmetic of conv3x3_split, staging by LDS-DMA.  slots / always: the magnitude slots and rule the producer
    scaled xs by (undone by the kernel; None: unscaled)."""
    if wq is None or not wq.is_cuda or wq.dtype not in (torch.bfloat16, torch.float16) or xs.dtype != wq.dtype:
        raise TypeError("conv3x3_split_pre: xs and wq must be split packs of the same 16-bit type on the GPU")
    B, C8, H, two, W, eight = xs.shape
    f16 = 2 if two == 1 else int(wq.dtype == torch.float16)            # 2: plain bf16, one part
    Cin = C8 * 8
    if out is None:           # z16 (plain bf16 operands only): the output is stored as bf16, rounded once in the epilogue
        out = torch.empty((B, Cout, H, W), dtype=BF if (z16 and two == 1) else F32, device=xs.device)
    e0 = _prof_begin("conv3x3_split_pre_kernel")
    _lib.call("onet_conv3x3_split_fwd_pre", _p(xs), _pbs(xs), _p(slots), int(always), _p(slots2), int(split_ch if slots2 is not None or slots is not None else 0),
              _p(wq), f16, _p(out), _z16(out),
              out.stride(0) if B > 1 else Cout * H * W, _p(stats), B, Cin, Cout, H, W, _stream())
    _prof_end("conv3x3_split_pre_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0,
              B * H * W * (2.0 * two * Cin + out.element_size() * Cout) + 2.0 * two * 9 * Cin * Cout)
    return out


def conv3x3_split_dgrad_pre_bnreduce(dzP, wq, Cout, z_prev, save_prev, slots=None, always=False, want_amax=False):
    """da = input gradient of a DoubleConv's second convolution from pre-split dz (conv3x3_split_pre's arithmetic) with the
    BatchNorm-backward REDUCE of the first unit -- whose output gradient da is -- in the kernel's epilogue: -> (da, rec4, da_amax | None),
    or None where the kernel does not take the shape.  z_prev / save_prev [G, 4, Cout]: the first unit's pre-activation and coefficients
    (G statistics groups = consecutive batch slices).  rec4 [nparts, Cout, 4] is bn_relu_bwd_reduce's record format (_bn_bwd_groups)."""
    if not FUSE_BN_REDUCE or sync_bn() or not FUSE_DGRAD_REDUCE:
        return None
    B, C8, H, two, W, _ = dzP.shape
    Cin = C8 * 8
    G = save_prev.shape[0]
    if tuple(z_prev.shape) != (B, Cout, H, W) or B % G or not save_prev.is_contiguous() or wq.dtype != dzP.dtype:
        return None
    lib = _lib.load()
    nparts = int(lib.onet_conv3x3_split_pre_nparts(B, H, W))
    z_prev, zbs = plane(z_prev)
    if nparts <= 0 or nparts % G or (zbs & 3) or (z_prev.data_ptr() & 15):
        return None
    f16 = 2 if two == 1 else int(wq.dtype == torch.float16)
    da = torch.empty((B, Cout, H, W), dtype=F32, device=dzP.device)
    rec4 = torch.empty((nparts, Cout, 4), dtype=F32, device=dzP.device)
    am = new_amax(dzP.device) if want_amax else None
    e0 = _prof_begin("conv3x3_split_pre_kernel")
    rc = lib.onet_conv3x3_split_dgrad_pre_bnreduce(_p(dzP), _pbs(dzP), _p(slots), int(always), _p(wq), f16, _p(da), Cout * H * W, _p(z_prev), _z16(z_prev), zbs,
                                                   _p(save_prev), B // G if G > 1 else 0, _p(rec4), _p(am), B, Cin, Cout, H, W, _stream())
    _prof_end("conv3x3_split_pre_kernel", 2.0 * B * H * W * Cin * Cout * 9 if rc == 0 else 0.0, e0,
              (B * H * W * (2.0 * two * Cin + (4.0 + z_prev.element_size()) * Cout) + 2.0 * two * 9 * Cin * Cout) if rc == 0 else 0.0)
    if rc < 0:
        raise _lib.OnetHipError(f"onet_conv3x3_split_dgrad_pre_bnreduce failed ({rc}): {_lib.last_error()}")
    return (da, rec4, am) if rc == 0 else None


def eval_layer_ok(B, Cin, Cout, H, W):
    """Does the fused eval plan (onet_amd/inference.py) take a 3x3 convolution layer (Cin -> Cout on B maps of H x W) on pre-split
    operands?  Yes wherever today's eval dispatch selects the in-staging split kernel for the layer and the shape lies in the domain
    of onet_conv3x3_split_fwd_pre_act: fp16 (hi | mid) parts, maps made of full 16 x 32 tiles, Cin % 16 == 0, Cout % 64 == 0.  A
    function of shapes, settings and -- through conv3x3_algo's tile threshold -- the current device's compute-unit count (n_cu): no
    tensor is looked at, nothing is launched, but the fused depth of a small batch can differ between devices."""
    return _eval_domain("fp16x2", "full", B, Cin, Cout, H, W)


def _eval_domain(fmt, mode, B, Cin, Cout, H, W):
    """Does a 3x3 convolution layer lie in the domain the fused eval plan gives the entry points of slot format `fmt` on a level of `mode`
    (EVAL_ENTRIES), and does the dispatch want it there?  The eval_layer_ok* predicates are this function and their chains: each mode's
    rule covers the maps that mode ADDS ("anymap": outside the ragged domain; "pairs": the caller has W <= 16; fp16 "ragged": the caller
    has sent maps made of full tiles to "full").  The floors are read at call time (tests and tools reassign them)."""
    fp16 = fmt == "fp16x2"
    # storage, channel multiples
    if not presplit() or (fp16 and p16_parts() != 2) or Cin % (16 if fp16 else 32) or Cout % 64:
        return False
    # the mode's maps, above its width floor
    if mode == "full":
        map_ok = full_tiles(H, W) and H * W < 2 ** 24
    elif mode == "ragged":
        map_ok = W > 16 and _ragged_map(H, W) and (W >= RAGGED_MIN_W or full_tiles(H, W))
    elif mode == "anymap":
        map_ok = H > 0 and W > 16 and W >= max(RAGGED_MIN_W, ANYMAP_MIN_W) and H * W < 2 ** 24 and not _ragged_map(H, W)
    else:
        map_ok = B > 0 and H > 0 and W >= max(PAIRS_MIN_W, 1)
    if not map_ok:
        return False
    # fill rule.  fp16 levels of whole images: wherever today's dispatch selects the split kernel (which asks the buffer-resource range
    # itself); elsewhere inside that range, every layer under the format's own conv settings, else tiles >= 3/4 of the compute units
    if fp16 and mode != "pairs":
        return conv3x3_algo(B, Cin, Cout, H, W) == "split"
    if not _in_buffer_range(Cin, Cout, H, W):
        return False
    if conv_algo() in (("split",) if fp16 else ("bf16", "split")):
        return True
    # (cdiv: a partly filled tile occupies a compute unit like a full one; a pair tile holds two images)
    tiles = -(-B // 2) * -(-H // 16) if mode == "pairs" else B * -(-H // 16) * -(-W // 32)
    return tiles * (Cout // 64) >= (n_cu() * 3) // 4


def eval_layer_ok_bf16(B, Cin, Cout, H, W):
    """eval_layer_ok for the one-part plan (Settings.fused_eval = "bf16"): the domain of onet_conv3x3_plain16_fwd_pre_act -- maps made of
    full 16 x 32 tiles, Cin % 32 == 0, Cout % 64 == 0 -- inside the buffer-resource range, with pre-split storage on.  Under conv in
    ("bf16", "split") every such layer is taken, as those settings take every legal layer of their own kernels; otherwise conv3x3_algo's
    fill rule decides (tiles >= 3/4 of the compute units; smaller layers stay on the existing eval kernels).  A function of shapes,
    settings and n_cu()."""
    return _eval_domain("bf16", "full", B, Cin, Cout, H, W)


def full_tiles(H, W):
    """Is an H x W map made of full 16 x 32 tiles -- the domain of the fused eval entry points without `_ragged`?"""
    return W >= 32 and W % 32 == 0 and H % 16 == 0


def _ragged_map(H, W):
    """The maps the *_ragged entry points take (include/onet_hip_ragged.h)"""
    return H > 0 and W > 0 and H % 2 == 0 and W % 4 == 0 and H * W < 2 ** 24


# The narrowest map that is not made of full tiles which eval_layer_ok_ragged takes (ONET_FLAGS / tools: 32, 64, 128 leave the 28-, 56-,
# 112-pixel level of a 224 x 224 input to the fall-back -- tools/time_ragged_eval.py times the plan level by level with it).
# eval_layer_ok_ragged_fp16 keeps the same floor (tools/time_ragged_fp16_eval.py: every level is faster fused on that format too)
RAGGED_MIN_W = int(_FLAGS.get("RAGGED_MIN_W", 20))


def eval_layer_ok_ragged(B, Cin, Cout, H, W):
    """eval_layer_ok_bf16 for Settings.fused_eval = "bf16+pool+ragged": the domain of onet_conv3x3_plain16_fwd_pre_act_ragged -- even H
    and W (every fused level is then pooled and up-sampled without pad offsets, and a 2 x 2 window never straddles the map's edge),
    W % 4 == 0 (the float4 accesses of L, z and the fp32 activation), Cin % 32 == 0, Cout % 64 == 0, inside the buffer-resource range,
    with pre-split storage on.  conv in ("bf16", "split"): every such layer; otherwise conv3x3_algo's fill rule on the tile counts the
    kernel walks (cdiv: a partly filled tile occupies a compute unit like a full one).  On a map made of full tiles the answer is
    eval_layer_ok_bf16's.  Narrower than the entry points' domain by one rule: W >= RAGGED_MIN_W = 20, that is W > 16 -- a map 16 pixels
    wide or narrower fills at most half of every tile's columns (the existing dispatch's own special case: image pairs), is left to the
    fall-back levels, and so the plan of an input made of full tiles (256 x 256: its 16-pixel level) stays the plan of "bf16+pool"."""
    return _eval_domain("bf16", "ragged", B, Cin, Cout, H, W)


# The narrowest map outside eval_layer_ok_ragged's domain (odd H or W, W % 4 != 0) that eval_layer_ok_anymap takes: the floor of the ragged
# levels unless set apart (ONET_FLAGS / tools/time_anymap_eval.py: 26 leaves the 25-pixel level of a 200 x 200 input to the fall-back)
ANYMAP_MIN_W = int(_FLAGS.get("ANYMAP_MIN_W", RAGGED_MIN_W))


def eval_layer_ok_anymap(B, Cin, Cout, H, W):
    """eval_layer_ok_ragged for the levels below the first of Settings.fused_eval = "bf16+pool+anymap": wherever that predicate says yes,
    yes; besides, the domain of onet_conv3x3_plain16_fwd_pre_act_anymap -- ANY H and W, odd included (the kernel's fp32 side outputs
    are stored float by float, pooling rounds down as nn.MaxPool2d(2) does) -- above the same width floor (W > 16, W >= RAGGED_MIN_W
    and ANYMAP_MIN_W), Cin % 32 == 0, Cout % 64 == 0, inside the buffer-resource range, with pre-split storage on, under the same fill
    rule on cdiv tile counts."""
    return eval_layer_ok_ragged(B, Cin, Cout, H, W) or _eval_domain("bf16", "anymap", B, Cin, Cout, H, W)


# The narrowest map eval_layer_ok_pairs takes: a map of 8 or fewer columns fills at most half of each image's half of a pair tile -- the
# argument of the W > 16 rule above, one size down (four images per tile would be the answer there), not a measurement
PAIRS_MIN_W = int(_FLAGS.get("PAIRS_MIN_W", 9))
# tools/time_pairs_eval.py's diagnostic: the maps eval_layer_ok_pairs adds are launched one image per (half-empty) tile by the any-map
# entry -- what pairing itself is worth
PAIRS_SINGLE = _flag("PAIRS_SINGLE", False)


def eval_layer_ok_pairs(B, Cin, Cout, H, W):
    """eval_layer_ok_anymap for level 4 of Settings.fused_eval = "bf16+pool+anymap+pairs": on W > 16 that predicate's answer; on
    PAIRS_MIN_W <= W <= 16 the domain of onet_conv3x3_plain16_fwd_pre_act_pairs -- any H > 0, Cin % 32 == 0, Cout % 64 == 0, inside the
    buffer-resource range, with pre-split storage on.  conv in ("bf16", "split"): every such layer; otherwise the fill rule on the tiles
    the kernel walks, which hold two images each: cdiv(B, 2) cdiv(H, 16) Cout / 64 >= 3/4 n_cu."""
    if W > 16:
        return eval_layer_ok_anymap(B, Cin, Cout, H, W)
    return _eval_domain("bf16", "pairs", B, Cin, Cout, H, W)


def eval_layer_ok_ragged_fp16(B, Cin, Cout, H, W):
    """eval_layer_ok for Settings.fused_eval = "fp16x2+ragged": the domain of onet_conv3x3_split_fwd_pre_act_ragged -- fp16 (hi | mid)
    parts with pre-split storage, Cin % 16 == 0, Cout % 64 == 0, even H and W % 4 == 0 (_ragged_map: the kernel's own slot stores are
    per pixel, but the stem's and the `pack` route's passes, the head's float4 accesses and the fall-back levels need W % 4) -- where
    today's dispatch selects the split kernel (conv3x3_algo: its fill rule counts tiles by cdiv).  On a map made of full tiles the
    answer is eval_layer_ok's.  A map that is not must be wider than 16 pixels and no narrower than RAGGED_MIN_W (eval_layer_ok_ragged's
    floor: a 256 x 256 input keeps the plan of "fp16x2+pool")."""
    if full_tiles(H, W):
        return eval_layer_ok(B, Cin, Cout, H, W)
    return _eval_domain("fp16x2", "ragged", B, Cin, Cout, H, W)


def eval_layer_ok_pairs_fp16(B, Cin, Cout, H, W):
    """eval_layer_ok_ragged_fp16 for level 4 of Settings.fused_eval = "fp16x2+ragged+pairs": on W > 16 that predicate's answer; on
    PAIRS_MIN_W <= W <= 16 the domain of onet_conv3x3_split_fwd_pre_act_pairs -- fp16 (hi | mid) parts with pre-split storage, any H > 0,
    Cin % 16 == 0, Cout % 64 == 0, inside the buffer-resource range.  conv == "split": every such layer; otherwise the fill rule on the
    tiles the kernel walks, which hold two images each: cdiv(B, 2) cdiv(H, 16) Cout / 64 >= 3/4 n_cu."""
    if W > 16:
        return eval_layer_ok_ragged_fp16(B, Cin, Cout, H, W)
    return _eval_domain("fp16x2", "pairs", B, Cin, Cout, H, W)


def conv3x3_act_bound(weight, save, x_amax, x_amax2=None, split_ch=0):
    """Magnitude slots bounding relu(bn_eval(conv3x3(x))) from the layer's weights, the coefficients `save` [4, Cout] and the magnitude
    slots of x (two producers of a concat buffer: x_amax2 for the channels from split_ch): the scale slots of the fused eval kernel."""
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    slots = new_amax(w.device)
    _lib.call("onet_conv3x3_act_bound", _p(w), w.shape[0], w.shape[1], _p(save), _p(x_amax), _p(x_amax2), int(split_ch if x_amax2 is not None else 0),
              _p(slots), _stream())
    return slots


# The fused eval convolutions (onet_amd/inference.py): (slot format, level mode, epilogue) -> (C entry, profile kind).  Slot format:
# "fp16x2" (fp16 hi | mid parts, include/onet_hip_eval.h) | "bf16" (one part of plain bf16); level mode: "full" (maps made of full 16 x 32
# tiles) | "ragged" (even H, W % 4 == 0: onet_hip_ragged.h, onet_hip_ragged_split.h) | "anymap" (any H and W: onet_hip_anymap.h) | "pairs"
# (image-pair tiles, 0 < W <= 16: onet_hip_pairs.h, onet_hip_split_pairs.h); epilogue: "act" (BatchNorm + ReLU, slots out) | "act_pool" (...
# and the 2 x 2 max-pooling) | "head" (... times L, summed over the 64 channels: V alone) | "plain" (fp32 z).  A combination that is not
# a row does not exist: eval_conv raises KeyError, the plan (inference._launch) says which level asked for it.  Every row has a binding by
# name below (eval_conv_name): conv3x3_{plain16,split}_pre_<epilogue>[_<mode>].
EVAL_ENTRIES = {
    ("fp16x2", "full", "act"): ("onet_conv3x3_split_fwd_pre_act", "conv3x3_split_pre_act_kernel"),
    ("fp16x2", "full", "act_pool"): ("onet_conv3x3_split_fwd_pre_act_pool", "conv3x3_split_pre_act_pool_kernel"),
    ("fp16x2", "full", "head"): ("onet_conv3x3_split_fwd_pre_head", "conv3x3_split_pre_head_kernel"),
    ("fp16x2", "ragged", "act"): ("onet_conv3x3_split_fwd_pre_act_ragged", "conv3x3_split_pre_act_kernel"),
    ("fp16x2", "ragged", "act_pool"): ("onet_conv3x3_split_fwd_pre_act_pool_ragged", "conv3x3_split_pre_act_pool_kernel"),
    ("fp16x2", "ragged", "head"): ("onet_conv3x3_split_fwd_pre_head_ragged", "conv3x3_split_pre_head_kernel"),
    ("fp16x2", "ragged", "plain"): ("onet_conv3x3_split_fwd_pre_plain_ragged", "conv3x3_split_pre_kernel"),
    ("fp16x2", "pairs", "act"): ("onet_conv3x3_split_fwd_pre_act_pairs", "conv3x3_split_pre_act_pairs_kernel"),
    ("bf16", "full", "act"): ("onet_conv3x3_plain16_fwd_pre_act", "conv3x3_pre16_act_kernel"),
    ("bf16", "full", "act_pool"): ("onet_conv3x3_plain16_fwd_pre_act_pool", "conv3x3_pre16_act_pool_kernel"),
    ("bf16", "full", "head"): ("onet_conv3x3_plain16_fwd_pre_head", "conv3x3_pre16_head_kernel"),
    ("bf16", "ragged", "act"): ("onet_conv3x3_plain16_fwd_pre_act_ragged", "conv3x3_pre16_act_kernel"),
    ("bf16", "ragged", "act_pool"): ("onet_conv3x3_plain16_fwd_pre_act_pool_ragged", "conv3x3_pre16_act_pool_kernel"),
    ("bf16", "ragged", "head"): ("onet_conv3x3_plain16_fwd_pre_head_ragged", "conv3x3_pre16_head_kernel"),
    ("bf16", "ragged", "plain"): ("onet_conv3x3_plain16_fwd_pre_plain_ragged", "conv3x3_split_pre_kernel"),
    ("bf16", "anymap", "act"): ("onet_conv3x3_plain16_fwd_pre_act_anymap", "conv3x3_pre16_act_kernel"),
    ("bf16", "anymap", "act_pool"): ("onet_conv3x3_plain16_fwd_pre_act_pool_anymap", "conv3x3_pre16_act_pool_kernel"),
    ("bf16", "pairs", "act"): ("onet_conv3x3_plain16_fwd_pre_act_pairs", "conv3x3_pre16_act_pairs_kernel"),
}


_EVAL_NAMES = {key: entry[len("onet_"):].replace("_fwd_pre_", "_pre_") for key, (entry, _) in EVAL_ENTRIES.items()}


def eval_conv_name(fmt, mode, epilogue):
    """The name in this module of the binding of EVAL_ENTRIES[fmt, mode, epilogue] (the C entry's, without onet_ and _fwd) -- None: no row"""
    return _EVAL_NAMES.get((fmt, mode, epilogue))


def eval_conv(fmt, mode, epilogue, xs, wq, Cout, save=None, L=None, aP_slots=None, out=None, slots=None, slots2=None, split_ch=0,
              a_amax=None, a=None, yP=None, y=None):
    """The launch of EVAL_ENTRIES[fmt, mode, epilogue] on the slots xs with the weight pack wq: what the conv3x3_{plain16,split}_pre_*
    functions below are bindings of, where each argument is described.  save: every epilogue but "plain"; L: "head"; aP_slots, slots,
    slots2, split_ch: the magnitude slots of "fp16x2"; a_amax, a: "act" / "act_pool" (a_amax: not on the one-part ragged, any-map and pair
    entries); yP, y: "act_pool".  -> the output (slots, V or z), or None where the entry does not take the shape (nothing launched)."""
    entry, kind = EVAL_ENTRIES[fmt, mode, epilogue]
    two = fmt == "fp16x2"
    dt = torch.float16 if two else BF
    if wq is None or not wq.is_cuda or wq.dtype != dt or xs.dtype != dt or xs.shape[3] != 1 + two:
        raise TypeError(f"{eval_conv_name(fmt, mode, epilogue)}: xs and wq must be " + ("fp16 (hi | mid) split" if two else "one-part bf16") + " packs on the GPU")
    if PAIRS_SINGLE and (fmt, mode) == ("bf16", "pairs"):
        mode = "anymap"
        entry, kind = EVAL_ENTRIES[fmt, mode, epilogue]
    # (fp16: the magnitude slots the producers scaled xs by -- one set, or two with the first channel of the second)
    x_slots = (_p(slots), 0, _p(slots2), int(split_ch if slots2 is not None or slots is not None else 0)) if two else ()
    if epilogue == "head":
        return _pre_head(entry, kind, 1 + two, xs, wq, Cout, save, L, out, x_slots)
    if epilogue == "plain":
        return _pre_plain(entry, kind, 1 + two, xs, wq, Cout, out, x_slots)
    return _pre_act(entry, kind, 1 + two, mode, xs, wq, Cout, save, out, a_amax, a, x_slots, (_p(aP_slots),) if two else (),
                    pooled=(yP, y) if epilogue == "act_pool" else None)


def _pre_act(entry, kind, two, mode, xs, wq, Cout, save, out, a_amax, a, extra_in, extra_out, pooled=None):
    """pooled: (yP, y) of the _pool entries -- the pooled slots and / or the pooled fp32 tensor, at least one"""
    B, C8, H, _, W, _ = xs.shape
    Cin = C8 * 8
    if pooled is not None and pooled[0] is None and pooled[1] is None:
        raise ValueError(f"{entry[len('onet_'):]}: a pooled destination is required (yP, y or both)")
    if mode in ("anymap", "pairs"):         # every map below 2^24 pixels; pairs: any H on 0 < W <= 16
        map_ok = 0 < H * W < 2 ** 24 and (mode == "anymap" or W <= 16)
    else:
        map_ok = _ragged_map(H, W) if mode == "ragged" else full_tiles(H, W)
    if not map_ok or Cin % (16 if two == 2 else 32) or Cout % 64:
        return None
    if out is None:
        out = p16_empty(B, Cout, H, W, xs.device, parts=two)
    n = Cout * H * W
    pool_args, pool_bytes = (), 0.0
    if pooled is not None:
        yP, y = pooled
        pool_args = (_p(yP), 0 if yP is None else _pbs(yP), _p(y), 0 if y is None else (y.stride(0) if B > 1 else Cout * (H // 2) * (W // 2)))
        pool_bytes = 0.25 * (2.0 * two * (yP is not None) + 4.0 * (y is not None)) * Cout      # per pixel: a quarter as many pooled ones
    e0 = _prof_begin(kind)
    rc = getattr(_lib.load(), entry)(_p(xs), _pbs(xs), *extra_in, _p(wq), _p(save), _p(out), _pbs(out), *extra_out, _p(a_amax), _p(a),
                                     0 if a is None else (a.stride(0) if B > 1 else n), *pool_args, B, Cin, Cout, H, W, _stream())
    _prof_end(kind, 2.0 * B * H * W * Cin * Cout * 9 if rc == 0 else 0.0, e0,
              (B * H * W * (2.0 * two * Cin + (2.0 * two + 4.0 * (a is not None)) * Cout + pool_bytes) + 2.0 * two * 9 * Cin * Cout) if rc == 0 else 0.0)
    if rc < 0:
        raise _lib.OnetHipError(f"{entry} failed ({rc}): {_lib.last_error()}")
    return out if rc == 0 else None


def _pre_head(entry, kind, two, xs, wq, Cout, save, L, out, extra):
    name = entry[len("onet_"):]
    B, C8, H, _, W, _ = xs.shape
    Cin = C8 * 8
    if tuple(L.shape) != (B, Cout, H, W) or L.dtype != F32:
        raise ValueError(f"{name}: L must be an fp32 [B, Cout, H, W] tensor of the convolution's output shape")
    L, lbs = plane(L)
    if out is None:
        out = torch.empty((B, 1, H, W), dtype=F32, device=xs.device)
    elif tuple(out.shape) != (B, 1, H, W) or out.dtype != F32 or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous fp32 [B, 1, H, W] tensor")
    e0 = _prof_begin(kind)
    rc = getattr(_lib.load(), entry)(_p(xs), _pbs(xs), *extra, _p(wq), _p(save), _p(L), lbs, _p(out), B, Cin, Cout, H, W, _stream())
    _prof_end(kind, 2.0 * B * H * W * Cin * Cout * 9 if rc == 0 else 0.0, e0,
              (B * H * W * (2.0 * two * Cin + 4.0 * Cout + 4.0) + 2.0 * two * 9 * Cin * Cout) if rc == 0 else 0.0)
    if rc < 0:
        raise _lib.OnetHipError(f"{entry} failed ({rc}): {_lib.last_error()}")
    return out if rc == 0 else None


def _pre_plain(entry, kind, two, xs, wq, Cout, out, extra):
    B, C8, H, _, W, _ = xs.shape
    Cin = C8 * 8
    if not _ragged_map(H, W) or Cin % (16 if two == 2 else 32) or Cout % 64:
        return None
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=F32, device=xs.device)
    e0 = _prof_begin(kind)
    rc = getattr(_lib.load(), entry)(_p(xs), _pbs(xs), *extra, _p(wq), _p(out), out.stride(0) if B > 1 else Cout * H * W, B, Cin, Cout, H, W,
                                     _stream())
    _prof_end(kind, 2.0 * B * H * W * Cin * Cout * 9 if rc == 0 else 0.0, e0,
              (B * H * W * (2.0 * two * Cin + 4.0 * Cout) + 2.0 * two * 9 * Cin * Cout) if rc == 0 else 0.0)
    if rc < 0:
        raise _lib.OnetHipError(f"{entry} failed ({rc}): {_lib.last_error()}")
    return out if rc == 0 else None


# ---- the table's rows by name: one-part bf16 operands
def conv3x3_plain16_pre_act(xs, wq, Cout, save, out=None, a_amax=None, a=None):
    """aP = relu(bn(conv3x3(xs))) on PLAIN bf16 operands (xs [B, Cin/8, H, 1, W, 8] bf16, wq the plain16 forward pack), written as one
    part of bf16 slots, BatchNorm with the fixed coefficients `save` [4, Cout] (bn_eval_coeffs) in the convolution's epilogue:
    conv3x3_split_pre (fp32 z) followed by bn_relu_apply_split, bit for bit, without the tensor z.  Unscaled: no magnitude slots.
    a_amax: slots that receive the exact max a; a: optional fp32 destination.  -> aP, or None where the kernel does not take the shape
    (nothing launched)."""
    return eval_conv("bf16", "full", "act", xs, wq, Cout, save, out=out, a_amax=a_amax, a=a)


def conv3x3_plain16_pre_act_ragged(xs, wq, Cout, save, out=None, a=None):
    """conv3x3_plain16_pre_act on a ragged map (even H, W % 4 == 0; onet_conv3x3_plain16_fwd_pre_act_ragged): on the map, value for value,
    what conv3x3_plain16_pre_act writes on the map zero-padded to whole 16 x 32 tiles; nothing outside the map is written.  No exact
    maximum is recorded.  -> aP, or None where the kernel does not take the shape (nothing launched)."""
    return eval_conv("bf16", "ragged", "act", xs, wq, Cout, save, out=out, a=a)


def conv3x3_plain16_pre_act_pool_ragged(xs, wq, Cout, save, out=None, a=None, yP=None, y=None):
    """conv3x3_plain16_pre_act_pool on a ragged map (conv3x3_plain16_pre_act_ragged's domain): the pooled maps are H / 2 x W / 2.
    -> aP, or None (nothing launched)."""
    return eval_conv("bf16", "ragged", "act_pool", xs, wq, Cout, save, out=out, a=a, yP=yP, y=y)


def conv3x3_plain16_pre_act_anymap(xs, wq, Cout, save, out=None, a=None):
    """conv3x3_plain16_pre_act_ragged on a map of ANY H and W (onet_conv3x3_plain16_fwd_pre_act_anymap): on the map, value for value, what
    conv3x3_plain16_pre_act writes on the map zero-padded to whole 16 x 32 tiles; nothing outside the map is written, and `a` needs no
    row alignment.  On a map the ragged entry takes: that entry's launch.  -> aP, or None (nothing launched)."""
    return eval_conv("bf16", "anymap", "act", xs, wq, Cout, save, out=out, a=a)


def conv3x3_plain16_pre_act_pairs(xs, wq, Cout, save, out=None, a=None):
    """conv3x3_plain16_pre_act_anymap on maps of 0 < W <= 16 and any H, on IMAGE-PAIR tiles (onet_conv3x3_plain16_fwd_pre_act_pairs): two
    images of the batch side by side in a tile's 32 columns; the same values.  Any batch size (an odd one: the last tile holds one
    image).  -> aP, or None where the kernel does not take the shape (nothing launched).  (PAIRS_SINGLE: the any-map entry's launch.)"""
    return eval_conv("bf16", "pairs", "act", xs, wq, Cout, save, out=out, a=a)


def conv3x3_plain16_pre_act_pool_anymap(xs, wq, Cout, save, out=None, a=None, yP=None, y=None):
    """conv3x3_plain16_pre_act_pool_ragged on a map of ANY H and W (onet_conv3x3_plain16_fwd_pre_act_pool_anymap): the pooled maps are
    H // 2 x W // 2 -- floor pooling, nn.MaxPool2d(2)'s; a window partly outside an odd map is pooled nowhere.  -> aP, or None."""
    return eval_conv("bf16", "anymap", "act_pool", xs, wq, Cout, save, out=out, a=a, yP=yP, y=y)


def conv3x3_plain16_pre_plain_ragged(xs, wq, Cout, out=None):
    """z = conv3x3 (fp32) of one-part bf16 slots on a ragged map (conv3x3_plain16_pre_act_ragged's domain): conv3x3_split_pre's launch
    there.  -> z, or None (nothing launched)."""
    return eval_conv("bf16", "ragged", "plain", xs, wq, Cout, out=out)


def conv3x3_plain16_pre_act_pool(xs, wq, Cout, save, out=None, a_amax=None, a=None, yP=None, y=None):
    """conv3x3_plain16_pre_act with the 2 x 2 max-pooling of the activation in the same epilogue: besides aP (`out`: the skip groups of a
    concat buffer qualify), `a` and `a_amax` the launch writes the pooled tensor as one-part bf16 slots (yP [B, Cout/8, H/2, 1, W/2, 8]),
    as fp32 (y [B, Cout, H/2, W/2]) or both -- at least one.  conv3x3_split_pre (fp32 z) followed by bn_relu_apply_pool_split, bit for
    bit, without the tensor z.  -> aP, or None where the kernel does not take the shape (nothing launched)."""
    return eval_conv("bf16", "full", "act_pool", xs, wq, Cout, save, out=out, a_amax=a_amax, a=a, yP=yP, y=y)


def conv3x3_plain16_pre_head(xs, wq, Cout, save, L, out=None):
    """V [B, 1, H, W] = sum_c L[c] relu(bn(conv3x3(xs)))[c] on PLAIN bf16 operands (conv3x3_plain16_pre_act's), the model's last unit
    with the head's channel product in the convolution's epilogue: neither the pre-activation nor the activation is written.  `save`
    [4, Cout] (bn_eval_coeffs); L: fp32 [B, Cout, H, W], a batch slice of a larger tensor qualifies; out: optional contiguous
    destination.  The accumulators are those of conv3x3_split_pre's launch bit for bit; the channel sum runs in the kernel's own fixed
    order.  -> V, or None where the kernel does not take the shape (Cout != 64, maps not made of full 16 x 32 tiles, Cin % 32: nothing
    launched, nothing written)."""
    return eval_conv("bf16", "full", "head", xs, wq, Cout, save, L, out=out)


def conv3x3_plain16_pre_head_ragged(xs, wq, Cout, save, L, out=None):
    """conv3x3_plain16_pre_head on a ragged map (conv3x3_plain16_pre_act_ragged's domain, Cout == 64).  -> V, or None (nothing launched,
    nothing written)."""
    return eval_conv("bf16", "ragged", "head", xs, wq, Cout, save, L, out=out)


# ---- fp16 (hi | mid) operands.  slots / slots2 / split_ch: the magnitude slots the producers scaled xs by
def conv3x3_split_pre_act(xs, wq, Cout, save, aP_slots, out=None, slots=None, slots2=None, split_ch=0, a_amax=None, a=None):
    """aP = relu(bn(conv3x3(xs))) written PRE-SPLIT, BatchNorm with the fixed coefficients `save` [4, Cout] (bn_eval_coeffs) in the
    convolution's epilogue: conv3x3_split_pre followed by bn_relu_apply_split(.., slots=aP_slots), bit for bit, without the tensor z.
    aP_slots: the bound the parts are scaled by (conv3x3_act_bound, before this launch); a_amax: slots that receive the exact max a;
    a: optional fp32 destination.  -> aP, or None where the kernel does not take the shape (nothing launched)."""
    return eval_conv("fp16x2", "full", "act", xs, wq, Cout, save, None, aP_slots, out, slots, slots2, split_ch, a_amax, a)


def conv3x3_split_pre_act_ragged(xs, wq, Cout, save, aP_slots, out=None, slots=None, slots2=None, split_ch=0, a_amax=None, a=None):
    """conv3x3_split_pre_act on a ragged map (even H, W % 4 == 0; onet_conv3x3_split_fwd_pre_act_ragged): on the map, value for value,
    what conv3x3_split_pre_act writes on the map zero-padded to whole 16 x 32 tiles; nothing outside the map is written.  a_amax: the
    exact maximum over the MAP's pixels (bit-equal to a.max() of the same launch).  -> aP, or None (nothing launched)."""
    return eval_conv("fp16x2", "ragged", "act", xs, wq, Cout, save, None, aP_slots, out, slots, slots2, split_ch, a_amax, a)


def conv3x3_split_pre_act_pairs(xs, wq, Cout, save, aP_slots, out=None, slots=None, slots2=None, split_ch=0, a_amax=None, a=None):
    """conv3x3_split_pre_act_ragged on maps of 0 < W <= 16 and any H, on IMAGE-PAIR tiles (onet_conv3x3_split_fwd_pre_act_pairs): two
    images of the batch side by side in a tile's 32 columns; the same values, a_amax the exact maximum over the map's pixels of the
    batch's own images.  Any batch size (an odd one: the last tile holds one image).  -> aP, or None where the kernel does not take
    the shape (nothing launched)."""
    return eval_conv("fp16x2", "pairs", "act", xs, wq, Cout, save, None, aP_slots, out, slots, slots2, split_ch, a_amax, a)


def conv3x3_split_pre_act_pool(xs, wq, Cout, save, aP_slots, out=None, slots=None, slots2=None, split_ch=0, a_amax=None, a=None, yP=None,
                               y=None):
    """conv3x3_split_pre_act with the 2 x 2 max-pooling of the activation in the same epilogue (conv3x3_plain16_pre_act_pool on fp16
    hi | mid parts): the pooled slots yP [B, Cout/8, H/2, 2, W/2, 8] are parts of 2^k m with the k of aP (aP_slots).  conv3x3_split_pre
    followed by bn_relu_apply_pool_split(.., slots=aP_slots), bit for bit.  -> aP, or None (nothing launched)."""
    return eval_conv("fp16x2", "full", "act_pool", xs, wq, Cout, save, None, aP_slots, out, slots, slots2, split_ch, a_amax, a, yP, y)


def conv3x3_split_pre_act_pool_ragged(xs, wq, Cout, save, aP_slots, out=None, slots=None, slots2=None, split_ch=0, a_amax=None, a=None,
                                      yP=None, y=None):
    """conv3x3_split_pre_act_pool on a ragged map (even H, W % 4 == 0; onet_conv3x3_split_fwd_pre_act_pool_ragged): the pooled maps are
    H / 2 x W / 2; a_amax receives the maximum over the map's own pixels.  -> aP, or None (nothing launched)."""
    return eval_conv("fp16x2", "ragged", "act_pool", xs, wq, Cout, save, None, aP_slots, out, slots, slots2, split_ch, a_amax, a, yP, y)


def conv3x3_split_pre_head(xs, wq, Cout, save, L, out=None, slots=None, slots2=None, split_ch=0):
    """conv3x3_plain16_pre_head on fp16 (hi | mid) parts (conv3x3_split_pre_act's operands).  The convolution runs on the 16x16x32
    kernel: its accumulators agree with conv3x3_split_pre's (the 32x32x16 kernel) to fp32 accumulation order.  -> V, or None
    (Cout != 64, maps not made of full tiles, Cin % 16)."""
    return eval_conv("fp16x2", "full", "head", xs, wq, Cout, save, L, None, out, slots, slots2, split_ch)


def conv3x3_split_pre_head_ragged(xs, wq, Cout, save, L, out=None, slots=None, slots2=None, split_ch=0):
    """conv3x3_split_pre_head on a ragged map (conv3x3_split_pre_act_ragged's domain, Cout == 64).  -> V, or None (nothing launched,
    nothing written)."""
    return eval_conv("fp16x2", "ragged", "head", xs, wq, Cout, save, L, None, out, slots, slots2, split_ch)


def conv3x3_split_pre_plain_ragged(xs, wq, Cout, out=None, slots=None, slots2=None, split_ch=0):
    """z = conv3x3 (fp32) of fp16 (hi | mid) slots on a ragged map (conv3x3_split_pre_act_ragged's domain): conv3x3_split_pre's launch
    there.  -> z, or None (nothing launched)."""
    return eval_conv("fp16x2", "ragged", "plain", xs, wq, Cout, out=out, slots=slots, slots2=slots2, split_ch=split_ch)


FUSE_DGRAD_REDUCE = _flag("FUSE_DGRAD_REDUCE", True)      # False (tests / A-B): the first unit of a DoubleConv runs its own BatchNorm-backward reduce pass


def conv3x3_split_wgrad_pre(xs, dzs, dw_shape, out=None, x_slots=None, dz_slots=None, x_slots2=None, split_ch=0):
    """Weight gradient of a 3x3 convolution from PRE-SPLIT x and dz (split_pack_act layout, same 16-bit type):
    conv3x3_split_wgrad's arithmetic with LDS-DMA staging and transposed fragment reads; x_slots / dz_slots: the magnitude slots the
    producers scaled the operands by (undone on the result)."""
    if xs.dtype != dzs.dtype or xs.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError("conv3x3_split_wgrad_pre: xs and dzs must be pre-split tensors of the same 16-bit type")
    B, C8, H, two, W, eight = xs.shape
    Cin, Cout = C8 * 8, dzs.shape[1] * 8
    assert tuple(dw_shape) == (Cout, Cin, 3, 3) and dzs.shape[3] == two
    dw = out if out is not None else torch.empty(dw_shape, dtype=F32, device=xs.device)
    need = _lib.load().onet_conv3x3_split_wgrad_ws_bytes(B, Cin, Cout, H, W)
    ws = workspace(need, xs.device)
    e0 = _prof_begin("conv3x3_split_wgrad_pre_kernel")
    _lib.call("onet_conv3x3_split_wgrad_pre", _p(xs), _pbs(xs), _p(x_slots), _p(x_slots2), int(split_ch), _p(dzs),
              _pbs(dzs), _p(dz_slots), 2 if two == 1 else int(xs.dtype == torch.float16), _p(dw), _p(ws),
              ws.numel() * 4, B, Cin, Cout, H, W, 0, _stream())
    _prof_end("conv3x3_split_wgrad_pre_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0,
              2.0 * two * B * H * W * (Cin + Cout) + 4.0 * 9 * Cin * Cout)
    return dw


# ----------------------------------------------------------------------------- pre-split storage (Settings.presplit)
def pre_layer_ok(B, Cin, Cout, H, W):
    """Can a 3x3 convolution layer (Cin -> Cout on B maps of H x W) run ALL THREE of its kernels on pre-split operands -- forward and
    input gradient by conv3x3_split_pre_kernel, weight gradient by conv3x3_split_wgrad_pre_kernel?  Producers write the pre-split
    form of a tensor only where this says yes for its consumer (the decision is a function of shapes and settings, so producer and
    consumer agree without talking)."""
    if not presplit() or Cin % 16 or Cout % 16 or W < 16 or (W % 32 and W != 16) or H % 16 or H * W >= 2 ** 24:
        return False
    np_ = p16_parts()
    if np_ == 1 and (Cin % 32 or Cout % 32):                         # plain bf16: 32-channel chunks
        return False
    if W <= 32 and B * max(Cin, Cout) * H * W * 2 * np_ >= 2 ** 31:  # weight-gradient units pair images: one buffer resource over the batch
        return False
    lib = _lib.load()
    if W == 16:
        # the 16-pixel level: two images side by side per forward tile, four per weight-gradient unit; worth it once the tiles fill
        # the chip (the dispatch of the fp32-operand kernels has no split kernel for this width, so the decision is made here)
        return PRESPLIT_W16 and B % 4 == 0 and (B // 2) * -(-min(Cin, Cout) // 64) >= (n_cu() * 3) // 4 and \
            bool(lib.onet_conv3x3_split_wgrad_pre_ok(B, Cin, Cout, H, W)) and int(lib.onet_maxpool2_bwd_bn_bands(H, W)) >= 0
    want = "bf16" if np_ == 1 else "split"
    return conv3x3_algo(B, Cin, Cout, H, W) == want and conv3x3_algo(B, Cout, Cin, H, W) == want and \
        bool(lib.onet_conv3x3_split_wgrad_pre_ok(B, Cin, Cout, H, W)) and int(lib.onet_conv3x3_split_nparts(B, H, W)) > 0 and \
        int(lib.onet_maxpool2_bwd_bn_bands(H, W)) > 0


def p16_empty(B, C, H, W, device, parts=None):
    """An uninitialised pre-split tensor in the slot layout [B, C/8, H, parts, W, 8]: fp16 (hi | mid) parts (4 bytes per element) or,
    under conv == "bf16", one part of plain bf16 (2 bytes per element)."""
    parts = p16_parts() if parts is None else parts
    return torch.empty((B, C // 8, H, parts, W, 8), dtype=torch.float16 if parts == 2 else BF, device=device)


def p16_of(t):
    """The valid pre-split form riding on tensor `t` (tag_p16), or None."""
    tag = getattr(t, "_onet_p16", None)
    if tag is None:
        return None
    return tag[0] if tag[1] == t._version else None


def p16_slots(t):
    """The magnitude slots the pre-split form of `t` was scaled by: None (unscaled), one set, or (skip set, up-sampled set, first
    channel of the second group) for a concat buffer with two producers."""
    tag = getattr(t, "_onet_p16", None)
    if tag is None or tag[1] != t._version:
        return None
    return tag[2]


def tag_p16(t, P, slots=None):
    if P is not None and t is not None:
        t._onet_p16 = (P, t._version, slots)
    return t


def _slots3(info):
    """-> (slots of the first group | None, slots of the second group | None, first channel of the second group or 0)"""
    if isinstance(info, tuple):
        return info
    return info, None, 0


def _pbs(P):
    """batch stride of a pre-split tensor (or of a channel-group slice of one) in 4-byte units"""
    return P.stride(0) // 2 if P.shape[0] > 1 else P.shape[1] * P.shape[2] * P.shape[3] * P.shape[4] * 4


def bn_relu_apply_split(z, save, xs, a=None, slots=None, group_images=0):
    """relu(bn(z)) written pre-split into xs [B, C/8, H, 2, W, 8] (a whole tensor or the leading channel groups of a concat buffer)
    and, when `a` is given, in fp32 too.  The same values, bit for bit, as bn_relu_apply (times the power of two the magnitude
    slots select -- 1 unless the activation's bound reaches 2^15).  group_images > 0: `save` is [G][4][C], one set of coefficients
    per group of that many consecutive images (the statistics groups of a twin batch in one launch)."""
    z, zbs = plane(z)
    B, C, H, W = z.shape
    assert group_images == 0 or (B % group_images == 0 and save.numel() == (B // group_images) * 4 * C and save.is_contiguous())
    _lib.call("onet_bn_relu_apply_split", _p(z), _z16(z), zbs, _p(xs), _pbs(xs), _p(a), 0 if a is None else (a.stride(0) if B > 1 else C * H * W),
              _p(save), _p(slots), xs.shape[3], group_images, B, C, H, W, _stream(),
              nbytes=(z.element_size() + 2 * xs.shape[3] + 4 * (a is not None)) * z.numel())


def bn_relu_apply_pool_split(z, save, xs, a, ys, y, slots=None, group_images=0):
    """relu(bn(z)) and its 2 x 2 max-pooling in one pass: the activation pre-split (xs) and / or fp32 (a), the pooled tensor pre-split
    (ys) or fp32 (y).  -> False where the kernel does not take the shape.  group_images: as bn_relu_apply_split."""
    z, zbs = plane(z)
    B, C, H, W = z.shape
    assert group_images == 0 or (B % group_images == 0 and save.numel() == (B // group_images) * 4 * C and save.is_contiguous())
    n, m = C * H * W, C * (H // 2) * (W // 2)
    rc = _lib.load().onet_bn_relu_apply_pool_split(_p(z), _z16(z), zbs, _p(xs), 0 if xs is None else _pbs(xs), _p(a),
                                                  0 if a is None else (a.stride(0) if B > 1 else n), _p(ys), 0 if ys is None else _pbs(ys),
                                                  _p(y), 0 if y is None else (y.stride(0) if B > 1 else m), _p(save), _p(slots),
                                                  (xs if xs is not None else ys).shape[3] if (xs is not None or ys is not None) else 2,
                                                  group_images, B, C, H, W, _stream())
    if rc < 0:
        raise _lib.OnetHipError(f"onet_bn_relu_apply_pool_split failed ({rc}): {_lib.last_error()}")
    return rc == 0


def conv3x3_pre_bn_partials(xP, pk, slots=None):
    """conv3x3_fwd_bn_partials for a pre-split input: -> (z, cm) with the BatchNorm statistics records of the epilogue.
    slots: what xP's producer(s) scaled it by (p16_slots)."""
    B, C8, H, np_, W, _ = xP.shape
    Co = pk["Cout"]
    wq = pk.get_pack("split" if np_ == 2 else "plain16")[0]
    nparts = int(_lib.load().onet_conv3x3_split_pre_nparts(B, H, W))
    cm = torch.empty((Co, nparts, 3), dtype=F32, device=xP.device) if nparts > 0 else None
    s1, s2, sc = _slots3(slots)
    # (z stored as bf16 only where the statistics come from the epilogue: a separate statistics pass would read the rounded values)
    return conv3x3_split_pre(xP, wq, Co, slots=s1, stats=cm, slots2=s2, split_ch=sc, z16=cm is not None and np_ == 1 and z16_storage()), cm


def _bn_bwd_groups(da, dabs, z, zbs, save_all, training, affine_out, rec4, da_amax, dz_slots):
    """Reduce + finalize of a BatchNorm + ReLU backward over ALL statistics groups of the tensor (consecutive batch slices; save_all
    [G][4][C]) in one launch each: -> (coef [G][4][C] | None, dgamma, dbeta).  rec4: the reduce records [G * np][C][4] a producer of
    da already wrote; da_amax: magnitude slots the reduce pass records max |da| in; dz_slots: slots that receive the bound of |dz|."""
    B, C, H, W = z.shape
    HW = H * W
    G = save_all.shape[0]
    Bg = B // G
    dev = z.device
    assert B % G == 0 and save_all.is_contiguous()
    if rec4 is None:
        nparts = _bn_nparts(Bg, HW)
        rec4 = torch.empty((G * nparts, C, 4), dtype=F32, device=dev)
        _lib.call("onet_bn_relu_bwd_reduce", _p(da), dabs, _p(z), _z16(z), zbs, _p(save_all), _p(rec4), G * nparts, _p(da_amax), Bg if G > 1 else 0,
                  B, C, HW, _stream(), nbytes=(4 + z.element_size()) * z.numel())
    else:
        assert rec4.shape[0] % G == 0 and rec4.shape[1] == C and rec4.shape[2] == 4 and rec4.is_contiguous()
    og, ob = affine_out if affine_out is not None else (None, None)
    dgamma = torch.empty(C, dtype=F32, device=dev) if og is None else og
    dbeta = torch.empty(C, dtype=F32, device=dev) if ob is None else ob
    coef = torch.empty((G, 4, C), dtype=F32, device=dev) if training else None
    _lib.call("onet_bn_bwd_finalize", _p(rec4), rec4.shape[0] // G, Bg * HW, _p(dgamma), _p(dbeta), _p(coef), 0, G, C, _p(save_all),
              _p(da_amax), _p(dz_slots), _stream())
    return coef, dgamma, dbeta


def bn_relu_bwd_split(da, z, save_all, training, need_affine_grads=True, affine_out=None, rec=None, rec4=None, da_amax=None, da_gl=None):
    """BatchNorm + ReLU backward of a layer whose dz is consumed by the pre-split kernels, all statistics groups of the tensor per
    launch: the reduce pass (also recording max |da|, unless the records -- and da's magnitude slots -- came fused from da's producer),
    then the finalize pass, which also writes the bound of |dz| into fresh magnitude slots, then dz written pre-split, scaled by the
    power of two those slots select.  Plain bf16 operands (conv == "bf16", one part): no magnitudes, no scale.
    da_gl = (g, L) (the network's last unit behind the fused head backward, head_bwd_reduce, which also wrote rec4 and da_amax): da is
    g[b, 0, y, x] * L[b, c, y, x] and exists nowhere -- `da` is its placeholder -- the apply pass forms it on load.
    -> (dzP, dz_slots | None, dgamma, dbeta)."""
    if da_gl is not None:
        if rec4 is None or _z16(z) or (p16_parts() == 2 and da_amax is None):
            raise RuntimeError("onet_amd: a BatchNorm backward on an unmaterialised g * L needs the records of the fused head backward")
        gmap = da_gl[0]
        da, dabs = plane(da_gl[1])
        assert gmap.is_contiguous() and gmap.shape[0] == z.shape[0] and gmap.numel() == z.shape[0] * z.shape[2] * z.shape[3] and da.shape == z.shape
    else:
        da, dabs = plane(da)
    z, zbs = plane(z)
    B, C, H, W = z.shape
    G = save_all.shape[0]
    dev = z.device
    np_ = p16_parts()
    dzP = p16_empty(B, C, H, W, dev, np_)
    scaled = np_ == 2
    dz_slots = new_amax(dev) if scaled else None
    if scaled and rec4 is not None and da_amax is None:
        da_amax = absmax_slots(da)                  # records fused by a producer that did not record the magnitude: one extra pass
    if rec4 is None:
        da_amax = new_amax(dev) if scaled else None
    coef, dgamma, dbeta = _bn_bwd_groups(da, dabs, z, zbs, save_all, training, affine_out, rec4, da_amax, dz_slots)
    if da_gl is not None:
        _lib.call("onet_bn_relu_bwd_apply_split_gl", _p(da), dabs, _p(gmap), _p(z), zbs, _p(save_all), _p(coef), _p(dzP), _pbs(dzP), _p(dz_slots), np_,
                  B // G if G > 1 else 0, B, C, H, W, _stream(), nbytes=(8 + 2 * np_) * z.numel() + 4 * gmap.numel())
        return dzP, dz_slots, dgamma, dbeta
    _lib.call("onet_bn_relu_bwd_apply_split", _p(da), dabs, _p(z), _z16(z), zbs, _p(save_all), _p(coef), _p(dzP), _pbs(dzP), _p(dz_slots), np_,
              B // G if G > 1 else 0, B, C, H, W, _stream(), nbytes=(4 + z.element_size() + 2 * np_) * z.numel())
    return dzP, dz_slots, dgamma, dbeta


def stem_wgrad_bn(x, da, z, save_all, training, dw_shape, affine_out=None, rec4=None, out=None, twin=None):
    """BatchNorm + ReLU backward and weight gradient of the stem unit (Cin <= 4; its input has no gradient, so dz has no other reader):
    reduce + finalize as bn_relu_bwd_groups, then ONE pass over (da, z) that forms dz per element and accumulates dW -- the apply pass
    and its dz tensor are gone.  Same bits as bn_relu_bwd_groups + conv_wgrad.  -> (dw, dgamma, dbeta)."""
    require_gpu(x, da, z)
    if twin is None:
        twin = twin_src_of(x)            # (X, bias) of a virtual twin batch: x is then only its placeholder
    B, Cin, H, W = x.shape
    x, xbs = plane(twin[0] if twin is not None else x)
    da, dabs = plane(da)
    z, zbs = plane(z)
    Cout = z.shape[1]
    G = save_all.shape[0]
    coef, dgamma, dbeta = _bn_bwd_groups(da, dabs, z, zbs, save_all, training, affine_out, rec4, None, None)
    dw = torch.empty(dw_shape, dtype=F32, device=x.device) if out is None else out
    ws = workspace(_lib.load().onet_conv_wgrad_ws_bytes(B, Cin, Cout, H, W, 3), x.device)
    e0 = _prof_begin("conv_wgrad_kernel")
    _lib.call("onet_conv3x3_stem_wgrad_bn", _p(x), xbs, _p(da), dabs, _p(z), zbs, _p(save_all), _p(coef), B // G if G > 1 else 0, _p(dw),
              _p(ws), ws.numel() * 4, B, Cin, Cout, H, W, 0, B // 2 if twin is not None else 0, twin[1] if twin is not None else 0.0, _stream())
    _prof_end("conv_wgrad_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0, 4.0 * (B * H * W * (Cin + 2 * Cout) + 9 * Cin * Cout))
    return dw, dgamma, dbeta


STEM_WGRAD_BN = _flag("STEM_WGRAD_BN", True)     # 0 (diagnostic): the stem's dz is materialised by the apply pass


def bn_relu_bwd_groups(da, z, save_all, training, affine_out=None, rec4=None):
    """The same for a layer whose dz stays fp32 (the stem under pre-split storage): -> (dz, dgamma, dbeta)."""
    da, dabs = plane(da)
    z, zbs = plane(z)
    B, C, H, W = z.shape
    G = save_all.shape[0]
    coef, dgamma, dbeta = _bn_bwd_groups(da, dabs, z, zbs, save_all, training, affine_out, rec4, None, None)
    dz = torch.empty((B, C, H, W), dtype=F32, device=z.device)
    _lib.call("onet_bn_relu_bwd_apply", _p(da), dabs, _p(z), zbs, _p(save_all), _p(coef), _p(dz), C * H * W, None, B // G if G > 1 else 0,
              B, C, H * W, _stream(), nbytes=12 * z.numel())
    return dz, dgamma, dbeta


def split_wgrad_ok(x, dz):
    B, Cin, H, W = x.shape
    ok = bool(_lib.load().onet_conv3x3_split_wgrad_ok(B, Cin, dz.shape[1], H, W)) and \
        x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and dz.is_contiguous() and dz.data_ptr() % 16 == 0 and \
        max(Cin, dz.shape[1]) * H * W * 4 < 2 ** 31
    if ok and W < 64:        # 64 / W images side by side per unit: one buffer resource over the whole batch
        ok = ((B - 1) * x.stride(0) + Cin * H * W) * 4 < 2 ** 31 and B * dz.shape[1] * H * W * 4 < 2 ** 31
    return ok


def norm_on_load_ok(B, Cmid, Cout, H, W, groups):
    """May the second convolution of a DoubleConv (Cmid -> Cout on B maps of H x W, `groups` BatchNorm statistics groups) take
    the first unit's BatchNorm + ReLU into its own operand staging -- forward AND weight gradient -- so that the first unit's
    activation is never written?  Both must be the split-bf16 kernels (fp32 model, default dispatch)."""
    if not _setting("bn_on_load", BN_ON_LOAD) or sync_bn() or conv_algo() not in ("auto", "split") or groups not in (1, 2) or B % groups:
        return False
    if conv3x3_algo(B, Cmid, Cout, H, W) != "split" or W < SPLIT_WGRAD_MINW:
        return False
    if Cout > BN_ON_LOAD_MAX_COUT:
        return False
    if not _lib.load().onet_conv3x3_split_wgrad_ok(B, Cmid, Cout, H, W) or max(Cmid, Cout) * H * W * 4 >= 2 ** 31:
        return False
    return W >= 64 or B * max(Cmid, Cout) * H * W * 4 < 2 ** 31


def conv3x3_split_wgrad(x, dz, dw_shape, out=None, norm=None, dz_amax=None, x_amax=None):
    """dW of a 3x3 convolution in fp32 accuracy on the 16-bit matrix cores (conv_split.hip: both operands split, three MFMAs per term).
    norm = save [G, 4, Cin]: x is the pre-activation of the unit below, normalised (BatchNorm + ReLU) on load.
    dz_amax (magnitude slots of dz, from onet_bn_relu_bwd_apply): fp16 parts of the scaled operands (22-bit operands; x_amax:
    the overflow guard for x); None: bf16 parts (16-bit operands), the round-3 arithmetic."""
    if dz_amax is not None:
        require_gpu(x, dz)
        x, xbs = plane(x)
        dz, dzbs = plane(dz)
        B, Cin, H, W = x.shape
        Cout = dz.shape[1]
        dw = torch.empty(dw_shape, dtype=F32, device=x.device) if out is None else out
        ws = workspace(_lib.load().onet_conv3x3_split_wgrad_ws_bytes(B, Cin, Cout, H, W), x.device)
        e0 = _prof_begin("conv3x3_split_wgrad_kernel")
        _lib.call("onet_conv3x3_split_wgrad_f16", _p(x), xbs, _p(x_amax), _p(norm), 0 if norm is None else norm.shape[0], _p(dz), dzbs,
                  _p(dz_amax), _p(dw), _p(ws), ws.numel() * 4, B, Cin, Cout, H, W, 0, _stream())
        _prof_end("conv3x3_split_wgrad_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0, 4.0 * (B * H * W * (Cin + Cout) + 9 * Cin * Cout))
        return dw
    if norm is not None:
        require_gpu(x, dz, norm)
        x, xbs = plane(x)
        dz, dzbs = plane(dz)
        B, Cin, H, W = x.shape
        Cout = dz.shape[1]
        dw = torch.empty(dw_shape, dtype=F32, device=x.device) if out is None else out
        ws = workspace(_lib.load().onet_conv3x3_split_wgrad_ws_bytes(B, Cin, Cout, H, W), x.device)
        e0 = _prof_begin("conv3x3_split_wgrad_kernel")
        _lib.call("onet_conv3x3_split_wgrad_norm", _p(x), xbs, _p(norm), norm.shape[0], _p(dz), dzbs, _p(dw), _p(ws), ws.numel() * 4,
                  B, Cin, Cout, H, W, 0, _stream())
        _prof_end("conv3x3_split_wgrad_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0, 4.0 * (B * H * W * (Cin + Cout) + 9 * Cin * Cout))
        return dw
    require_gpu(x, dz)
    x, xbs = plane(x)
    dz, dzbs = plane(dz)
    B, Cin, H, W = x.shape
    Cout = dz.shape[1]
    dw = torch.empty(dw_shape, dtype=F32, device=x.device) if out is None else out
    need = _lib.load().onet_conv3x3_split_wgrad_ws_bytes(B, Cin, Cout, H, W)
    ws = workspace(need, x.device)
    e0 = _prof_begin("conv3x3_split_wgrad_kernel")
    _lib.call("onet_conv3x3_split_wgrad", _p(x), xbs, _p(dz), dzbs, _p(dw), _p(ws), ws.numel() * 4, B, Cin, Cout, H, W, 0, _stream())
    _prof_end("conv3x3_split_wgrad_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0, 4.0 * (B * H * W * (Cin + Cout) + 9 * Cin * Cout))
    return dw


def _engine_accumulates(param):
    """Will the running backward accumulate into param.grad?  Not under torch.autograd.grad (the gradient is returned to the caller,
    who must not get a view of the flat buffer that the next zero_grad clears) nor under backward(inputs=...) without param."""
    # (its AccumulateGrad node, looked up per call -- a few microseconds, once per parameter and zero_grad: kept on the parameter it
    # would form a reference cycle through the node's own reference to the parameter)
    try:
        return bool(torch._C._will_engine_execute_node(torch.autograd.graph.get_gradient_edge(param).node))
    except RuntimeError:            # "... a leaf node was passed ... while running autograd.grad()"
        return False


def grad_slot_if_free(param):
    """FlatAdam registers, per parameter, its slice of the flat gradient buffer.  When the parameter has no .grad yet
    (FlatAdam.zero_grad sets it to None) a backward kernel may write its result straight into that slice and hand the
    view to autograd, which then adopts it as .grad without an accumulation kernel (62 + 72 tiny adds per step
    otherwise).  -> a fresh contiguous view, or None (no slot, or a gradient is already there: regular path)."""
    slot = getattr(param, "_onet_gslot", None)
    if slot is None or param.grad is not None or getattr(param, "_onet_gslot_taken", False) or not _engine_accumulates(param):
        return None
    # one taker per zero_grad: with shared weights used twice in a graph (two-pass mode) autograd sums the two
    # contributions in its input buffer BEFORE .grad is set, so ".grad is None" alone would hand the slice out twice
    param._onet_gslot_taken = True
    flat, off, n, shape = slot
    return flat[off:off + n].view(shape)




def conv3x3_winograd4_wgrad(x, dz, dw_shape, out=None):
    """dW of a 3x3 convolution by Winograd F(3x3,4x4) (conv_wino4w.hip); see `winograd4_wgrad_ok` for its shapes."""
    require_gpu(x, dz)
    x, xbs = plane(x)
    dz, dzbs = plane(dz)
    B, Cin, H, W = x.shape
    Cout = dz.shape[1]
    dw = torch.empty(dw_shape, dtype=F32, device=x.device) if out is None else out
    need = _lib.load().onet_conv3x3_winograd4_wgrad_ws_bytes(B, Cin, Cout, H, W)
    ws = workspace(need, x.device)
    e0 = _prof_begin("conv_wino4_wgrad_kernel")
    _lib.call("onet_conv3x3_winograd4_wgrad", _p(x), xbs, _p(dz), dzbs, _p(dw), _p(ws), ws.numel() * 4, B, Cin, Cout, H, W,
              0, _stream())
    _prof_end("conv_wino4_wgrad_kernel", 2.0 * B * H * W * Cin * Cout * 9, e0, 4.0 * (B * H * W * (Cin + Cout) + 9 * Cin * Cout))
    return dw


def winograd4_wgrad_ok(x, dz):
    B, Cin, H, W = x.shape
    return bool(_lib.load().onet_conv3x3_winograd4_wgrad_ok(B, Cin, dz.shape[1], H, W)) and \
        x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and dz.is_contiguous()


def conv3x3_wgrad_auto(x, dz, dw_shape, out=None, dz_amax=None, x_amax=None):
    Cout, Cin = dw_shape[0], dw_shape[1]
    # fp32 tensors, maps 16 / 32 / >= 64 pixels wide: the split-bf16 row kernel (the stem, Cin < 16, keeps its own VALU kernel)
    if conv_algo() in ("auto", "split", "bf16") and (split_enabled() or conv_algo() == "split") and Cin >= 16 and \
            x.shape[3] >= SPLIT_WGRAD_MINW and split_wgrad_ok(x, dz):
        return conv3x3_split_wgrad(x, dz, dw_shape, out=out, dz_amax=dz_amax if grad_f16() else None, x_amax=x_amax)
    if use_winograd(Cin, Cout, x.shape[2], x.shape[3]) and winograd4_wgrad_ok(x, dz):
        return conv3x3_winograd4_wgrad(x, dz, dw_shape, out=out)
    return conv_wgrad(x, dz, dw_shape, 3, out=out)


def conv_fwd(x, wp, Cout, ks, out=None):
    """z = conv_ks(x) with packed weights wp ([Cin][ks*ks][Cout]); also used for dgrad."""
    require_gpu(x, wp)
    x, xbs = plane(x)
    B, Cin, H, W = x.shape
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=F32, device=x.device)
    zbs = out.stride(0) if B > 1 else Cout * H * W
    e0 = _prof_begin("conv_fwd_kernel")
    _lib.call("onet_conv_fwd", _p(x), xbs, _p(wp), _p(out), zbs, None, B, Cin, Cout, H, W, ks, _stream())
    _prof_end("conv_fwd_kernel", 2.0 * B * H * W * Cin * Cout * ks * ks, e0,
              4.0 * (B * H * W * (Cin + Cout) + ks * ks * Cin * Cout))
    return out


def conv_wgrad(x, dz, dw_shape, ks, out_layout=0, out=None):
    require_gpu(x, dz)
    x, xbs = plane(x)
    dz, dzbs = plane(dz)
    B, Cin, H, W = x.shape
    Cout = dz.shape[1]
    dw = torch.empty(dw_shape, dtype=F32, device=x.device) if out is None else out
    need = _lib.load().onet_conv_wgrad_ws_bytes(B, Cin, Cout, H, W, ks)
    ws = workspace(need, x.device)
    e0 = _prof_begin("conv_wgrad_kernel")
    _lib.call("onet_conv_wgrad", _p(x), xbs, _p(dz), dzbs, _p(dw), _p(ws), ws.numel() * 4, B, Cin, Cout, H, W, ks,
              out_layout, 0, _stream())
    _prof_end("conv_wgrad_kernel", 2.0 * B * H * W * Cin * Cout * ks * ks, e0,
              4.0 * (B * H * W * (Cin + Cout) + ks * ks * Cin * Cout))
    return dw


# ----------------------------------------------------------------------------- batch norm + relu
# SyncBN (opt-in): the per-rank Welford partials (forward) and (sum dy, sum dy*xhat)
# partials (backward) are all-gathered over the data-parallel group before the finalize kernels, so
# every rank normalises with the statistics of the GLOBAL batch and running stats stay identical.
SYNC_BN = False


def set_sync_bn(flag: bool):
    global SYNC_BN
    SYNC_BN = bool(flag)


def _gather_partials(part):
    """[nparts, C, k] -> [world*nparts, C, k] over the default process group (RCCL)."""
    import torch.distributed as dist
    if not (sync_bn() and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return part, 1
    world = dist.get_world_size()
    out = torch.empty((world * part.shape[0],) + tuple(part.shape[1:]), dtype=part.dtype, device=part.device)
    if dist.get_backend() == "nccl":
        dist.all_gather_into_tensor(out, part.contiguous())
    else:       # gloo (CPU tests, the two-ranks-on-one-GPU rehearsal) has no flat all-gather: per-rank views of `out`
        dist.all_gather(list(out.chunk(world, dim=0)), part.contiguous())
    return out, world


def _bn_nparts(B, HW):
    return B * max(1, (HW + 16383) // 16384)


def bn_train_coeffs(z, gamma, beta, running_mean, running_var, momentum, eps, cm=None, save=None, act_slots=None, groups=1):
    """batch statistics -> save [4][C] = (mean, invstd, scale, shift); updates running stats in place.
    `cm` = (records [C, NP, 3], first, count): the convolution already produced this batch's statistics records
    (`conv3x3_fwd_bn_partials`), records first .. first+count-1 of every channel belong to `z`.
    groups > 1 (with `cm`): z is ONE statistics group of a twin batch and the records of the others follow (count each): all groups in
    one launch, save [groups][4][C], the running statistics updated group after group."""
    z, zbs = plane(z)
    B, C, H, W = z.shape
    if B * H * W <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {list(z.shape)}")
    if cm is not None:
        rec, first, count = cm
        assert rec.shape[0] == C and rec.shape[2] == 3 and 0 <= first and first + count <= rec.shape[1]
        if save is None:
            save = torch.empty((4, C), dtype=F32, device=z.device)
        assert groups == 1 or (first + groups * count <= rec.shape[1] and save.shape[0] == groups and save.is_contiguous())
        # (act_slots: also the bound of relu(bn(z)) into the activation's magnitude slots -- pre-split storage)
        _lib.call("onet_bn_finalize_cm", rec.data_ptr() + first * 12, count, rec.shape[1] * 3, _p(gamma), _p(beta),
                  _p(running_mean), _p(running_var), float(momentum), float(eps), _p(save), _p(act_slots), groups, C, _stream())
        return save
    assert groups == 1
    nparts = _bn_nparts(B, H * W)
    part = torch.empty((nparts, C, 3), dtype=F32, device=z.device)
    _lib.call("onet_bn_stats_partial", _p(z), zbs, _p(part), nparts, B, C, H * W, _stream(), nbytes=4 * z.numel())
    part, world = _gather_partials(part)
    nparts *= world
    if save is None:
        save = torch.empty((4, C), dtype=F32, device=z.device)
    _lib.call("onet_bn_finalize", _p(part), nparts, B * H * W * world, _p(gamma), _p(beta), _p(running_mean),
              _p(running_var), float(momentum), float(eps), _p(save), _p(act_slots), C, _stream())
    return save


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps, save=None):
    C = running_mean.numel()
    if save is None:
        save = torch.empty((4, C), dtype=F32, device=running_mean.device)
    _lib.call("onet_bn_eval_coeffs", _p(gamma), _p(beta), _p(running_mean), _p(running_var), float(eps), _p(save),
              C, _stream())
    return save


def amax_of(t):
    """The valid magnitude slots riding on activation `t` (tag_amax), or None."""
    tag = getattr(t, "_onet_amax", None)
    if tag is None:
        return None
    slots, ver = tag
    return slots if ver == t._version else None


def tag_amax(t, slots):
    if slots is not None and t is not None:
        t._onet_amax = (slots, t._version)
    return t


def bn_relu_apply(z, save, out=None, amax=None, group_images=0):
    """a = relu(bn(z)) in fp32.  amax: magnitude slots that receive max a.  group_images > 0: save is [G][4][C], one set per group of
    that many consecutive images.  (z may be stored as bf16: ops.z16_storage.)"""
    z, zbs = plane(z)
    B, C, H, W = z.shape
    assert group_images == 0 or (B % group_images == 0 and save.numel() == (B // group_images) * 4 * C and save.is_contiguous())
    if out is None:
        out = torch.empty((B, C, H, W), dtype=F32, device=z.device)
    abs_ = out.stride(0) if B > 1 else C * H * W
    _lib.call("onet_bn_relu_apply", _p(z), _z16(z), zbs, _p(out), abs_, _p(save), _p(amax), group_images,
              B, C, H * W, _stream(), nbytes=(4 + z.element_size()) * z.numel())
    return out


FUSE_POOL = _flag("FUSE_POOL", True)       # 0: separate max-pool pass after BatchNorm + ReLU


def bn_relu_apply_pool(z, save, out, y, amax=None):
    """a = relu(bn(z)) and y = maxpool2(a) in one pass (an encoder block's output that is pooled next); out, y: plane-contiguous fp32
    destinations.  -> False (nothing done) where the fused kernel does not take the shape.  amax: magnitude slots that receive
    max a = max y."""
    z, zbs = plane(z)
    B, C, H, W = z.shape
    if H % 2 or W % 4:
        return False

    def bs(t, n):
        return 0 if t is None else (t.stride(0) if B > 1 else n)
    n, m = C * H * W, C * (H // 2) * (W // 2)
    rc = _lib.load().onet_bn_relu_apply_pool(_p(z), zbs, _p(out), bs(out, n), _p(y), bs(y, m), _p(save), _p(amax), B, C, H, W, _stream())
    if rc < 0:
        raise _lib.OnetHipError(f"onet_bn_relu_apply_pool failed ({rc}): {_lib.last_error()}")
    return rc == 0


def bn_bwd_coefs(da, z, save, training, need_affine_grads=True, acc=None, affine_out=None, red=None, red4=None, da_amax=None):
    """The reduce + finalize passes of bn_relu_bwd for one statistics group: -> (coef [4, C] | None, dgamma, dbeta).  da_amax: magnitude
    slots in which the (standalone) reduce pass records max |da|."""
    da, dabs = plane(da)
    z, zbs = plane(z)
    B, C, H, W = z.shape
    HW = H * W
    nparts = _bn_nparts(B, HW)
    dev = z.device
    dgamma = dbeta = coef = None
    if red is not None and (training or need_affine_grads):
        rec, first, count = red
        assert rec.shape[0] == C and rec.shape[2] == 2 and 0 <= first and first + count <= rec.shape[1]
        if acc is None:
            og, ob = affine_out if affine_out is not None else (None, None)
            dgamma = torch.empty(C, dtype=F32, device=dev) if og is None else og
            dbeta = torch.empty(C, dtype=F32, device=dev) if ob is None else ob
        else:
            dgamma, dbeta = acc
        coef = torch.empty((4, C), dtype=F32, device=dev) if training else None
        _lib.call("onet_bn_bwd_finalize_cm", rec.data_ptr() + first * 8, count, rec.shape[1] * 2, B * HW, _p(dgamma),
                  _p(dbeta), _p(coef), 0 if acc is None else 1, C, _stream())
    elif training or need_affine_grads:
        if red4 is not None:
            rec4, first, count = red4
            assert rec4.shape[1] == C and rec4.shape[2] == 4 and 0 <= first and first + count <= rec4.shape[0]
            part2, nparts = rec4[first:first + count], count
        else:
            part2 = torch.empty((nparts, C, 4), dtype=F32, device=dev)
            _lib.call("onet_bn_relu_bwd_reduce", _p(da), dabs, _p(z), _z16(z), zbs, _p(save), _p(part2), nparts, _p(da_amax), 0, B, C, HW,
                      _stream(), nbytes=(4 + z.element_size()) * z.numel())
        if acc is None:
            og, ob = affine_out if affine_out is not None else (None, None)
            dgamma = torch.empty(C, dtype=F32, device=dev) if og is None else og
            dbeta = torch.empty(C, dtype=F32, device=dev) if ob is None else ob
        else:
            dgamma, dbeta = acc
        accf = 0 if acc is None else 1
        coef = torch.empty((4, C), dtype=F32, device=dev) if training else None
        gathered, world = _gather_partials(part2) if training else (part2, 1)
        if world == 1:
            _lib.call("onet_bn_bwd_finalize", _p(part2), nparts, B * HW, _p(dgamma), _p(dbeta), _p(coef), accf, 1, C, None, None, None, _stream())
        else:
            # SyncBN: dgamma/dbeta are the LOCAL sums (the gradient all-reduce adds the ranks, as in
            # torch.nn.SyncBatchNorm); c1/c2 in `coef` are means over the GLOBAL batch.
            _lib.call("onet_bn_bwd_finalize", _p(part2), nparts, B * HW, _p(dgamma), _p(dbeta), None, accf, 1, C, None, None, None, _stream())
            _lib.call("onet_bn_bwd_finalize", _p(gathered), nparts * world, B * HW * world, None, None, _p(coef), 0, 1, C, None, None, None,
                      _stream())
    return coef, dgamma, dbeta


def bn_relu_bwd(da, z, save, training, need_affine_grads=True, out=None, acc=None, affine_out=None, red=None, red4=None, amax=None):
    """-> dz, dgamma, dbeta.  `out`: plane-contiguous destination for dz (a batch slice of a larger buffer);
    `acc` = (dgamma, dbeta) of another statistics group of the same layer to accumulate into; `affine_out` =
    (dgamma, dbeta) destinations to overwrite (None entries are allocated); `red` = (records [C, NP, 2], first, count):
    the (sum dy, sum dy*xhat) records of this batch slice were already written by the dgrad launch that produced
    `da` (`conv3x3_dgrad_bnreduce`), so the reduce pass over (da, z) is skipped; `red4` = (records [NP, C, 4], first,
    count): the same in the reduce kernel's own record format (written by the pooling-backward kernel).
    `amax`: 64 zeroed magnitude slots (new_amax) in which the apply pass
    records max |dz| for the fp16-split gradient kernels (several statistics groups of one tensor share them)."""
    coef, dgamma, dbeta = bn_bwd_coefs(da, z, save, training, need_affine_grads, acc, affine_out, red, red4)
    da, dabs = plane(da)
    z, zbs = plane(z)
    B, C, H, W = z.shape
    HW = H * W
    dev = z.device
    dz = torch.empty((B, C, H, W), dtype=F32, device=dev) if out is None else out
    dzbs = dz.stride(0) if B > 1 else C * HW
    _lib.call("onet_bn_relu_bwd_apply", _p(da), dabs, _p(z), zbs, _p(save), _p(coef), _p(dz), dzbs, _p(amax), 0, B, C, HW,
              _stream(), nbytes=12 * z.numel())
    return dz, dgamma, dbeta


# ----------------------------------------------------------------------------- pool / up / cat
def maxpool2_fwd(x):
    """y = MaxPool2d(2)(x)"""
    x, xbs = plane(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, H // 2, W // 2), dtype=F32, device=x.device)
    _lib.call("onet_maxpool2_fwd", _p(x), xbs, _p(y), C * (H // 2) * (W // 2), B, C, H, W, _stream(), nbytes=5 * x.numel())
    return y


def maxpool2_bwd(x, dy, add=None, add2=None, bn=None, dx_amax=None):
    """dx of MaxPool2d(2); `add`, `add2`: other gradients of x (plane-contiguous, e.g. a slice of a concat gradient)
    summed in the same pass.  `bn` = (z, save_all [G, 4, C]): x is the output relu(bn(z)) of a Conv-BN-ReLU unit with G
    statistics groups -- the unit's BatchNorm-backward reduce records are taken on the way: -> (dx, part2 [B * bands, C, 4])
    (or (dx, None) where the fused form is not available).  Pre-split storage: x may be a placeholder (the activation exists only
    pre-split; with `bn` the kernel recomputes it from z) and dx_amax = magnitude slots that receive max |dx|."""
    if is_placeholder(x):
        if bn is None:
            raise RuntimeError("onet_amd: max-pooling backward of an activation kept only pre-split needs its (z, coefficients)")
        B, C, H, W = x.shape
        x, xbs = None, C * H * W
    else:
        x, xbs = plane(x)
        B, C, H, W = x.shape
    dy, dybs = plane(dy)
    dx = torch.empty((B, C, H, W), dtype=F32, device=dy.device)
    if add is None and add2 is not None:
        add, add2 = add2, None
    a1, a1bs = plane(add) if add is not None else (None, 0)
    a2, a2bs = plane(add2) if add2 is not None else (None, 0)
    if bn is not None:
        z, save_all = bn
        bands = int(_lib.load().onet_maxpool2_bwd_bn_bands(H, W)) if (FUSE_BN_REDUCE and not sync_bn()) else 0
        z, zbs = plane(z)
        G = save_all.shape[0]
        aligned = all(t is None or (t.data_ptr() & 15) == 0 for t in (x, a1, a2)) and (z.data_ptr() & (7 if _z16(z) else 15)) == 0 and \
            (dy.data_ptr() & 7) == 0 and all((v & 3) == 0 for v in (xbs, zbs, a1bs, a2bs)) and (dybs & 1) == 0
        if bands > 0 and aligned and B % G == 0 and tuple(z.shape) == (B, C, H, W) and save_all.is_contiguous():
            part2 = torch.empty((B * bands, C, 4), dtype=F32, device=dy.device)
            _lib.call("onet_maxpool2_bwd_add_bnreduce", _p(x), xbs, _p(dy), dybs, _p(a1), a1bs, _p(a2), a2bs, _p(dx),
                      C * H * W, _p(z), _z16(z), zbs, _p(save_all), B // G, _p(part2), _p(dx_amax), B, C, H, W, _stream(),
                      nbytes=(5 + z.element_size() + 4 * (x is not None) + 4 * (a1 is not None) + 4 * (a2 is not None)) * dx.numel())
            return dx, part2
        if x is None:
            raise RuntimeError("onet_amd: max-pooling backward of an activation kept only pre-split: the fused kernel does not take this shape")
    _lib.call("onet_maxpool2_bwd", _p(x), xbs, _p(dy), dybs, _p(a1), a1bs, _p(a2), a2bs, _p(dx), C * H * W,
              B, C, H, W, 0, _stream(), nbytes=(9 + 4 * (a1 is not None) + 4 * (a2 is not None)) * x.numel())
    return dx if bn is None else (dx, None)


def copy_strided(src, dst):
    """dst[b] = src[b] for plane-contiguous [B,C,H,W] views."""
    src, sbs = plane(src)
    B, C, H, W = src.shape
    dbs = dst.stride(0) if B > 1 else C * H * W
    _lib.call("onet_copy_strided", _p(src), sbs, _p(dst), dbs, B, C * H * W, _stream())
    return dst


def pixel_shuffle2_bias(sub, bias, out, pt, pl):
    """sub [B,4C,h,w] -> out [B,C,Ho,Wo] (a plane-contiguous view, e.g. the 2nd half of a cat buffer)."""
    B, C4, h, w = sub.shape
    C = C4 // 4
    Ho, Wo = out.shape[2], out.shape[3]
    obs = out.stride(0) if B > 1 else C * Ho * Wo
    _lib.call("onet_pixel_shuffle2_bias", _p(sub), _p(bias), _p(out), obs, B, C, h, w, Ho, Wo, pt, pl, _stream())
    return out


def space_to_depth2(dy, h, w, pt, pl, want_dbias):
    dy, dybs = plane(dy)
    B, C, Ho, Wo = dy.shape
    sub = torch.empty((B, 4 * C, h, w), dtype=F32, device=dy.device)
    dbias = torch.empty(C, dtype=F32, device=dy.device) if want_dbias else None
    scratch = torch.empty(B * C, dtype=torch.float64, device=dy.device) if want_dbias else None
    _lib.call("onet_space_to_depth2", _p(dy), dybs, _p(sub), _p(dbias), _p(scratch), 0, B, C, h, w, Ho, Wo, pt, pl,
              _stream())
    return sub, dbias


def convT2x2_bwd_fusable(Ct):
    """The gather-fused ConvTranspose2d backward needs a block's 64 GEMM rows inside one sub-pixel plane."""
    return Ct % 64 == 0


def convT2x2_dgrad(dy, wp_dgrad, Cin, h, w, pt, pl, want_dbias=False, db_out=None):
    """dx1 of ConvTranspose2d(k=2, s=2) straight from the [B, Ct, Ho, Wo] window `dy` of the concat gradient.
    want_dbias: -> (dx1, dbias | None): where the 128 x 128 GEMM path takes the shape the bias gradient is summed from the
    dy rows that launch stages anyway; None = not taken (the caller then runs the separate dbias pass)."""
    require_gpu(dy, wp_dgrad)
    dy, dybs = plane(dy)
    B, Ct, Ho, Wo = dy.shape
    dx = torch.empty((B, Cin, h, w), dtype=F32, device=dy.device)
    flops, nbytes = 2.0 * B * h * w * Cin * 4 * Ct, 4.0 * (B * h * w * (Cin + 4 * Ct) + 4 * Cin * Ct)
    if want_dbias:
        lib = _lib.load()
        need = int(lib.onet_convT2x2_dgrad_dbias_ws_bytes(B, Ct, h, w))
        if need > 0:
            db = torch.empty(Ct, dtype=F32, device=dy.device) if db_out is None else db_out
            ws = torch.empty(need // 4, dtype=F32, device=dy.device)
            e0 = _prof_begin("convt_gemm_kernel")
            rc = lib.onet_convT2x2_dgrad_dbias(_p(dy), dybs, _p(wp_dgrad), _p(dx), Cin * h * w, _p(db), _p(ws), need, B, Cin, Ct, h,
                                               w, Ho, Wo, pt, pl, convt_operand_bf16(B, h, w, Ct), _stream())
            if rc == 0:
                _prof_end("convt_gemm_kernel", flops, e0, nbytes)
                return dx, db
            _prof_end("convt_gemm_kernel", 0.0, e0, 0.0)
            if rc < 0:
                raise _lib.OnetHipError(f"onet_convT2x2_dgrad_dbias failed ({rc}): {_lib.last_error()}")
    e0 = _prof_begin("convt_gemm_kernel")
    _lib.call("onet_convT2x2_dgrad", _p(dy), dybs, _p(wp_dgrad), _p(dx), Cin * h * w, B, Cin, Ct, h, w, Ho, Wo, pt, pl,
              convt_operand_bf16(B, h, w, Ct), _stream())
    _prof_end("convt_gemm_kernel", flops, e0, nbytes)
    return (dx, None) if want_dbias else dx


def convT2x2_wgrad(x, dy, dw_shape, pt, pl, want_dbias, out=None, db_out=None):
    """(dW [Cin, Ct, 2, 2], dbias | None) of ConvTranspose2d(k=2, s=2) from x1 and the concat-gradient window."""
    require_gpu(x, dy)
    x, xbs = plane(x)
    dy, dybs = plane(dy)
    B, Cin, h, w = x.shape
    Ct, Ho, Wo = dy.shape[1], dy.shape[2], dy.shape[3]
    dw = torch.empty(dw_shape, dtype=F32, device=x.device) if out is None else out
    need = _lib.load().onet_convT2x2_wgrad_ws_bytes(B, Cin, Ct, h, w)
    ws = workspace(need, x.device)
    e0 = _prof_begin("convt_wgrad_gemm_kernel")
    _lib.call("onet_convT2x2_wgrad", _p(x), xbs, _p(dy), dybs, _p(dw), _p(ws), ws.numel() * 4, B, Cin, Ct, h, w, Ho, Wo,
              pt, pl, convt_operand_bf16(B, h, w, Ct), _stream())
    _prof_end("convt_wgrad_gemm_kernel", 2.0 * B * h * w * Cin * 4 * Ct, e0, 4.0 * (B * h * w * (Cin + 4 * Ct) + 4 * Cin * Ct))
    db = None
    if want_dbias:
        db = torch.empty(Ct, dtype=F32, device=x.device) if db_out is None else db_out
        scratch = torch.empty(B * Ct, dtype=torch.float64, device=x.device)
        _lib.call("onet_convT2x2_dbias", _p(dy), dybs, _p(db), _p(scratch), 0, B, Ct, h, w, Ho, Wo, pt, pl, _stream())
    return dw, db


def bilinear2x_fwd(x, out, pt, pl):
    x, xbs = plane(x)
    B, C, h, w = x.shape
    Ho, Wo = out.shape[2], out.shape[3]
    obs = out.stride(0) if B > 1 else C * Ho * Wo
    _lib.call("onet_bilinear2x_fwd", _p(x), xbs, _p(out), obs, B, C, h, w, Ho, Wo, pt, pl, _stream())
    return out


def bilinear2x_bwd(dy, h, w, pt, pl):
    dy, dybs = plane(dy)
    B, C, Ho, Wo = dy.shape
    dx = torch.empty((B, C, h, w), dtype=F32, device=dy.device)      # (gather kernel: every element written, no atomics)
    _lib.call("onet_bilinear2x_bwd", _p(dy), dybs, _p(dx), C * h * w, B, C, h, w, Ho, Wo, pt, pl, _stream())
    return dx


# ----------------------------------------------------------------------------- elementwise
def complement_clip(x, bias, out=None):
    require_gpu(x)
    x = x.contiguous()
    y = torch.empty_like(x) if out is None else out          # `out`: a contiguous tensor of x's size
    _lib.call("onet_complement_clip", _p(x), _p(y), float(bias), x.numel(), _stream())
    return y


def fill(t, value):
    _lib.call("onet_fill", _p(t), float(value), t.numel(), _stream())
    return t


# ----------------------------------------------------------------------------- head / loss
HEAD_NORM = _flag("HEAD_NORM", True)      # 0: the last unit's BatchNorm + ReLU pass writes its activation for the head to read


def head_softmax_fwd(Lt, Ht, Ld, Hd, want_sums=False, h_norm=None):
    """-> Vt, Vd, S  (+ sLt, sLd = per-pixel channel sums of Lt / Ld, [B,1,H,W], when want_sums).
    h_norm = (save_t, save_d): Ht / Hd are the pre-activations of the last unit, normalised + rectified on load."""
    require_gpu(Lt, Ht, Ld, Hd)
    Lt, a = plane(Lt)
    Ht, b = plane(Ht)
    Ld, c = plane(Ld)
    Hd, d = plane(Hd)
    B, C, H, W = Lt.shape
    dev = Lt.device
    Vt = torch.empty((B, 1, H, W), dtype=F32, device=dev)
    Vd = torch.empty((B, 1, H, W), dtype=F32, device=dev)
    S = torch.empty((B, 2, H, W), dtype=F32, device=dev)
    sLt = torch.empty((B, 1, H, W), dtype=F32, device=dev) if want_sums else None
    sLd = torch.empty((B, 1, H, W), dtype=F32, device=dev) if want_sums else None
    nt, nd = h_norm if h_norm is not None else (None, None)
    _lib.call("onet_head_softmax_fwd", _p(Lt), a, _p(Ht), b, _p(Ld), c, _p(Hd), d, _p(Vt), _p(Vd), _p(S), _p(sLt), _p(sLd), _p(nt), _p(nd),
              B, C, H * W, _stream(), nbytes=16 * Lt.numel())
    return (Vt, Vd, S, sLt, sLd) if want_sums else (Vt, Vd, S)


def head_softmax_bwd(dVt, dVd, dS, S, Lt, Ht, Ld, Hd, twin=False, gsums=(None, None), h_norm=None):
    """-> dLt, dHt, dLd, dHd; twin=True: -> (dL, dH) of shape [2B, C, H, W], the top and down halves adjacent.
    gsums = (d loss / d sLt, d loss / d sLd), [B,1,H,W] each or None: added to every channel of dLt / dLd."""
    Lt, a = plane(Lt)
    Ht, b = plane(Ht)
    Ld, c = plane(Ld)
    Hd, d = plane(Hd)
    B, C, H, W = Lt.shape
    dev = Lt.device
    dVt = None if dVt is None else dVt.contiguous()
    dVd = None if dVd is None else dVd.contiguous()
    dS = None if dS is None else dS.contiguous()
    if twin:
        dL = torch.empty((2 * B, C, H, W), dtype=F32, device=dev)
        dH = torch.empty((2 * B, C, H, W), dtype=F32, device=dev)
        outs = [dL[:B], dH[:B], dL[B:], dH[B:]]
    else:
        outs = [torch.empty((B, C, H, W), dtype=F32, device=dev) for _ in range(4)]
    gst = None if gsums[0] is None else gsums[0].contiguous()
    gsd = None if gsums[1] is None else gsums[1].contiguous()
    nt, nd = h_norm if h_norm is not None else (None, None)
    _lib.call("onet_head_softmax_bwd", _p(dVt), _p(dVd), _p(dS), _p(gst), _p(gsd), _p(S), _p(Lt), a, _p(Ht), b,
              _p(Ld), c, _p(Hd), d, _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(nt), _p(nd), B, C, H * W, _stream(),
              nbytes=32 * Lt.numel())
    return (dL, dH) if twin else outs


# The twin head's backward carries the last unit's BatchNorm-backward reduce and dH = g L is never written (head_bwd_reduce; the unit's
# apply pass forms it on load, bn_relu_bwd_split(da_gl=...)).  0 (tests / A-B): head_softmax_bwd writes dH and the unit reduces it.
HEAD_BWD_FUSE = _flag("HEAD_BWD_FUSE", True)


def head_bwd_fuse_ok(L, z):
    """Do the fused head backward's 16-byte loads fit these tensors (the twin batch's L and the last unit's fp32 pre-activation z)?"""
    if L.shape != z.shape or z.dtype != F32 or L.dtype != F32 or L.shape[0] % 2 or is_placeholder(L) or is_placeholder(z):
        return False
    B, C, H, W = L.shape
    for t in (L, z):
        ok = (W == 1 or t.stride(3) == 1) and (H == 1 or t.stride(2) == W) and (C == 1 or t.stride(1) == H * W) and t.stride(0) >= C * H * W
        if not ok or t.stride(0) % 4 or t.data_ptr() % 16:
            return False
    return (H * W) % 4 == 0 and W % 4 == 0 and C % 8 == 0


def head_grad_map(dVt, dVd, dS, S):
    """The head's per-pixel gradients as one map [2B,1,H,W] (top half d loss / d Vt, down half d loss / d Vd) from the upstream
    gradients of Vt, Vd [B,1,H,W] and S [B,2,H,W] (each may be None), head_softmax_bwd's expressions."""
    B, _, H, W = S.shape
    dVt = None if dVt is None else dVt.contiguous()
    dVd = None if dVd is None else dVd.contiguous()
    dS = None if dS is None else dS.contiguous()
    S = S.contiguous()
    g = torch.empty((2 * B, 1, H, W), dtype=F32, device=S.device)
    _lib.call("onet_head_grad_map", _p(dVt), _p(dVd), _p(dS), _p(S), _p(g), B, H * W, _stream(),
              nbytes=4.0 * B * H * W * (2 + (dVt is not None) + (dVd is not None) + 4 * (dS is not None)))
    return g


def head_bwd_reduce(g, gsums, L, z, save_all, want_amax=True):
    """The twin head's backward fused with the BatchNorm-backward reduce of the unit whose pre-activation z the head normalised on load
    (save_all [2][4][C]); g: head_grad_map's map, gsums as in head_softmax_bwd.  One pass over L and z: dL = g relu(bn(z)) + gsums is
    written (head_softmax_bwd's bits), dH = g L is only summed.  -> (dL, rec4 [2 * np][C][4], da_amax | None): what
    bn_relu_bwd_split takes as rec4 / da_amax beside da_gl=(g, L)."""
    require_gpu(g, L, z)
    L, lbs = plane(L)
    z, zbs = plane(z)
    B2, C, H, W = L.shape
    HW = H * W
    dev = L.device
    assert save_all.shape == (2, 4, C) and save_all.is_contiguous() and g.is_contiguous() and g.numel() == B2 * HW
    gst = None if gsums[0] is None else gsums[0].contiguous()
    gsd = None if gsums[1] is None else gsums[1].contiguous()
    dL = torch.empty((B2, C, H, W), dtype=F32, device=dev)
    nparts = 2 * _bn_nparts(B2 // 2, HW)
    rec4 = torch.empty((nparts, C, 4), dtype=F32, device=dev)
    da_amax = new_amax(dev) if want_amax else None
    _lib.call("onet_head_bwd_reduce", _p(L), lbs, _p(z), zbs, _p(g), _p(gst), _p(gsd), _p(save_all), _p(dL), _p(rec4), nparts, _p(da_amax),
              B2, C, HW, _stream(), nbytes=12.0 * L.numel() + 4.0 * B2 * HW * (1 + (gst is not None)))
    return dL, rec4, da_amax


def _rows(t):
    """[B,1,H,W] slice of S -> (tensor, batch stride) with the H*W block contiguous."""
    B, C, H, W = t.shape
    assert C == 1
    ok = (W == 1 or t.stride(3) == 1) and (H == 1 or t.stride(2) == W)
    if not ok:
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else H * W)


def jsd_fwd(L, Si, Sp, sums=None):
    """one jsd term; `sums` given ([B,1,H,W] contiguous channel sums from the head kernel): L is not read (may be None)."""
    require_gpu(Si, Sp)
    Si, ibs = _rows(Si)
    Sp, pbs = _rows(Sp)
    if sums is not None:
        B, _, H, W = sums.shape
        C, lbs, L = 1, 0, None
        dev = sums.device
        sums = sums.contiguous()
    else:
        require_gpu(L)
        L, lbs = plane(L)
        B, C, H, W = L.shape
        dev = L.device
        sums = torch.empty(B * H * W, dtype=F32, device=dev)
    part = torch.empty(_lib.load().onet_jsd_nparts(), dtype=torch.float64, device=dev)
    out = torch.empty((), dtype=F32, device=dev)
    _lib.call("onet_jsd_fwd", _p(L), lbs, _p(Si), ibs, _p(Sp), pbs, _p(sums), _p(part), _p(out), B, C, H * W,
              _stream())
    return out, sums


def jsd_bwd(g, sums, Si, Sp, shape):
    B, C, H, W = shape
    Si, ibs = _rows(Si)
    Sp, pbs = _rows(Sp)
    dev = sums.device
    g = g.contiguous()
    gL = torch.empty((B, 1, H, W), dtype=F32, device=dev)
    dSi = torch.empty((B, 1, H, W), dtype=F32, device=dev)
    dSp = torch.empty((B, 1, H, W), dtype=F32, device=dev)
    _lib.call("onet_jsd_bwd", _p(g), _p(sums), _p(Si), ibs, _p(Sp), pbs, _p(gL), _p(dSi), _p(dSp), B, H * W,
              _stream())
    return gL, dSi, dSp


def log1pexp_(x):
    require_gpu(x)
    if not x.is_contiguous():
        raise ValueError("log1pexp_: contiguous tensor required (it is mutated in place)")
    _lib.call("onet_log1pexp_inplace", _p(x), x.numel(), _stream())
    return x


def log1pexp_bwd(x_orig, g):
    g = g.contiguous()
    out = torch.empty_like(x_orig)
    _lib.call("onet_log1pexp_bwd", _p(x_orig), _p(g), _p(out), x_orig.numel(), _stream())
    return out


def argmax2(S):
    require_gpu(S)
    S = S.contiguous()
    B, C, H, W = S.shape
    if C != 2:
        raise ValueError("argmax2: S must have 2 channels")
    Y = torch.empty((B, H, W), dtype=torch.int64, device=S.device)
    _lib.call("onet_argmax2", _p(S), _p(Y), B, H * W, _stream())
    return Y


def softmax2_labels(Vt, Vd, want_S=True, want_labels=True):
    """-> (S [B, 2, H, W] | None, Y int64 [B, H, W] | None) from the head's Vt, Vd [B, 1, H, W]: S by head_softmax_fwd's expressions,
    Y = argmax2(S) (ties -> 0), in one streaming launch; an output that is not wanted is neither allocated nor written."""
    require_gpu(Vt, Vd)
    if Vt.shape != Vd.shape or Vt.dim() != 4 or Vt.shape[1] != 1 or Vt.dtype != F32 or Vd.dtype != F32:
        raise ValueError("softmax2_labels: Vt and Vd must be fp32 [B, 1, H, W] tensors of one shape")
    if not (want_S or want_labels):
        raise ValueError("softmax2_labels: nothing asked for")
    Vt, Vd = Vt.contiguous(), Vd.contiguous()
    B, _, H, W = Vt.shape
    S = torch.empty((B, 2, H, W), dtype=F32, device=Vt.device) if want_S else None
    Y = torch.empty((B, H, W), dtype=torch.int64, device=Vt.device) if want_labels else None
    _lib.call("onet_softmax2_labels", _p(Vt), _p(Vd), _p(S), _p(Y), B, H * W, _stream(),
              nbytes=4.0 * B * H * W * (2 + 2 * want_S + 2 * want_labels))
    return S, Y


# dtype codes of a label map (include/onet_hip_eval.h): read in place, no conversion pass
_LABEL_DTYPES = {torch.uint8: 0, torch.bool: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}


def _label_map(t, B, HW, what):
    """-> (tensor, dtype code, batch stride in elements) of a label map of B images of HW elements, each image contiguous (a batch
    slice of a wider tensor is read where it lies; anything else is copied)"""
    require_gpu(t)
    if t.dtype not in _LABEL_DTYPES:
        raise TypeError(f"{what}: label maps are uint8 / bool, int32, int64 or float32, not {t.dtype}")
    if t.dim() < 2 or t.shape[0] != B or t.numel() != B * HW:
        raise ValueError(f"{what}: a label map of {B} images of {HW} elements expected, got {tuple(t.shape)}")
    if not t[0].is_contiguous() or (B > 1 and t.stride(0) < HW):
        t = t.contiguous()
    return t, _LABEL_DTYPES[t.dtype], (t.stride(0) if B > 1 else HW)


def _count_rows(counts, row, B, what):
    if counts.dtype != torch.int64 or counts.dim() != 2 or counts.shape[1] != 4 or not counts.is_cuda or not counts.is_contiguous():
        raise ValueError(f"{what}: counts must be a contiguous int64 [n, 4] tensor on the GPU")
    if row < 0 or row + B > counts.shape[0]:
        raise ValueError(f"{what}: rows [{row}, {row + B}) outside a counts tensor of {counts.shape[0]} rows")
    return counts.data_ptr() + 32 * row


def score_counts(Vt, Vd, gt, counts, row=0, want_S=False, want_labels=False):
    """The validation step in one launch: per-image confusion counts (TP, FP, FN, TN) of the head's labels of Vt, Vd [B, 1, H, W]
    against the ground truth `gt` (B images in its own dtype, positive where != 0), ADDED to rows [row, row + B) of `counts` (int64
    [n, 4]: the caller zeroes it once per epoch).  -> (S [B, 2, H, W] | None, Y int64 [B, H, W] | None): softmax2_labels' bits, written
    by the same launch where asked for."""
    require_gpu(Vt, Vd)
    if Vt.shape != Vd.shape or Vt.dim() != 4 or Vt.shape[1] != 1 or Vt.dtype != F32 or Vd.dtype != F32:
        raise ValueError("score_counts: Vt and Vd must be fp32 [B, 1, H, W] tensors of one shape")
    Vt, Vd = Vt.contiguous(), Vd.contiguous()
    B, _, H, W = Vt.shape
    gt, code, gbs = _label_map(gt, B, H * W, "score_counts")
    dst = _count_rows(counts, row, B, "score_counts")
    S = torch.empty((B, 2, H, W), dtype=F32, device=Vt.device) if want_S else None
    Y = torch.empty((B, H, W), dtype=torch.int64, device=Vt.device) if want_labels else None
    _lib.call("onet_score_counts", _p(Vt), _p(Vd), _p(gt), code, gbs, _p(S), _p(Y), dst, B, H * W, _stream(),
              nbytes=B * H * W * (4.0 * (2 + 2 * want_S + 2 * want_labels) + gt.element_size()))
    return S, Y


def label_counts(pred, gt, counts, row=0):
    """Per-image confusion counts of a label map `pred` against `gt` (B images each, any of the label dtypes, read in place), ADDED to
    rows [row, row + B) of `counts` like score_counts.  -> counts"""
    B = pred.shape[0]
    HW = pred.numel() // max(B, 1)
    pred, pcode, pbs = _label_map(pred, B, HW, "label_counts")
    gt, gcode, gbs = _label_map(gt, B, HW, "label_counts")
    dst = _count_rows(counts, row, B, "label_counts")
    _lib.call("onet_label_counts", _p(pred), pcode, pbs, _p(gt), gcode, gbs, dst, B, HW, _stream(),
              nbytes=float(B * HW * (pred.element_size() + gt.element_size())))
    return counts


# per image and block of onet_snr_moments' fixed partition (include/onet_hip_verify.h): 9 doubles and 4 floats, at most 64 blocks
_SNR_WS_PER_IMAGE = 64 * (9 * 8 + 4 * 4)


def _scores_pair(Vt, Vd, what):
    require_gpu(Vt, Vd)
    if Vt.shape != Vd.shape or Vt.dim() != 4 or Vt.shape[1] != 1 or Vt.dtype != F32 or Vd.dtype != F32:
        raise ValueError(f"{what}: Vt and Vd must be fp32 [B, 1, H, W] tensors of one shape")
    return Vt.contiguous(), Vd.contiguous()


def _minmax_rows(minmax, B, device, what):
    if minmax is None:
        return torch.empty((B, 4), dtype=F32, device=device)
    if minmax.dtype != F32 or tuple(minmax.shape) != (B, 4) or not minmax.is_cuda or not minmax.is_contiguous():
        raise ValueError(f"{what}: minmax must be a contiguous fp32 [{B}, 4] tensor on the GPU")
    return minmax


def snr_moments(X, Vt, Vd, gt, moments, row=0, minmax=None):
    """What get_psnr (UT:457-476) is made of, per image, in one call: rows [row, row + B) of `moments` (fp64 [n, 9]) are WRITTEN with
    (sum v^2 on the target, sum v^2 off it, max(0, max v on it)) of X as it is, of n(Vt) and of n(Vd) -- n = tensor_normal_per_frame's
    expression in fp32, each square and every sum in fp64, a fixed summation order (the same bits in every run) -- and `minmax` (fp32
    [B, 4], allocated where None) with (min Vt, max Vt, min Vd, max Vd).  Vt, Vd fp32 [B, 1, H, W]; X fp32 of the same shape (a batch
    slice of a wider tensor is read where it lies) or None: its three values are written as 0; gt as score_counts takes it.
    -> minmax"""
    Vt, Vd = _scores_pair(Vt, Vd, "snr_moments")
    B, _, H, W = Vt.shape
    x_bs = H * W
    if X is not None:
        require_gpu(X)
        if X.shape != Vt.shape or X.dtype != F32:
            raise ValueError(f"snr_moments: X must be an fp32 tensor of Vt's shape {tuple(Vt.shape)}, got {tuple(X.shape)}")
        if not X[0].is_contiguous() or (B > 1 and X.stride(0) < H * W):
            X = X.contiguous()
        x_bs = X.stride(0) if B > 1 else H * W
    gt, code, gbs = _label_map(gt, B, H * W, "snr_moments")
    if moments.dtype != torch.float64 or moments.dim() != 2 or moments.shape[1] != 9 or not moments.is_cuda or not moments.is_contiguous():
        raise ValueError("snr_moments: moments must be a contiguous float64 [n, 9] tensor on the GPU")
    if row < 0 or row + B > moments.shape[0]:
        raise ValueError(f"snr_moments: rows [{row}, {row + B}) outside a moments tensor of {moments.shape[0]} rows")
    minmax = _minmax_rows(minmax, B, Vt.device, "snr_moments")
    ws = workspace(B * _SNR_WS_PER_IMAGE, Vt.device)
    _lib.call("onet_snr_moments", _p(X), x_bs, _p(Vt), _p(Vd), _p(gt), code, gbs, moments.data_ptr() + 72 * row, _p(minmax), B, H * W,
              _p(ws), ws.numel() * 4, _stream(),
              nbytes=B * H * W * (4.0 * (4 + (X is not None)) + gt.element_size()))
    return minmax


def cascade_input(Vt, Vd, counts, minmax=None, out=None):
    """The two-stage cascade's second input (TS:327-332) without the host round trip: X2 = n(Vt) where the hard re-assignment flips
    this batch's labels, n(Vd) where it keeps them -- the decision is read on the device from `counts`, the batch's B int64
    (TP, FP, FN, TN) rows as score_counts left them: flip = (sum TP + sum TN) < (sum FP + sum FN).  minmax: snr_moments' [B, 4], or
    None: the kernel finds the selected frames' min / max itself.  -> X2 fp32 [B, 1, H, W] (`out` where given)"""
    Vt, Vd = _scores_pair(Vt, Vd, "cascade_input")
    B, _, H, W = Vt.shape
    if counts.dtype != torch.int64 or tuple(counts.shape) != (B, 4) or not counts.is_cuda or not counts.is_contiguous():
        raise ValueError(f"cascade_input: counts must be the batch's contiguous int64 [{B}, 4] rows on the GPU")
    if minmax is not None:
        minmax = _minmax_rows(minmax, B, Vt.device, "cascade_input")
    if out is None:
        out = torch.empty_like(Vt)
    elif out.shape != Vt.shape or out.dtype != F32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"cascade_input: out must be a contiguous fp32 tensor of Vt's shape {tuple(Vt.shape)} on the GPU")
    _lib.call("onet_cascade_input", _p(Vt), _p(Vd), _p(minmax), _p(counts), _p(out), B, H * W, _stream(),
              nbytes=B * H * W * (8.0 if minmax is not None else 12.0))
    return out


# ----------------------------------------------------------------------------- optimizer
def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """one torch.optim.Adam step over flat buffers; the hyper-parameters go down as doubles (include/onet_hip_optim.h)"""
    require_gpu(p, g, m, v)
    _lib.call("onet_adam_step_f64", _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2),
              float(eps), float(weight_decay), int(step), float(grad_scale), _stream(), nbytes=28 * p.numel())
