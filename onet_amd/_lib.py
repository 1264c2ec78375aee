"""ctypes binding of libonet_hip.so (C ABI: include/onet_hip.h, include/onet_hip_eval.h for the validation step and
include/onet_hip_ragged.h / include/onet_hip_ragged_split.h for the one-part / fp16 two-part eval plan on ragged maps,
include/onet_hip_anymap.h for the one-part plan's levels on maps of any size, include/onet_hip_pairs.h for its bottom level on
image-pair tiles, include/onet_hip_upmap.h for its ConvTranspose2d edges on maps of any size, include/onet_hip_split_pairs.h for the
fp16 two-part plan's bottom level on image-pair tiles, include/onet_hip_verify.h for the SNR-gain report and the cascade).

The prototypes are PARSED from the header, so the Python side cannot drift from
the ABI.  There is no CPU fallback: if the library cannot be loaded (or built),
importing the compute path raises."""
from __future__ import annotations

import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip.h")
# the validation step's entry points: declared in a header of their own, bound by load() like the main header's
EVAL_HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip_eval.h")
# ONET_HIP_LIB: another build of the same library (onet_amd.build --variant ...) for same-box A/B runs
# the ragged-map entry points of the one-part eval plan (Settings.fused_eval = "bf16+pool+ragged"): likewise
RAGGED_HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip_ragged.h")
# ... and of the fp16 (hi | mid) plan (Settings.fused_eval = "fp16x2+ragged")
RAGGED_SPLIT_HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip_ragged_split.h")
# ... and of the one-part plan's levels below the first on maps of any size (Settings.fused_eval = "bf16+pool+anymap")
ANYMAP_HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip_anymap.h")
# ... and of its bottom level, maps 16 pixels wide or narrower on image-pair tiles (Settings.fused_eval = "bf16+pool+anymap+pairs")
PAIRS_HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip_pairs.h")
# ... and of its ConvTranspose2d edges with an odd-w input or a padded output (Settings.fused_eval = "bf16+pool+anymap+pairs+up")
UPMAP_HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip_upmap.h")
# ... and of the fp16 (hi | mid) plan's bottom level on image-pair tiles (Settings.fused_eval = "fp16x2+ragged+pairs")
SPLIT_PAIRS_HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip_split_pairs.h")
# ... and of the Adam step with its hyper-parameters in double (1 - beta rounded once, as torch.optim.Adam forms it)
OPTIM_HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip_optim.h")
# ... and of the performance report's device side: get_psnr's moments and the two-stage cascade's second input
VERIFY_HEADER = os.path.join(os.path.dirname(HERE), "include", "onet_hip_verify.h")
LIBPATH = os.environ.get("ONET_HIP_LIB") or os.path.join(HERE, "libonet_hip.so")

_CT = {
    "int": ctypes.c_int,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
}


def parse_header(path: str = HEADER):
    """-> {name: (restype, [argtypes], [argnames])} for every prototype in the header."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)
    protos = {}
    for m in re.finditer(r"((?:const\s+)?\w+\s*\*?)\s*(onet_\w+)\s*\(([^)]*)\)\s*;", src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret.endswith("*"):
            restype = ctypes.c_char_p if "char" in ret else ctypes.c_void_p
        else:
            restype = _CT[ret]
        argtypes, argnames = [], []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                mm = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)$", a)
                if not mm:
                    raise ValueError(f"cannot parse argument {a!r} of {name}")
                base, ptr, an = mm.groups()
                argtypes.append(ctypes.c_void_p if ptr else _CT[base])
                argnames.append(an)
        protos[name] = (restype, argtypes, argnames)
    return protos


class OnetHipError(RuntimeError):
    pass


_lib = None
_protos = None


def load(build_if_missing: bool = True):
    """Load (building in-tree first if needed) libonet_hip.so.  Raises if impossible."""
    global _lib, _protos
    if _lib is not None:
        return _lib
    if not os.path.exists(LIBPATH):
        if not build_if_missing:
            raise OnetHipError(f"{LIBPATH} not built; run `python -m onet_amd.build`")
        from . import build as _build
        _build.build()
    lib = ctypes.CDLL(LIBPATH)
    _protos = {}
    for header in (HEADER, EVAL_HEADER, RAGGED_HEADER, RAGGED_SPLIT_HEADER, ANYMAP_HEADER, PAIRS_HEADER, UPMAP_HEADER, SPLIT_PAIRS_HEADER, OPTIM_HEADER, VERIFY_HEADER):
        protos = parse_header(header)
        for name, (restype, argtypes, _) in protos.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:  # header/ABI drift must be loud
                raise OnetHipError(f"libonet_hip.so does not export {name} declared in {os.path.basename(header)}") from e
            fn.restype = restype
            fn.argtypes = argtypes
        _protos.update(protos)
    _lib = lib
    return lib


def last_error() -> str:
    return load().onet_last_error().decode()


# Optional per-launch timing hook (bench.py): an object with begin() -> token and end(name, nbytes, token), installed by
# onet_amd.ops while a profile is being taken.  None (default): no overhead.
PROFILE_HOOK = None


def call(name: str, *args, nbytes=None):
    """Call an int-returning entry point; raise OnetHipError on a negative code.  `nbytes`: the algorithmic HBM bytes of
    this launch (streaming kernels), recorded with its duration when a profile hook is installed."""
    lib = load()
    hook = PROFILE_HOOK
    tok = hook.begin() if hook is not None else None
    rc = getattr(lib, name)(*args)
    if tok is not None:
        hook.end(name, nbytes, tok)
    if rc != 0:
        raise OnetHipError(f"{name} failed ({rc}): {lib.onet_last_error().decode()}")
    return rc
