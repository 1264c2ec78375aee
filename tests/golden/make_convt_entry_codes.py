"""Writes convt_entry_codes.json: what the four slot-operand ConvTranspose2d forward entries of libonet_hip.so answer on arguments that
never launch -- the return code (1: outside the domain, nothing done; -1: an error) and, for -1, the text of onet_last_error() --
recorded before the entries became rows of one checked launch path (convt_gemm.hip, convt_slots).  Pointers are the sentinel address
16: non-null, 16-byte aligned, never dereferenced on the host.  No case lies inside a domain with good arguments; no GPU is needed.
tests/test_convt_table_host.py reruns table() and requires equality with the file.

    python tests/golden/make_convt_entry_codes.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "convt_entry_codes.json")

_IN = ["xP", "xP_bs"]
_OUT = ["wP", "bias", "yP", "yP_bs"]
_SHAPE = ["B", "Cin", "Ct", "h", "w"]
ARGS = {"onet_convT2x2_fwd_slots": _IN + ["x_amax"] + _OUT + ["y_amax", "nparts"] + _SHAPE + ["stream"],
        "onet_convT2x2_fwd_slots_ragged": _IN + _OUT + _SHAPE + ["stream"],
        "onet_convT2x2_fwd_slots_split_ragged": _IN + ["x_amax"] + _OUT + ["y_amax", "nparts"] + _SHAPE + ["stream"],
        "onet_convT2x2_fwd_slots_anymap": _IN + _OUT + _SHAPE + ["Ho", "Wo", "stream"]}
# entry -> its good maps (h, w, Ho - 2h, Wo - 2w): the entry's own, then the one it hands to a sibling's instance
MAPS = {"onet_convT2x2_fwd_slots": ((8, 16, 0, 0),),
        "onet_convT2x2_fwd_slots_ragged": ((6, 6, 0, 0), (8, 16, 0, 0)),
        "onet_convT2x2_fwd_slots_split_ragged": ((6, 6, 0, 0), (8, 16, 0, 0)),
        "onet_convT2x2_fwd_slots_anymap": ((6, 5, 1, 1), (6, 6, 0, 0))}
# the map rule of each entry: maps it does not take
OFF_MAP = {"onet_convT2x2_fwd_slots": (dict(h=6, w=6), dict(h=128, w=1), dict(h=25, w=25)),
           "onet_convT2x2_fwd_slots_ragged": (dict(h=6, w=5), dict(h=128, w=1)),
           "onet_convT2x2_fwd_slots_split_ragged": (dict(h=6, w=5), dict(h=128, w=1)),
           "onet_convT2x2_fwd_slots_anymap": (dict(padH=2), dict(padH=-1), dict(padW=2), dict(padW=-1), dict(padH=2, padW=2), dict(halve=1))}


def _good(entry, nparts, h, w, ph, pw, Cin=128, Ct=64):
    """good arguments of `entry` on an h x w map (any-map: into 2h + ph x 2w + pw), with the smallest batch strides (4-byte units)"""
    Ho, Wo = 2 * h + ph, 2 * w + pw
    return dict(xP=16, xP_bs=Cin * h * w * nparts // 2, x_amax=16, wP=16, bias=16, yP=16, yP_bs=(Ct // 8) * Ho * Wo * 4 * nparts, y_amax=16,
                nparts=nparts, B=2, Cin=Cin, Ct=Ct, h=h, w=w, Ho=Ho, Wo=Wo, stream=None)


def never_launches(entry, a):
    """Do the arguments `a` of `entry` end before a launch?  Written from the headers' contracts, independently of the library: a null
    pointer or a non-positive size, a map, channel count, alignment or byte count outside the domain, or a batch stride below the
    tensor's size.  Every case is held to this BEFORE the library sees it."""
    nparts = a.get("nparts", 1)
    if None in (a["xP"], a["wP"], a["yP"]) or min(a[k] for k in _SHAPE + ["Ho", "Wo"]) <= 0 or nparts not in (1, 2):
        return True
    Cin, Ct, h, w, Ho, Wo = (a[k] for k in ("Cin", "Ct", "h", "w", "Ho", "Wo"))
    if entry.endswith("split_ragged") and nparts != 2:
        return True
    if Cin % 32 or Cin < 128 or Ct % 32 or any(a[k] % 16 for k in ("xP", "wP", "yP")) or a["xP_bs"] % 4 or a["yP_bs"] % 4:
        return True
    if Cin * h * w * 2 * nparts >= 2 ** 31 or Cin * 4 * Ct * 2 * nparts >= 2 ** 31:
        return True
    if entry.endswith("anymap"):
        if Ho - 2 * h not in (0, 1) or Wo - 2 * w not in (0, 1):
            return True
    elif w % 2 or (entry.endswith("fwd_slots") and (h * w) % 128):
        return True
    return a["xP_bs"] < Cin * h * w * nparts // 2 or a["yP_bs"] < (Ct // 8) * Ho * Wo * 4 * nparts


def _cases(entry, nparts):
    """-> {case name: argument dict}: each one change (or a named pair of changes) away from good arguments"""
    anymap = "Ho" in ARGS[entry]
    out = {}
    for h0, w0, ph, pw in MAPS[entry]:
        def make(d_xbs=0, d_ybs=0, padH=ph, padW=pw, halve=False, h=h0, w=w0, Cin=128, Ct=64, **kw):
            # (the strides follow the shape, so that a case fails the one check it names)
            a = _good(entry, nparts, max(h, 1), max(w, 1), ph, pw, max(Cin, 1), max(Ct, 8))
            a.update(h=h, w=w, Cin=Cin, Ct=Ct, xP_bs=a["xP_bs"] + d_xbs, yP_bs=a["yP_bs"] + d_ybs)
            if anymap:
                a.update(Ho=h if halve else 2 * h + padH, Wo=w if halve else 2 * w + padW)
            a.update(kw)
            return a
        t = f"nparts={nparts} {h0}x{w0}+{ph}+{pw}: "
        # the domain: channels, the map rule, alignment, the two byte counts
        for k, v in (("Cin", 144), ("Cin", 96), ("Cin", 64), ("Ct", 48), ("Ct", 16)):
            out[t + f"{k}={v}"] = make(**{k: v})
        for off in OFF_MAP[entry]:
            out[t + "map " + ",".join(f"{k}={v}" for k, v in off.items())] = make(**off)
        for k, v in (("xP", 8), ("xP", 24), ("wP", 4), ("wP", 40), ("yP", 24), ("yP", 2)):
            out[t + f"{k}={v}"] = make(**{k: v})
        for k in ("d_xbs", "d_ybs"):
            for v in (1, 2, 3):
                out[t + f"{k}=+{v}"] = make(**{k: v})
        big = 1 << (11 if nparts == 1 else 10)                       # Cin h w 2 nparts = 2^31 at Cin = 128 (h w % 128 == 0, even w)
        out[t + "input bytes = 2^31"] = make(h=1 << 12, w=big)
        out[t + "input bytes < 2^31, short stride"] = make(h=(1 << 12) - 1, w=big, d_xbs=-4)
        out[t + "weight bytes = 2^31"] = make(Cin=16384 // nparts, Ct=16384)
        out[t + "weight bytes < 2^31, short stride"] = make(Cin=16384 // nparts, Ct=16352, d_ybs=-4)
        # bad arguments: nulls, sizes, nparts
        for k in ("xP", "wP", "yP"):
            out[t + f"{k}=NULL"] = make(**{k: None})
        for k in _SHAPE + (["Ho", "Wo"] if anymap else []):
            for v in (0, -1):
                out[t + f"{k}={v}"] = make(**{k: v})
        if "nparts" in ARGS[entry]:
            for v in (0, 3):
                out[t + f"nparts={v}"] = make(nparts=v)
        # short strides
        for k in ("d_xbs", "d_ybs"):
            for v in (-4, -8):
                out[t + f"{k}={v}"] = make(**{k: v})
        if anymap and (ph or pw):
            out[t + "the dense output's stride"] = make(yP_bs=(64 // 8) * (2 * h0) * (2 * w0) * 4)
        # the order of the checks: bad arguments before the domain, the domain before the strides
        out[t + "xP=NULL outside the domain"] = make(xP=None, Cin=96)
        out[t + "B=0 outside the domain"] = make(B=0, Ct=48)
        out[t + "short stride outside the domain"] = make(Cin=96, d_xbs=-64)
        out[t + "short stride, misaligned"] = make(yP=24, d_ybs=-4)
    return out


def cases():
    """-> {entry: {case name: [argument, ...] in the prototype's order}}"""
    out = {}
    for entry, args in ARGS.items():
        out[entry] = {}
        for nparts in ((1, 2) if "nparts" in args else (1,)):
            if entry.endswith("split_ragged") and nparts == 1:
                # one part is outside this entry's domain whatever else holds: good arguments included (1, nothing launched)
                out[entry]["nparts=1 6x6+0+0: good arguments"] = _good(entry, 1, 6, 6, 0, 0)
            out[entry].update(_cases(entry, nparts))
        for name, a in out[entry].items():
            assert never_launches(entry, a), (entry, name)
        out[entry] = {name: [a[k] for k in args] for name, a in out[entry].items()}
    return out


def table():
    """-> {entry: {case name: [return code, error text | None]}}"""
    from onet_amd import _lib
    lib = _lib.load()
    out = {}
    for entry, cs in cases().items():
        out[entry] = {}
        for name, a in cs.items():
            rc = getattr(lib, entry)(*a)
            assert rc in (1, -1), (entry, name, rc)          # (0 would have been a launch: no such case may exist)
            out[entry][name] = [rc, lib.onet_last_error().decode() if rc < 0 else None]
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
