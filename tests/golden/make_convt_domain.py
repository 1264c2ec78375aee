"""Writes convt_domain.json: the answers of the three slot-operand ConvTranspose2d edge predicates -- ops.convt_slots_ok,
ops.convt_slots_ok_ragged, ops.convt_slots_ok_anymap -- on one grid of channels, maps, parts, pad combinations, switches and conv
settings, recorded before the predicates became bindings of ops._convt_domain.  tests/test_convt_table_host.py reruns table() and
requires equality with the file.  An answer string holds one character per grid point ("1": yes, "0": no, "E": the call raises) in the
order of points(); nothing is launched.

    python tests/golden/make_convt_domain.py
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "convt_domain.json")

B = 2
CIN = (64, 96, 128, 144, 256, 1024)
CT = (16, 32, 48, 64, 512)
MAPS = ((1, 1), (6, 5), (8, 16), (12, 12), (14, 14), (16, 8), (25, 25), (32, 32), (1024, 1025))
PARTS = (1, 2, None)                # None: the argument is left to its default
PADS = (-1, 0, 1, 2)                # Ho - 2h, Wo - 2w of the any-map predicate
# (conv, CONVT_SLOTS, CONVT_BF16, presplit)
SETTINGS = tuple(itertools.product(("bf16", "split"), (True, False), (True, False), (True, False)))


def points(name):
    """The grid of predicate `name` in the order of its answer string -> [(args, kwargs)]"""
    out = []
    for Cin, Ct, (h, w) in itertools.product(CIN, CT, MAPS):
        if name == "convt_slots_ok_anymap":
            out += [((B, Cin, Ct, h, w, 2 * h + ph, 2 * w + pw), {}) for ph in PADS for pw in PADS]
        else:
            out += [((B, Cin, Ct, h, w), {} if parts is None else {"parts": parts}) for parts in PARTS]
    return out


def _answer(fn, args, kw):
    try:
        return "1" if fn(*args, **kw) else "0"
    except Exception:
        return "E"


def table():
    """-> {"conv=...,CONVT_SLOTS=...,CONVT_BF16=...,presplit=...": {predicate: answer string}}"""
    from onet_amd import ops
    names = ("convt_slots_ok", "convt_slots_ok_ragged", "convt_slots_ok_anymap")
    grids = {n: points(n) for n in names}
    real = ops.CONVT_SLOTS, ops.CONVT_BF16
    out = {}
    try:
        for conv, slots, bf16, presplit in SETTINGS:
            ops.CONVT_SLOTS, ops.CONVT_BF16 = slots, bf16
            with ops.using(ops.Settings(conv=conv, presplit=presplit)):
                out[f"conv={conv},CONVT_SLOTS={int(slots)},CONVT_BF16={int(bf16)},presplit={int(presplit)}"] = {
                    n: "".join(_answer(getattr(ops, n), a, kw) for a, kw in grids[n]) for n in names}
    finally:
        ops.CONVT_SLOTS, ops.CONVT_BF16 = real
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
