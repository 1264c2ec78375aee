"""Writes fused_eval_plans.json: what inference.unet_plan answers for CPU models over settings x shapes x heads, with the device's
compute-unit count stubbed to 256 -- the plan query is a function of the module tree, the settings, the shape and n_cu() alone, so no
GPU is needed.  tests/test_fused_eval_host.py reruns table() and requires equality with the file.

    python tests/golden/make_plan_table.py
"""
import contextlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fused_eval_plans.json")

SETTINGS = (dict(fused_eval=True), dict(conv="split", fused_eval=True), dict(fused_eval="bf16"), dict(conv="bf16", fused_eval="bf16"),
            dict(conv="direct", fused_eval=True), dict())
SHAPES = ((4, 1, 256, 256), (64, 1, 256, 256), (2, 1, 128, 128), (4, 1, 96, 96), (1, 3, 512, 512), (2, 1, 256, 250), (2, 1, 64, 32),
          (2, 1, 256, 512))
HEADS = (None, "fused")
MODELS = (dict(in_chns=1, bshare=True), dict(in_chns=3, bshare=False))


def _key(**kw):
    return ",".join(f"{k}={v!r}" for k, v in kw.items()) or "-"


def table():
    """-> {"model | settings | shape | head": unet_plan's dictionary}"""
    import onet_amd
    from onet_amd import inference, ops
    real_n_cu, real_device = ops.n_cu, torch.cuda.device
    ops.n_cu = lambda device=None: 256
    torch.cuda.device = lambda device: contextlib.nullcontext()
    out = {}
    try:
        for mk in MODELS:
            m = onet_amd.Onet(**mk).eval()
            for sk in SETTINGS:
                with ops.using(ops.Settings(**sk)):
                    for shape in SHAPES:
                        for h in HEADS:
                            key = " | ".join((_key(**mk), _key(**sk), "x".join(map(str, shape)), str(h)))
                            out[key] = inference.unet_plan(m.topu, shape, device=torch.device("cuda", 0), head=h)
    finally:
        ops.n_cu, torch.cuda.device = real_n_cu, real_device
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
