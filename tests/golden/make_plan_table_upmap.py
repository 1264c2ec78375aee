"""Writes fused_eval_plans_upmap.json: make_plan_table.py's table (the same stub of 256 compute units, the same models and heads) for
Settings.fused_eval = "bf16+pool+anymap+pairs+up" under conv "auto" and "bf16", over the inputs whose ConvTranspose2d edges the value
moves onto the slot-operand GEMM (200 x 200: up1 padded 12 -> 25, up2 from the odd-w 25-pixel map; 48 x 200 and 40 x 200: the same two
edges on 3 x 12 / 2 x 12 bottom levels, the second padded both ways) and three that have no such edge (224 x 224, 256 x 256,
512 x 512) -- those answer as "bf16+pool+anymap+pairs" does.  tests/test_upmap_eval_host.py reruns table() and requires equality with
the file.

    python tests/golden/make_plan_table_upmap.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fused_eval_plans_upmap.json")

VALUE = "bf16+pool+anymap+pairs+up"
SETTINGS = (dict(fused_eval=VALUE), dict(conv="bf16", fused_eval=VALUE))
SHAPES = ((32, 1, 200, 200), (1, 1, 48, 200), (1, 3, 40, 200), (1, 1, 224, 224), (4, 1, 256, 256), (1, 3, 512, 512))


def table(settings=SETTINGS, shapes=SHAPES):
    """make_plan_table.table() over `settings` x `shapes` (a private copy of that module: its own tables stay as they are)"""
    spec = importlib.util.spec_from_file_location("make_plan_table_for_upmap", os.path.join(HERE, "make_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.SETTINGS, mod.SHAPES = tuple(settings), tuple(shapes)
    return mod.table()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
