"""Writes fused_eval_plans_anymap.json: make_plan_table.py's table (the same stub of 256 compute units, the same models and heads) for
Settings.fused_eval = "bf16+pool+anymap" under conv "auto" and "bf16", over the NAU-rain resolution 200 x 200 (levels of 200, 100, 50,
25 and 12 pixels), two smaller inputs that reach a 25-pixel level (100 x 100; 48 x 100: 12 x 25 maps), the other data sets' 224 x 224,
an input made of full tiles and one whose FIRST level is outside the ragged domain (256 x 250: level 0 keeps that domain).
tests/test_anymap_eval_host.py reruns table() and requires equality with the file.

    python tests/golden/make_plan_table_anymap.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fused_eval_plans_anymap.json")

VALUE = "bf16+pool+anymap"
SETTINGS = (dict(fused_eval=VALUE), dict(conv="bf16", fused_eval=VALUE))
SHAPES = ((32, 1, 200, 200), (1, 1, 200, 200), (1, 3, 100, 100), (2, 1, 48, 100), (32, 1, 224, 224), (1, 1, 224, 224), (4, 1, 256, 256),
          (2, 1, 256, 250))


def table(settings=SETTINGS, shapes=SHAPES):
    """make_plan_table.table() over `settings` x `shapes` (a private copy of that module: its own tables stay as they are)"""
    spec = importlib.util.spec_from_file_location("make_plan_table_for_anymap", os.path.join(HERE, "make_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.SETTINGS, mod.SHAPES = tuple(settings), tuple(shapes)
    return mod.table()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
