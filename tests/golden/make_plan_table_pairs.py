"""Writes fused_eval_plans_pairs.json: make_plan_table.py's table (the same stub of 256 compute units, the same models and heads) for
Settings.fused_eval = "bf16+pool+anymap+pairs" under conv "auto" and "bf16", over the three resolutions whose bottom level the value
adds (200 x 200: 12 x 12; 224 x 224: 14 x 14; 256 x 256: 16 x 16), an input whose level 4 is wider than 16 pixels (512 x 512: 32 x 32)
and one whose level 3 already is too narrow (96 x 96: 12 x 12 at level 3) -- the last two answer as "bf16+pool+anymap" does.
tests/test_pairs_eval_host.py reruns table() and requires equality with the file.

    python tests/golden/make_plan_table_pairs.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fused_eval_plans_pairs.json")

VALUE = "bf16+pool+anymap+pairs"
SETTINGS = (dict(fused_eval=VALUE), dict(conv="bf16", fused_eval=VALUE))
SHAPES = ((32, 1, 200, 200), (1, 1, 224, 224), (4, 1, 256, 256), (1, 3, 512, 512), (4, 1, 96, 96))


def table(settings=SETTINGS, shapes=SHAPES):
    """make_plan_table.table() over `settings` x `shapes` (a private copy of that module: its own tables stay as they are)"""
    spec = importlib.util.spec_from_file_location("make_plan_table_for_pairs", os.path.join(HERE, "make_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.SETTINGS, mod.SHAPES = tuple(settings), tuple(shapes)
    return mod.table()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
