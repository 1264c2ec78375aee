"""Writes fused_eval_plans_ragged_fp16.json: make_plan_table.py's table (the same stub of 256 compute units, the same models and heads)
for Settings.fused_eval = "fp16x2+ragged" under conv "auto" and "split", over make_plan_table_ragged.py's shapes -- the data sets'
224 x 224 and 200 x 200, two of the existing table's ragged shapes and one made of full tiles.
tests/test_ragged_split_eval_host.py reruns table() and requires equality with the file.

    python tests/golden/make_plan_table_ragged_fp16.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fused_eval_plans_ragged_fp16.json")

VALUE = "fp16x2+ragged"
SETTINGS = (dict(fused_eval=VALUE), dict(conv="split", fused_eval=VALUE))
SHAPES = ((32, 1, 224, 224), (1, 3, 224, 224), (32, 1, 200, 200), (4, 1, 96, 96), (2, 1, 256, 250), (4, 1, 256, 256))


def table(settings=SETTINGS, shapes=SHAPES):
    """make_plan_table.table() over `settings` x `shapes` (a private copy of that module: its own tables stay as they are)"""
    spec = importlib.util.spec_from_file_location("make_plan_table_for_ragged_fp16", os.path.join(HERE, "make_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.SETTINGS, mod.SHAPES = tuple(settings), tuple(shapes)
    return mod.table()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
