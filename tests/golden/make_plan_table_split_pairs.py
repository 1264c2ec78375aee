"""Writes fused_eval_plans_split_pairs.json: make_plan_table.py's table (the same stub of 256 compute units, the same models and heads)
for Settings.fused_eval = "fp16x2+ragged+pairs" under conv "auto" and "split", over the two resolutions whose bottom level the value
adds (224 x 224: 14 x 14; 256 x 256: 16 x 16) and 200 x 200, whose plan it leaves at depth 2 (the fp16 plan has no any-map levels).
tests/test_split_pairs_eval_host.py reruns table() and requires equality with the file.

    python tests/golden/make_plan_table_split_pairs.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fused_eval_plans_split_pairs.json")

VALUE = "fp16x2+ragged+pairs"
SETTINGS = (dict(fused_eval=VALUE), dict(conv="split", fused_eval=VALUE))
SHAPES = ((32, 1, 224, 224), (32, 1, 256, 256), (16, 3, 224, 224), (32, 1, 200, 200))


def table(settings=SETTINGS, shapes=SHAPES):
    """make_plan_table.table() over `settings` x `shapes` (a private copy of that module: its own tables stay as they are)"""
    spec = importlib.util.spec_from_file_location("make_plan_table_for_split_pairs", os.path.join(HERE, "make_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.SETTINGS, mod.SHAPES = tuple(settings), tuple(shapes)
    return mod.table()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
