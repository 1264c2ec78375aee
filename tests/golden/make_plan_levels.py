"""Writes fused_eval_levels.json: what the plan record (inference._query) holds per LEVEL and the fused_eval_plans*.json tables do not --
each level's map mode, its ConvTranspose2d edge and route, whether its pooled tensor leaves as slots, and the units that keep an fp32
copy -- for every key of those seven tables (the same settings, models, shapes, heads and stub of 256 compute units: each table's own
generator runs, with the query swapped).  tests/test_plan_levels_host.py reruns table() and requires equality with the file.

    python tests/golden/make_plan_levels.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fused_eval_levels.json")

# generator -> the table it writes
TABLES = {"make_plan_table.py": "fused_eval_plans.json", "make_plan_table_ragged.py": "fused_eval_plans_ragged.json",
          "make_plan_table_ragged_fp16.py": "fused_eval_plans_ragged_fp16.json", "make_plan_table_anymap.py": "fused_eval_plans_anymap.json",
          "make_plan_table_pairs.py": "fused_eval_plans_pairs.json", "make_plan_table_upmap.py": "fused_eval_plans_upmap.json",
          "make_plan_table_split_pairs.py": "fused_eval_plans_split_pairs.json"}


def _levels(unet, shape, device=None, head=None):
    """unet_plan's signature -> one record per level 0 .. 4 (none where the plan does not run)"""
    from onet_amd import inference
    plan = inference._query(unet, shape, head, device)
    return [dict(mode=lv.mode, convt=lv.convt, route=lv.route, pooled_slots=bool(lv.pooled_slots),
                 keep_fp32=[u.name for u in lv.enc + lv.dec if u.keep_fp32]) for lv in plan.levels]


def table():
    """-> {table file: {its key: [level record]}}"""
    from onet_amd import inference
    real = inference.unet_plan
    inference.unet_plan = _levels
    out = {}
    try:
        for gen, name in TABLES.items():
            spec = importlib.util.spec_from_file_location("plan_levels_" + gen[:-3], os.path.join(HERE, gen))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            out[name] = mod.table()
    finally:
        inference.unet_plan = real
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
