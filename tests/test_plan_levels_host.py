"""The fused eval plan's record per level -- map mode, ConvTranspose2d edge and route, pooled slots, fp32 copies -- against
tests/golden/fused_eval_levels.json (tests/golden/make_plan_levels.py; compute units stubbed to 256), over every key of the seven
fused_eval_plans*.json tables.  No GPU."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEC = ("up4", "up3", "up2", "up1")


def _generator():
    spec = importlib.util.spec_from_file_location("make_plan_levels_for_test", os.path.join(GOLDEN, "make_plan_levels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_levels_match_the_golden_file_and_the_plan_tables():
    gen = _generator()
    got = gen.table()
    with open(gen.PATH) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want) == sorted(gen.TABLES.values())
    for name in want:
        assert sorted(got[name]) == sorted(want[name]), name
        for key in want[name]:
            assert got[name][key] == want[name][key], (name, key)
    assert json.dumps(got, indent=1) + "\n" == open(gen.PATH).read()
    # depth and convt are held by the older tables too: the two records must agree key by key
    for name, levels in got.items():
        with open(os.path.join(GOLDEN, name)) as f:
            plans = json.load(f)
        assert sorted(plans) == sorted(levels), name
        for key, plan in plans.items():
            lv = levels[key]
            assert len(lv) in (0, 5), (name, key)
            assert not lv or plan["fused"], (name, key)
            modes = [r["mode"] for r in lv]
            assert plan["depth"] == sum(m is not None for m in modes), (name, key)
            assert all(m is not None for m in modes[:plan["depth"]]), (name, key)
            assert all(m in (None, "full", "ragged", "anymap", "pairs") for m in modes), (name, key)
            assert plan["convt"] == {DEC[k]: r["convt"] for k, r in enumerate(lv[:4])}, (name, key)
            assert not lv or (lv[4]["convt"] is None and lv[4]["route"] is None), (name, key)
