"""Host side of the slot-operand ConvTranspose2d edge table (ops.CONVT_ENTRIES, ops._convt_domain, inference._ROUTES; convt_slots in
convt_gemm.hip): the three edge predicates and the four C entries answer what they answered before they became bindings of one domain
function and rows of one launch path (tests/golden/convt_domain.json, convt_entry_codes.json, with their generators), and no recorded
plan can reach a row that does not exist.  No GPU; nothing is launched."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEC = ("up4", "up3", "up2", "up1")
ENC = ("inc", "down1", "down2", "down3", "down4")
# what a unit of each announced kind launches from ops.EVAL_ENTRIES (None: not a fused convolution)
EPILOGUE = {"fused": "act", "fused+pool": "act_pool", "fused+head": "head", "two-pass": "plain", "plain+head": "plain", "stem": None,
            "fallback": None}


def _module(file):
    spec = importlib.util.spec_from_file_location(file[:-3] + "_for_test", os.path.join(GOLDEN, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_predicates_answer_as_recorded():
    from onet_amd import ops
    gen = _module("make_convt_domain.py")
    flags = ops.CONVT_SLOTS, ops.CONVT_BF16
    got = gen.table()
    assert (ops.CONVT_SLOTS, ops.CONVT_BF16) == flags
    with open(gen.PATH) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want) and len(want) == len(gen.SETTINGS) == 16
    for key in want:
        for name, answers in want[key].items():
            pts = gen.points(name)
            assert len(answers) == len(got[key][name]) == len(pts), (key, name)
            bad = [pts[i] for i, (a, b) in enumerate(zip(got[key][name], answers)) if a != b]
            assert not bad, (key, name, len(bad), bad[:4])
    n = len(gen.CIN) * len(gen.CT) * len(gen.MAPS)
    assert len(gen.points("convt_slots_ok")) == len(gen.points("convt_slots_ok_ragged")) == 3 * n and len(gen.points("convt_slots_ok_anymap")) == 16 * n
    # the grid decides something: under the default switches every predicate says yes and no, and the switches turn all of it off
    on = want["conv=bf16,CONVT_SLOTS=1,CONVT_BF16=1,presplit=1"]
    assert all("1" in s and "0" in s and "E" not in s for s in on.values())
    assert all("1" not in s for k, v in want.items() if "CONVT_SLOTS=0" in k or "presplit=0" in k for s in v.values())
    # the bindings keep their defaults: parts = None is p16_parts(), the ragged predicate's default is one part, the backward's asks the forward's
    with ops.using(ops.Settings(conv="split")):
        assert ops.convt_slots_ok(2, 128, 64, 8, 16) == ops.convt_slots_ok(2, 128, 64, 8, 16, parts=2) is True
        assert ops.convt_slots_ok_ragged(2, 128, 64, 6, 6) == ops.convt_slots_ok_ragged(2, 128, 64, 6, 6, parts=1) is True
        assert ops.convt_bwd_slots_ok(2, 128, 64, 64, 8, 16) and not ops.convt_bwd_slots_ok(2, 128, 64, 64, 6, 6)
    assert ops._convt_domain(1, "anymap", 2, 128, 64, 6, 5, 13, 11) is True and ops._convt_domain(1, "full", 2, 128, 64, 6, 6) is False


def test_entries_answer_as_recorded():
    """return codes and error texts of the four entries on arguments that never launch (the generator holds every case to its own
    restatement of the contracts before the library sees it)"""
    gen = _module("make_convt_entry_codes.py")
    cases = gen.cases()
    got = gen.table()
    with open(gen.PATH) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want) == sorted(gen.ARGS)
    for entry in want:
        assert list(got[entry]) == list(want[entry]) == list(cases[entry]), entry
        for name, (rc, text) in want[entry].items():
            assert got[entry][name] == [rc, text], (entry, name, got[entry][name], rc, text)
            assert rc in (1, -1) and ((text is None) if rc == 1 else text.startswith(entry[len("onet_"):] + ": ")), (entry, name)
        texts = {t.split(": ", 1)[1] for _, t in want[entry].values() if t}
        assert texts == {"bad args", "batch stride too small"}, (entry, texts)
    assert want["onet_convT2x2_fwd_slots_split_ragged"]["nparts=1 6x6+0+0: good arguments"] == [1, None]


def _declared():
    """-> {entry: prototype} of every header of the library"""
    import glob
    from onet_amd import _lib
    out = {}
    for header in sorted(glob.glob(os.path.join(os.path.dirname(_lib.HEADER), "onet_hip*.h"))):
        out.update(_lib.parse_header(header))
    return out


def test_no_recorded_plan_reaches_a_missing_row():
    """every route of every recorded level is a row of inference._ROUTES; a slot route has a CONVT_ENTRIES row for the plan's slot format
    whose binding exists and whose C entry is declared and bound; every fused unit has its EVAL_ENTRIES row"""
    from onet_amd import _lib, inference, ops
    lib, declared = _lib.load(), _declared()
    for (fmt, mode), (entry, name) in ops.CONVT_ENTRIES.items():
        assert ops.eval_convt_name(fmt, mode) == name and callable(getattr(ops, name)), (fmt, mode)
        assert entry in declared and len(getattr(lib, entry).argtypes) == len(declared[entry][2]), entry
    assert sorted(ops.CONVT_ENTRIES) == [("bf16", "anymap"), ("bf16", "full"), ("bf16", "ragged"), ("fp16x2", "full"), ("fp16x2", "ragged")]
    assert ops.eval_convt_name("fp16x2", "anymap") is None and ops.eval_convt_name("bf16", "pairs") is None
    assert {r.mode for r in inference._ROUTES.values()} == {"full", "ragged", "anymap", None}
    with open(os.path.join(GOLDEN, "fused_eval_levels.json")) as f:
        tables = json.load(f)
    assert len(tables) == 7
    seen, units = set(), set()
    for table, levels in tables.items():
        with open(os.path.join(GOLDEN, table)) as f:
            plans = json.load(f)
        for key, lv in levels.items():
            operands = plans[key]["operands"]
            for k, r in enumerate(lv):
                if r["route"] is None:
                    assert r["convt"] in (None, "fallback"), (table, key, k)
                    continue
                row = inference._ROUTES[r["route"]]
                assert r["convt"] == row.convt and row.convt == ("slots" if row.mode else "fp32->slots"), (table, key, k, r)
                if row.mode is not None:
                    entry, name = ops.CONVT_ENTRIES[operands, row.mode]
                    assert callable(getattr(ops, name)) and callable(getattr(ops, row.ok)) and entry in declared and hasattr(lib, entry), (table, key, k)
                seen.add((operands, r["route"]))
            for unit, kind in plans[key]["layers"].items():
                block = unit.split(".")[0]
                k = ENC.index(block) if block in ENC else DEC.index(block)
                epilogue = EPILOGUE[kind]
                if epilogue is None:
                    continue
                mode = lv[k]["mode"]
                assert mode is not None, (table, key, unit)
                units.add((operands, mode, epilogue))
                if (mode, epilogue) == ("full", "plain"):       # the training forward's launch, not an eval entry: inference._plain_conv
                    assert callable(ops.conv3x3_split_pre) and ops.eval_conv_name(operands, mode, epilogue) is None
                    continue
                entry, _ = ops.EVAL_ENTRIES[operands, mode, epilogue]
                assert callable(getattr(ops, ops.eval_conv_name(operands, mode, epilogue))) and entry in declared and hasattr(lib, entry), (table, key, unit)
    # the recorded plans exercise every slot row and both fp32 routes
    assert {(o, inference._ROUTES[r].mode) for o, r in seen if inference._ROUTES[r].mode} == set(ops.CONVT_ENTRIES)
    assert {r for _, r in seen} == set(inference._ROUTES)
    assert len(units) >= 16, sorted(units)
