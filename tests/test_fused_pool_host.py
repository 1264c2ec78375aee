"""Host side of the pooled fused eval units (Settings.fused_eval = "fp16x2+pool" | "bf16+pool"): the setting's values, the two entry
points' declarations and argument checks, and the plan query with the pooled units in one launch.  No GPU."""
import copy
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import pytest

POOL_FORM = {True: "fp16x2+pool", "bf16": "bf16+pool"}


def test_setting_values_and_slots_unchanged():
    from onet_amd import ops
    slots = ("conv", "twin", "convt_bf16", "lazy_nan", "split", "bn_on_load", "split_f16", "grad_f16", "split_dgrad",
             "stem_fused", "sync_bn", "presplit", "z_bf16", "fused_eval")
    assert ops.Settings.__slots__ == slots                     # no field added: "+pool" is a VALUE of fused_eval
    assert ops.FUSED_EVAL is False
    for v in ("fp16x2+pool", "bf16+pool"):
        s = ops.Settings(conv="split", fused_eval=v)
        r = s.replace(twin=False)
        assert r.fused_eval == v and r.conv == "split" and r.twin is False
        assert s.replace(fused_eval=True).fused_eval is True and s.fused_eval == v
        assert f"fused_eval={v!r}" in repr(s) and f"fused_eval={v!r}" in repr(r)
    for v, want in ((None, (False, None, False)), (False, (False, None, False)), (True, (True, "fp16x2", False)),
                    ("bf16", (True, "bf16", False)), ("fp16x2+pool", (True, "fp16x2", True)), ("bf16+pool", (True, "bf16", True))):
        with ops.using(ops.Settings(fused_eval=v)):
            got = (ops.fused_eval(), ops.fused_eval_operands(), ops.fused_eval_pool())
            assert got == want and all(type(g) is type(w) for g, w in zip(got, want)), (v, got)
    assert (ops.fused_eval(), ops.fused_eval_operands(), ops.fused_eval_pool()) == (False, None, False)     # no record active


@pytest.mark.parametrize("value", ["bf16+", "fp16x2", "pool", "BF16+POOL", "true"])
def test_unknown_string_raises_where_the_setting_is_read(value):
    import onet_amd
    from onet_amd import ops
    st = ops.Settings(fused_eval=value)                        # (the record itself holds any value, as it always did)
    with ops.using(st):
        for read in (ops.fused_eval, ops.fused_eval_operands, ops.fused_eval_pool):
            with pytest.raises(ValueError, match="fused_eval"):
                read()
    m = onet_amd.Onet(in_chns=1, binit=True, bshare=True).eval()
    m.settings = st
    with pytest.raises(ValueError, match="fused_eval"):
        onet_amd.fused_eval_plan(m, (2, 1, 256, 256))


def test_onet_flags_set_the_default():
    """ONET_FLAGS is read when onet_amd.ops is imported: a fresh process per value"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from onet_amd import ops; "
            "print(repr(ops.FUSED_EVAL), ops.fused_eval(), ops.fused_eval_operands(), ops.fused_eval_pool())" % root)
    for flags, want in (("FUSED_EVAL=bf16+pool", "'bf16+pool' True bf16 True"), ("TWIN=0,FUSED_EVAL=fp16x2+pool", "'fp16x2+pool' True fp16x2 True"),
                        ("FUSED_EVAL=bf16", "'bf16' True bf16 False"), ("FUSED_EVAL=1", "True True fp16x2 False"),
                        ("FUSED_EVAL=0", "False False None False")):
        env = dict(os.environ, ONET_FLAGS=flags)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip().splitlines()[-1] == want, (flags, out.stdout)


PLAIN_ARGS = ["xs", "xs_bs", "wq", "save", "aP", "aP_bs", "a_amax", "a", "a_bs", "yP", "yP_bs", "y", "y_bs", "B", "Cin", "Cout", "H", "W", "stream"]
SPLIT_ARGS = ["xs", "xs_bs", "x_amax", "scale_always", "x_amax2", "split_ch", "wq", "save", "aP", "aP_bs", "aP_slots", "a_amax", "a", "a_bs",
              "yP", "yP_bs", "y", "y_bs", "B", "Cin", "Cout", "H", "W", "stream"]


def test_entry_points_declared_and_exported():
    from onet_amd import _lib
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIBPATH) if os.path.exists(_lib.LIBPATH) else _lib.load()
    for name, names in (("onet_conv3x3_plain16_fwd_pre_act_pool", PLAIN_ARGS), ("onet_conv3x3_split_fwd_pre_act_pool", SPLIT_ARGS)):
        assert name in protos and hasattr(lib, name), name
        assert protos[name][2] == names and len(protos[name][1]) == len(names), protos[name][2]
    assert len(PLAIN_ARGS) == 19 and len(SPLIT_ARGS) == 24
    # the neighbours keep their signatures, the ABI its version; two entries more than the 106 before
    assert len(protos["onet_conv3x3_plain16_fwd_pre_act"][1]) == 15 and len(protos["onet_conv3x3_split_fwd_pre_act"][1]) == 20
    assert len(protos) == 108
    assert _lib.load().onet_abi_version() == 4


def _plain(lib):
    """-> call(xs=.., ..) of the one-part entry on a 1 x 32 -> 64 x 16 x 32 layer; 16: a non-null, 16-byte aligned address nothing may
    dereference (every call here returns before a launch)"""
    n_in, n_out = 32 * 16 * 32 // 2, 64 * 16 * 32 // 2
    base = dict(xs=16, xs_bs=n_in, wq=16, save=16, aP=16, aP_bs=n_out, a_amax=None, a=None, a_bs=0, yP=16, yP_bs=n_out // 4, y=None, y_bs=0,
                B=1, Cin=32, Cout=64, H=16, W=32, stream=None)
    return lambda **kw: lib.onet_conv3x3_plain16_fwd_pre_act_pool(*[dict(base, **kw)[k] for k in PLAIN_ARGS])


def _split(lib):
    n_in, n_out = 16 * 16 * 32, 64 * 16 * 32
    base = dict(xs=16, xs_bs=n_in, x_amax=None, scale_always=0, x_amax2=None, split_ch=0, wq=16, save=16, aP=16, aP_bs=n_out, aP_slots=16,
                a_amax=None, a=None, a_bs=0, yP=None, yP_bs=0, y=16, y_bs=n_out // 4, B=1, Cin=16, Cout=64, H=16, W=32, stream=None)
    return lambda **kw: lib.onet_conv3x3_split_fwd_pre_act_pool(*[dict(base, **kw)[k] for k in SPLIT_ARGS])


@pytest.mark.parametrize("which", ["plain16", "split"])
def test_bad_arguments_return_error_codes_without_a_device(which):
    from onet_amd import _lib
    lib = _lib.load()
    f = _plain(lib) if which == "plain16" else _split(lib)
    required = ("xs", "wq", "save", "aP") + (("aP_slots",) if which == "split" else ())
    for name in required:                                      # each required pointer on its own
        assert f(**{name: None}) == -1 and b"null" in lib.onet_last_error(), name
    assert f(yP=None, y=None) == -1 and b"pooled" in lib.onet_last_error()
    assert f(B=0) == -1 and b"bad shape" in lib.onet_last_error()
    # outside the domain: refused (1) before anything is dereferenced or launched
    assert f(W=48) == 1 and f(Cout=96) == 1 and f(H=24) == 1
    # inside the domain: misaligned destinations and short batch strides are errors, still without a launch
    n_out = 64 * 16 * 32 // (2 if which == "plain16" else 1)
    for kw in (dict(aP=8), dict(yP=8, yP_bs=n_out // 4), dict(y=8, y_bs=64 * 8 * 16), dict(a=8, a_bs=64 * 16 * 32), dict(yP=16, yP_bs=n_out // 4 + 2),
               dict(y=16, y_bs=64 * 8 * 16 + 2)):
        assert f(**kw) == -1 and b"aligned" in lib.onet_last_error(), kw
    for kw in (dict(B=2, aP_bs=n_out - 4), dict(B=2, yP=16, yP_bs=n_out // 4 - 4), dict(B=2, y=16, y_bs=64 * 8 * 16 - 4),
               dict(B=2, a=16, a_bs=64 * 16 * 32 - 4)):
        assert f(**kw) == -1 and b"stride" in lib.onet_last_error(), kw


def _plan_table_module():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_plan_table.py")
    spec = importlib.util.spec_from_file_location("make_plan_table_pool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plan_table_with_pool_is_the_recorded_one_with_the_pooled_units_renamed(monkeypatch):
    """tests/golden/make_plan_table.py's table() over every recorded settings record whose fused_eval is True or "bf16", with that value
    replaced by its "+pool" form: the recorded plan with "two-pass" replaced by "fused+pool" and nothing else different."""
    mod = _plan_table_module()
    with open(mod.PATH) as f:
        recorded = json.load(f)
    base = [sk for sk in mod.SETTINGS if sk.get("fused_eval") in (True, "bf16")]
    assert len(base) == 5
    pooled = [dict(sk, fused_eval=POOL_FORM[sk["fused_eval"]]) for sk in base]
    monkeypatch.setattr(mod, "SETTINGS", tuple(pooled))
    got = mod.table()
    assert len(got) == len(base) * len(mod.MODELS) * len(mod.SHAPES) * len(mod.HEADS)
    by_depth, n = {}, 0
    for mk in mod.MODELS:
        for sk, pk in zip(base, pooled):
            for shape in mod.SHAPES:
                for h in mod.HEADS:
                    tail = ("x".join(map(str, shape)), str(h))
                    want = copy.deepcopy(recorded[" | ".join((mod._key(**mk), mod._key(**sk)) + tail)])
                    want["layers"] = {k: ("fused+pool" if v == "two-pass" else v) for k, v in want["layers"].items()}
                    plan = got[" | ".join((mod._key(**mk), mod._key(**pk)) + tail)]
                    assert plan == want, (mk, pk, tail, plan, want)
                    assert list(plan) == list(want) and list(plan["layers"]) == list(want["layers"]) and \
                        list(plan["convt"]) == list(want["convt"]), (mk, pk, tail)
                    assert "two-pass" not in plan["layers"].values()
                    k = sum(v == "fused+pool" for v in plan["layers"].values())
                    assert k == (min(plan["depth"], 4) if plan["fused"] else 0), (pk, tail, plan)
                    if k:
                        by_depth[plan["depth"]] = by_depth.get(plan["depth"], 0) + 1
                    n += 1
    assert n == len(got)
    assert set(by_depth) == {1, 2, 3, 4, 5}, by_depth            # the new kind at every fused depth


def test_without_pool_the_plan_dictionaries_are_the_recorded_ones():
    """the settings values of before ("+pool" absent) keep answering the recorded table (tests/test_fused_eval_host.py holds every key;
    here: no plan of theirs names the new kind)"""
    mod = _plan_table_module()
    got = mod.table()
    with open(mod.PATH) as f:
        assert got == json.load(f)
    assert not any("fused+pool" in p["layers"].values() for p in got.values())
