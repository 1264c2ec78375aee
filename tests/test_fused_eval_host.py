"""Host side of fused eval-mode inference (Settings.fused_eval): the setting, the new entry points' declarations and argument checks,
and the plan query on a model that never touches a device."""
import ctypes
import os

import torch


def test_settings_field_defaults_round_trips_and_shows():
    from onet_amd import ops
    s = ops.Settings()
    assert s.fused_eval is None and ops.FUSED_EVAL is False
    assert ops.Settings.__slots__[-1] == "fused_eval"
    t = ops.Settings(conv="split", fused_eval=True)
    r = t.replace(twin=False)
    assert r.fused_eval is True and r.conv == "split" and r.twin is False
    assert t.replace(fused_eval=False).fused_eval is False and t.fused_eval is True
    assert "fused_eval=True" in repr(t) and "fused_eval=None" in repr(s)
    with ops.using(t):
        assert ops.fused_eval() is True
    with ops.using(s):
        assert ops.fused_eval() is False


def test_new_entry_points_declared_and_exported():
    from onet_amd import _lib
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIBPATH) if os.path.exists(_lib.LIBPATH) else _lib.load()
    for name in ("onet_conv3x3_split_fwd_pre_act", "onet_conv3x3_act_bound"):
        assert name in protos, name
        assert hasattr(lib, name), name
    assert len(protos["onet_conv3x3_split_fwd_pre_act"][1]) == 20
    assert len(protos["onet_conv3x3_act_bound"][1]) == 9
    assert _lib.load().onet_abi_version() == 4


def test_bad_arguments_return_error_codes():
    from onet_amd import _lib
    lib = _lib.load()
    rc = lib.onet_conv3x3_split_fwd_pre_act(None, 0, None, 0, None, 0, None, None, None, 0, None, None, None, 0, 1, 16, 64, 16, 32, None)
    assert rc == -1 and b"null" in lib.onet_last_error()
    rc = lib.onet_conv3x3_split_fwd_pre_act(16, 0, None, 0, None, 0, 16, 16, 16, 0, 16, None, None, 0, 0, 16, 64, 16, 32, None)
    assert rc == -1 and b"bad shape" in lib.onet_last_error()
    # outside the domain (W = 48): refused before anything is dereferenced or launched
    rc = lib.onet_conv3x3_split_fwd_pre_act(16, 0, None, 0, None, 0, 16, 16, 16, 0, 16, None, None, 0, 1, 16, 64, 16, 48, None)
    assert rc == 1
    rc = lib.onet_conv3x3_act_bound(None, 64, 16, None, None, None, 0, None, None)
    assert rc == -1 and b"bad args" in lib.onet_last_error()
    rc = lib.onet_conv3x3_act_bound(16, 64, 16, 16, 16, None, 8, 16, None)
    assert rc == -1 and b"split_ch" in lib.onet_last_error()


def test_exports():
    import onet_amd
    assert "fused_eval_plan" in onet_amd.__all__ and "segment" in onet_amd.__all__
    assert callable(onet_amd.fused_eval_plan) and callable(onet_amd.segment)


def test_plan_on_cpu_model_reports_the_reason_without_a_device():
    import onet_amd
    from onet_amd import ops
    m = onet_amd.Onet(in_chns=1, binit=True, bshare=True).eval()
    m.settings = ops.Settings(fused_eval=True)
    p = onet_amd.fused_eval_plan(m, (2, 1, 256, 256))
    assert p["fused"] is False and p["depth"] == 0 and "GPU" in p["reason"] and p["twin"] is True and p["batch"] == 4
    assert p["layers"] == {} and p["convt"] == {}
    p = onet_amd.fused_eval_plan(m, (1, 256, 256))
    assert p["fused"] is False and "4-D" in p["reason"]
    u = onet_amd.UNet(n_channels=1, bilinear=True).eval()
    assert onet_amd.fused_eval_plan(u, (2, 1, 256, 256))["fused"] is False
    # a CPU tensor still raises the module's own error: the setting adds no CPU path
    try:
        with torch.no_grad():
            m(torch.zeros(1, 1, 32, 32))
    except RuntimeError as e:
        assert "GPU" in str(e)
    else:
        raise AssertionError("a CPU forward did not raise")


def test_plan_query_table_matches_the_recorded_one():
    """inference.unet_plan over settings x shapes x heads on CPU models, compute units stubbed to 256 (tests/golden/make_plan_table.py):
    every dictionary -- keys, values, reason strings, key order -- equals the recorded table."""
    import importlib.util
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_plan_table.py")
    spec = importlib.util.spec_from_file_location("make_plan_table", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.PATH) as f:
        want = json.load(f)
    got = mod.table()
    assert list(got) == list(want)
    depths, convt, kinds = set(), set(), set()
    for key, plan in want.items():
        assert got[key] == plan, (key, got[key], plan)
        assert list(got[key]) == list(plan) and list(got[key]["layers"]) == list(plan["layers"]) and \
            list(got[key]["convt"]) == list(plan["convt"]), key
        depths.add(plan["depth"])
        convt.update(plan["convt"].values())
        kinds.update(plan["layers"].values())
    # the table covers what it is there to pin
    assert depths == {0, 1, 2, 3, 4, 5} and convt == {"slots", "fp32->slots", "fallback"}, (depths, convt)
    assert kinds == {"stem", "fused", "two-pass", "plain+head", "fused+head", "fallback"}, kinds
