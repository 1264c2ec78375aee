"""Host side of the fused eval plan on maps of any size (Settings.fused_eval = "bf16+pool+anymap"): the setting's value, the layer
predicate, the two entry points' declarations and refusals, and the plan query against tests/golden/fused_eval_plans_anymap.json
(tests/golden/make_plan_table_anymap.py; compute units stubbed to 256).  No GPU."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import pytest

VALUE = "bf16+pool+anymap"
RAGGED = "bf16+pool+ragged"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRIES = {
    "onet_conv3x3_plain16_fwd_pre_act_anymap": ["xs", "xs_bs", "wq", "save", "aP", "aP_bs", "a_amax", "a", "a_bs", "B", "Cin", "Cout", "H", "W",
                                                "stream"],
    "onet_conv3x3_plain16_fwd_pre_act_pool_anymap": ["xs", "xs_bs", "wq", "save", "aP", "aP_bs", "a_amax", "a", "a_bs", "yP", "yP_bs", "y", "y_bs",
                                                     "B", "Cin", "Cout", "H", "W", "stream"],
}


def _module(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_value_is_accepted_and_the_other_values_answer_as_before():
    import onet_amd
    from onet_amd import ops
    with ops.using(ops.Settings(fused_eval=VALUE)):
        assert (ops.fused_eval(), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged(), ops.fused_eval_anymap()) == \
            (True, "bf16", True, True, True)
    for v in (None, False, True, "bf16", "fp16x2+pool", "bf16+pool", RAGGED, "fp16x2+ragged"):           # every other value: no any-map levels
        with ops.using(ops.Settings(fused_eval=v)):
            assert ops.fused_eval_anymap() is False, v
    s = ops.Settings(conv="bf16", fused_eval=VALUE)
    assert s.replace(twin=False).fused_eval == VALUE and f"fused_eval={VALUE!r}" in repr(s)
    m = onet_amd.Onet(in_chns=1, binit=True, bshare=True).eval()
    for bad in ("bf16+pool+anymaps", "bf16+anymap", "fp16x2+anymap", "bf16+pool+ragged+anymap"):
        with ops.using(ops.Settings(fused_eval=bad)):
            with pytest.raises(ValueError, match="fused_eval"):
                ops.fused_eval_anymap()
        m.settings = ops.Settings(fused_eval=bad)
        with pytest.raises(ValueError, match="fused_eval"):
            onet_amd.fused_eval_plan(m, (2, 1, 200, 200))


def test_onet_flags_reach_the_value():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from onet_amd import ops; "
            "print(repr(ops.FUSED_EVAL), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged(), ops.fused_eval_anymap(), "
            "ops.ANYMAP_MIN_W)" % root)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ONET_FLAGS="FUSED_EVAL=" + VALUE + ",ANYMAP_MIN_W=26"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == f"{VALUE!r} bf16 True True True 26", out.stdout


def test_layer_predicate():
    """eval_layer_ok_anymap: the any-map domain above the width floor, the fill rule on cdiv tile counts under "auto", equality with
    eval_layer_ok_ragged wherever that says yes (its acceptance shapes, maps made of full tiles); eval_layer_ok_ragged answers as before"""
    from onet_amd import ops
    real = ops.n_cu
    ops.n_cu = lambda device=None: 256
    try:
        with ops.using(ops.Settings(conv="bf16", fused_eval=VALUE)):
            ok = ops.eval_layer_ok_anymap
            for H, W in ((50, 50), (25, 25), (13, 22), (12, 25), (24, 50), (25, 26), (1, 21), (3, 21)):            # outside the ragged domain
                assert ok(1, 64, 64, H, W) and not ops.eval_layer_ok_ragged(1, 64, 64, H, W), (H, W)
            for H, W in ((12, 12), (25, 16), (13, 15), (6, 12), (25, 19), (50, 18)):                                 # too narrow (W > 16, W >= 20)
                assert not ok(1, 64, 64, H, W), (H, W)
            assert not ok(1, 48, 64, 25, 25) and not ok(1, 64, 96, 25, 25) and not ok(1, 64, 64, 4097, 4097) and not ok(1, 64, 64, 0, 25)
            # the ragged predicate's acceptance shapes and refusals of its own (W <= 16 on full tiles or not): the same answer
            for H, W in ((224, 224), (112, 112), (56, 56), (28, 28), (200, 200), (100, 100), (24, 40), (12, 20), (16, 20), (256, 256), (16, 32)):
                assert ok(1, 64, 64, H, W) and ops.eval_layer_ok_ragged(1, 64, 64, H, W), (H, W)
            for H, W in ((16, 16), (8, 12), (14, 14)):
                assert not ok(1, 64, 64, H, W) and not ops.eval_layer_ok_ragged(1, 64, 64, H, W), (H, W)
            assert not ops.eval_layer_ok_ragged(1, 64, 64, 50, 50)
        with ops.using(ops.Settings(fused_eval=VALUE)):
            # "auto": tiles >= 3/4 of 256 compute units, counted as the kernel walks them -- 25 x 25 is 2 x 1 tiles per image and channel tile
            assert ops.eval_layer_ok_anymap(32, 512, 512, 25, 25) and ops.eval_layer_ok_anymap(12, 512, 512, 25, 25)
            assert not ops.eval_layer_ok_anymap(11, 512, 512, 25, 25) and not ops.eval_layer_ok_anymap(1, 64, 64, 50, 50)
            assert ops.eval_layer_ok_anymap(6, 256, 256, 50, 50) and not ops.eval_layer_ok_anymap(5, 256, 256, 50, 50)      # 4 x 2 x 4 per image
        for conv in ("auto", "bf16", "split", "direct"):
            with ops.using(ops.Settings(conv=conv, fused_eval=VALUE)):
                for B in (1, 4, 64):
                    for Cin, Cout in ((64, 64), (48, 64), (128, 96), (512, 1024)):
                        for H, W in ((16, 32), (256, 256), (224, 224), (100, 100), (28, 28), (12, 20), (23, 40), (24, 38), (8, 12)):
                            if ops._ragged_map(H, W):
                                assert ops.eval_layer_ok_anymap(B, Cin, Cout, H, W) == ops.eval_layer_ok_ragged(B, Cin, Cout, H, W), \
                                    (conv, B, Cin, Cout, H, W)
        with ops.using(ops.Settings(conv="bf16", presplit=False, fused_eval=VALUE)):
            assert not ops.eval_layer_ok_anymap(4, 64, 64, 25, 25) and not ops.eval_layer_ok_anymap(4, 64, 64, 224, 224)
        floor = ops.ANYMAP_MIN_W
        try:
            ops.ANYMAP_MIN_W = 26               # the tools' switch: the 25-pixel level is left to the fall-back, the ragged floor stays
            with ops.using(ops.Settings(conv="bf16", fused_eval=VALUE)):
                assert not ops.eval_layer_ok_anymap(1, 64, 64, 25, 25) and ops.eval_layer_ok_anymap(1, 64, 64, 50, 50)
                assert ops.eval_layer_ok_anymap(1, 64, 64, 12, 20)
        finally:
            ops.ANYMAP_MIN_W = floor
    finally:
        ops.n_cu = real


def test_entry_points_declared_bound_and_the_old_headers_unchanged():
    from onet_amd import _lib, build
    protos = _lib.parse_header(_lib.ANYMAP_HEADER)
    assert sorted(protos) == sorted(ENTRIES)
    lib, raw = _lib.load(), ctypes.CDLL(_lib.LIBPATH)
    for name, names in ENTRIES.items():
        assert protos[name][2] == names and protos[name][0] is ctypes.c_int, name
        assert hasattr(raw, name) and len(getattr(lib, name).argtypes) == len(names), name
    # each entry has the argument list of its ragged sibling
    ragged = _lib.parse_header(_lib.RAGGED_HEADER)
    for sib in ("act", "act_pool"):
        assert protos[f"onet_conv3x3_plain16_fwd_pre_{sib}_anymap"][1:] == ragged[f"onet_conv3x3_plain16_fwd_pre_{sib}_ragged"][1:], sib
    main = _lib.parse_header()
    assert len(main) == 108 and len(ragged) == 5 and len(_lib.parse_header(_lib.RAGGED_SPLIT_HEADER)) == 5
    assert sorted(_lib.parse_header(_lib.EVAL_HEADER)) == ["onet_label_counts", "onet_score_counts"]
    assert not set(ENTRIES) & (set(main) | set(ragged))
    assert lib.onet_abi_version() == 4
    # the header is a dependency of the build
    lib_t, st = os.path.getmtime(build.LIB), os.stat(_lib.ANYMAP_HEADER)
    try:
        os.utime(_lib.ANYMAP_HEADER, (lib_t + 10, lib_t + 10))
        assert build._stale()
    finally:
        os.utime(_lib.ANYMAP_HEADER, ns=(st.st_atime_ns, st.st_mtime_ns))


def test_entries_refuse_and_reject_before_a_launch():
    """outside the domain: 1, nothing dereferenced (16: a non-null, 16-byte aligned address nothing may read); bad arguments inside
    it: an error code, still without a launch.  The pooled entry's stride checks use the floor-pooled sizes"""
    from onet_amd import _lib
    lib = _lib.load()
    H, W, Cin, Cout = 25, 25, 32, 64
    n_in, n_out, n_pool = Cin * H * W // 2, Cout * H * W // 2, Cout * (H // 2) * (W // 2)
    base = dict(xs=16, xs_bs=n_in, wq=16, save=16, aP=16, aP_bs=n_out, a_amax=None, a=None, a_bs=0, yP=16, yP_bs=n_pool // 2, y=None, y_bs=0,
                B=1, Cin=Cin, Cout=Cout, H=H, W=W, stream=None)
    for name in ENTRIES:
        def f(**kw):
            return getattr(lib, name)(*[dict(base, **kw)[k] for k in ENTRIES[name]])
        assert f(Cin=48, xs_bs=48 * H * W // 2) == 1 and f(Cout=96) == 1 and f(a_amax=16) == 1 and f(H=4097, W=4097) == 1, name
        assert f(a_amax=16, H=24, W=40) == 1, name                                     # ... on a map of the ragged domain too
        assert f(xs=None) == -1 and b"null" in lib.onet_last_error(), name
        assert f(B=0) == -1 and b"bad shape" in lib.onet_last_error(), name
        assert f(H=0) == -1 and b"bad shape" in lib.onet_last_error(), name
        assert f(xs=8) == -1 and b"aligned" in lib.onet_last_error(), name
        assert f(a=18, a_bs=Cout * H * W) == -1 and b"aligned" in lib.onet_last_error(), name
        assert f(B=2, xs_bs=n_in - 4) == -1 and b"stride" in lib.onet_last_error(), name
        assert f(B=2, a=16, a_bs=Cout * H * W - 1) == -1 and b"stride" in lib.onet_last_error(), name
    pool = "onet_conv3x3_plain16_fwd_pre_act_pool_anymap"

    def g(**kw):
        return getattr(lib, pool)(*[dict(base, **kw)[k] for k in ENTRIES[pool]])
    assert g(yP=None, y=None) == -1 and b"pooled" in lib.onet_last_error()
    # 12 x 12 pooled pixels per channel, not 25 x 25 / 4: one 4-byte unit less than the floor-pooled image is too small
    assert g(B=2, yP_bs=n_pool // 2 - 4) == -1 and b"stride" in lib.onet_last_error()
    assert g(B=2, yP=None, y=16, y_bs=n_pool - 1) == -1 and b"stride" in lib.onet_last_error()
    assert g(yP=8) == -1 and b"aligned" in lib.onet_last_error()


def test_plan_table_is_the_recorded_one_and_equal_on_rerun():
    mod = _module("make_plan_table_anymap_t", "make_plan_table_anymap.py")
    got = mod.table()
    with open(mod.PATH) as f:
        assert got == json.load(f)
    assert got == mod.table()
    assert len(got) == 2 * 2 * len(mod.SHAPES) * 2
    fused = ("stem", "fused+pool", "fused", "plain+head")
    key = "in_chns=1,bshare=True | conv='bf16',fused_eval='%s' | %s | %s" % (VALUE, "%s", "%s")
    # 200 x 200: levels of 200, 100, 50 and 25 pixels, the 12-pixel level falls back
    for shape in ("32x1x200x200", "1x1x200x200"):
        p = got[key % (shape, "None")]
        assert p["fused"] and p["depth"] == 4 and p["operands"] == "bf16", p
        assert p["convt"] == {"up4": "slots", "up3": "slots", "up2": "fp32->slots", "up1": "fp32->slots"}, p
        assert p["fallback_reason"].startswith("level 4: down4.c1") and "12 x 12" in p["fallback_reason"], p
        assert all((v == "fallback") == n.startswith("down4") and (v in fused or v == "fallback") for n, v in p["layers"].items()), p
        assert p["layers"]["down3.c2"] == "fused+pool" and p["layers"]["inc.c2"] == "fused+pool" and p["layers"]["up4.c2"] == "plain+head"
    assert got[key % ("32x1x200x200", "fused")]["layers"]["up4.c2"] == "fused+head"
    # under "auto" the fill rule decides: a batch of 32 fills the chip down to the 25-pixel level, one image does not fill level 0
    p = got["in_chns=1,bshare=True | fused_eval='%s' | 32x1x200x200 | None" % VALUE]
    assert p["fused"] and p["depth"] == 4 and p["convt"]["up1"] == "fp32->slots" and p["convt"]["up2"] == "fp32->slots", p
    assert got["in_chns=1,bshare=True | fused_eval='%s' | 1x1x200x200 | None" % VALUE]["depth"] == 0
    # 100 x 100: 100, 50, 25;  48 x 100: 48 x 100, 24 x 50, 12 x 25 -- in each the edge into the 25-pixel level is "fp32->slots"
    p = got["in_chns=3,bshare=False | conv='bf16',fused_eval='%s' | 1x3x100x100 | None" % VALUE]
    assert p["fused"] and p["depth"] == 3 and p["convt"] == {"up4": "slots", "up3": "fp32->slots", "up2": "fp32->slots", "up1": "fallback"}, p
    assert "12 x 12" in p["fallback_reason"], p
    p = got[key % ("2x1x48x100", "None")]
    assert p["fused"] and p["depth"] == 3 and p["convt"] == {"up4": "slots", "up3": "fp32->slots", "up2": "fp32->slots", "up1": "fallback"}, p
    assert "6 x 12" in p["fallback_reason"], p
    # level 0 keeps the ragged domain
    p = got[key % ("2x1x256x250", "None")]
    assert not p["fused"] and p["depth"] == 0 and "W = 250" in p["reason"], p
    assert all(sorted(p) == ["batch", "convt", "depth", "fallback_reason", "fused", "layers", "operands", "reason"] for p in got.values())


def test_ragged_and_full_tile_shapes_answer_as_the_ragged_value():
    """224 x 224 and 256 x 256: the dictionaries of the new value == those of "bf16+pool+ragged", computed under that value and as
    recorded in its table; and that value still stops at depth 2 on 200 x 200, naming W = 50"""
    mod = _module("make_plan_table_anymap_t2", "make_plan_table_anymap.py")
    rag = _module("make_plan_table_ragged_t3", "make_plan_table_ragged.py")
    with open(rag.PATH) as f:
        recorded = json.load(f)
    shapes = ((32, 1, 224, 224), (1, 1, 224, 224), (1, 3, 224, 224), (4, 1, 256, 256), (4, 1, 96, 96))
    got = mod.table(shapes=shapes)
    old = mod.table(settings=(dict(fused_eval=RAGGED), dict(conv="bf16", fused_eval=RAGGED)), shapes=shapes + ((32, 1, 200, 200),))
    assert len(got) == 2 * 2 * len(shapes) * 2
    hit = 0
    for k, plan in got.items():
        k_old = k.replace(VALUE, RAGGED)
        assert plan == old[k_old] and list(plan["layers"]) == list(old[k_old]["layers"]), k
        if k_old in recorded:
            hit += 1
            assert plan == recorded[k_old], k
    assert hit == 2 * 2 * 4 * 2 and {p["depth"] for p in got.values()} == {0, 2, 3, 4}
    p = old["in_chns=1,bshare=True | conv='bf16',fused_eval='%s' | 32x1x200x200 | None" % RAGGED]
    assert p["fused"] and p["depth"] == 2 and "W = 50" in p["fallback_reason"], p
