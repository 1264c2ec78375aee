"""Host side of the fp32-level fused eval plan on ragged maps (Settings.fused_eval = "fp16x2+ragged"): the setting's value, the layer
predicate, the entry points' declarations and refusals, and the plan query against tests/golden/fused_eval_plans_ragged_fp16.json
(tests/golden/make_plan_table_ragged_fp16.py; compute units stubbed to 256).  No GPU."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import pytest

VALUE = "fp16x2+ragged"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_X = ["xs", "xs_bs", "x_amax", "scale_always", "x_amax2", "split_ch", "wq"]
_T = ["B", "Cin", "Cout", "H", "W", "stream"]
ENTRIES = {
    "onet_conv3x3_split_fwd_pre_plain_ragged": _X + ["z", "z_bs"] + _T,
    "onet_conv3x3_split_fwd_pre_act_ragged": _X + ["save", "aP", "aP_bs", "aP_slots", "a_amax", "a", "a_bs"] + _T,
    "onet_conv3x3_split_fwd_pre_act_pool_ragged": _X + ["save", "aP", "aP_bs", "aP_slots", "a_amax", "a", "a_bs", "yP", "yP_bs", "y", "y_bs"] + _T,
    "onet_conv3x3_split_fwd_pre_head_ragged": _X + ["save", "L", "L_bs", "V"] + _T,
    "onet_convT2x2_fwd_slots_split_ragged": ["xP", "xP_bs", "x_amax", "wP", "bias", "yP", "yP_bs", "y_amax", "nparts", "B", "Cin", "Ct", "h", "w",
                                             "stream"],
}
SIBLINGS = {"onet_conv3x3_split_fwd_pre_act_ragged": "onet_conv3x3_split_fwd_pre_act",
            "onet_conv3x3_split_fwd_pre_act_pool_ragged": "onet_conv3x3_split_fwd_pre_act_pool",
            "onet_conv3x3_split_fwd_pre_head_ragged": "onet_conv3x3_split_fwd_pre_head",
            "onet_convT2x2_fwd_slots_split_ragged": "onet_convT2x2_fwd_slots"}


def _module(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_value_is_accepted_and_a_misspelling_raises():
    import onet_amd
    from onet_amd import ops
    assert ops._FUSED_EVAL_VALUES[VALUE] == ops._FusedEval("fp16x2", True, frozenset(("full", "ragged")), False)
    with ops.using(ops.Settings(fused_eval=VALUE)):
        assert (ops.fused_eval(), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged()) == (True, "fp16x2", True, True)
    for v, want in ((None, False), (False, False), (True, False), ("bf16", False), ("fp16x2+pool", False), ("bf16+pool", False),
                    ("bf16+pool+ragged", True)):
        with ops.using(ops.Settings(fused_eval=v)):
            assert ops.fused_eval_ragged() is want, v
    s = ops.Settings(conv="split", fused_eval=VALUE)
    assert s.replace(twin=False).fused_eval == VALUE and f"fused_eval={VALUE!r}" in repr(s)
    m = onet_amd.Onet(in_chns=1, binit=True, bshare=True).eval()
    for bad in ("fp16x2+raged", "fp16x2+pool+ragged", "bf16+ragged", "fp16+ragged", "FP16X2+RAGGED"):
        with ops.using(ops.Settings(fused_eval=bad)):
            for read in (ops.fused_eval, ops.fused_eval_pool, ops.fused_eval_ragged):
                with pytest.raises(ValueError, match="fused_eval"):
                    read()
        m.settings = ops.Settings(fused_eval=bad)
        with pytest.raises(ValueError, match="fused_eval"):
            onet_amd.fused_eval_plan(m, (2, 1, 224, 224))


def test_onet_flags_reach_the_value():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from onet_amd import ops; "
            "print(repr(ops.FUSED_EVAL), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged())" % root)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ONET_FLAGS="FUSED_EVAL=" + VALUE), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == f"{VALUE!r} fp16x2 True True", out.stdout


def test_layer_predicate():
    """eval_layer_ok_ragged_fp16: its domain, the fill rule on cdiv tile counts under "auto", equality with eval_layer_ok on maps made
    of full tiles; the existing predicates answer as before"""
    from onet_amd import ops
    real = ops.n_cu
    ops.n_cu = lambda device=None: 256
    try:
        ok = ops.eval_layer_ok_ragged_fp16
        with ops.using(ops.Settings(conv="split", fused_eval=VALUE)):
            for H, W in ((224, 224), (112, 112), (56, 56), (28, 28), (200, 200), (100, 100), (24, 40), (12, 20)):   # the acceptance shapes and below
                assert ok(1, 64, 64, H, W), (H, W)
            assert ok(1, 16, 64, 24, 40) and ok(1, 48, 64, 24, 40)                                                  # Cin % 16
            assert not ok(1, 64, 64, 14, 14) and not ok(1, 64, 64, 50, 50) and not ok(1, 64, 64, 256, 250)          # W % 4
            assert not ok(1, 64, 64, 16, 16) and not ok(1, 64, 64, 8, 12) and ok(1, 64, 64, 16, 20)                 # W > 16
            assert not ok(1, 64, 64, 23, 40) and not ok(1, 24, 64, 24, 40) and not ok(1, 64, 96, 24, 40) and not ok(1, 64, 64, 4096, 4096)
            assert not ops.eval_layer_ok(1, 64, 64, 112, 112) and not ops.eval_layer_ok_bf16(1, 64, 64, 112, 112)
            # ConvTranspose2d: the default parts keep today's answer (one part: needs the bf16 ConvTranspose2d operands), parts = 2 is new
            assert not ops.convt_slots_ok(1, 128, 64, 14, 14, parts=2) and ops.convt_slots_ok_ragged(1, 128, 64, 14, 14, parts=2)
            assert ops.convt_slots_ok_ragged(1, 128, 64, 14, 14) == ops.convt_slots_ok_ragged(1, 128, 64, 14, 14, parts=1)
            assert not ops.convt_slots_ok_ragged(1, 96, 64, 14, 14, parts=2) and not ops.convt_slots_ok_ragged(1, 128, 64, 14, 13, parts=2)
        with ops.using(ops.Settings(fused_eval=VALUE)):
            # "auto": tiles >= 3/4 of 256 compute units, counted as the kernel walks them -- 28 x 28 is 2 x 1 tiles per image and channel tile
            assert ok(32, 512, 512, 28, 28) and ok(12, 512, 512, 28, 28)
            assert not ok(11, 512, 512, 28, 28) and not ok(1, 64, 64, 224, 224)
        for conv in ("auto", "bf16", "split", "direct"):
            with ops.using(ops.Settings(conv=conv, fused_eval=VALUE)):
                for B in (1, 4, 64):
                    for Cin, Cout in ((64, 64), (48, 64), (128, 96), (512, 1024)):
                        for H, W in ((16, 32), (256, 256), (64, 32), (128, 512), (32, 64)):
                            assert ops.full_tiles(H, W)
                            assert ok(B, Cin, Cout, H, W) == ops.eval_layer_ok(B, Cin, Cout, H, W), (conv, B, Cin, Cout, H, W)
                        assert not ok(B, Cin, Cout, 16, 16)
        for st in (ops.Settings(conv="split", presplit=False, fused_eval=VALUE), ops.Settings(conv="bf16", fused_eval=VALUE)):
            with ops.using(st):
                assert not ok(4, 64, 64, 112, 112)      # no pre-split storage / one-part operands
    finally:
        ops.n_cu = real


def test_ragged_min_w_raises_the_floor():
    """RAGGED_MIN_W (ONET_FLAGS, tools/time_ragged_fp16_eval.py): the narrowest map not made of full tiles that the predicate takes"""
    from onet_amd import ops
    real = ops.RAGGED_MIN_W
    try:
        with ops.using(ops.Settings(conv="split", fused_eval=VALUE)):
            ops.RAGGED_MIN_W = 32
            assert not ops.eval_layer_ok_ragged_fp16(4, 64, 64, 28, 28) and ops.eval_layer_ok_ragged_fp16(4, 64, 64, 56, 56)
            assert ops.eval_layer_ok_ragged_fp16(4, 64, 64, 16, 32)                      # (full tiles: not this floor's business)
            ops.RAGGED_MIN_W = 128
            assert not ops.eval_layer_ok_ragged_fp16(4, 64, 64, 112, 112) and ops.eval_layer_ok_ragged_fp16(4, 64, 64, 224, 224)
    finally:
        ops.RAGGED_MIN_W = real


def test_entry_points_declared_bound_and_the_old_headers_unchanged():
    from onet_amd import _lib, build
    protos = _lib.parse_header(_lib.RAGGED_SPLIT_HEADER)
    assert sorted(protos) == sorted(ENTRIES)
    lib, raw = _lib.load(), ctypes.CDLL(_lib.LIBPATH)
    for name, names in ENTRIES.items():
        assert protos[name][2] == names and protos[name][0] is ctypes.c_int, name
        assert hasattr(raw, name) and len(getattr(lib, name).argtypes) == len(names), name
    # each entry with a full-tile sibling has exactly its argument list
    main = _lib.parse_header()
    for name, sib in SIBLINGS.items():
        assert protos[name][1:] == main[sib][1:], name
    assert len(main) == 108 and not set(ENTRIES) & set(main)
    assert sorted(_lib.parse_header(_lib.EVAL_HEADER)) == ["onet_label_counts", "onet_score_counts"]
    assert len(_lib.parse_header(_lib.RAGGED_HEADER)) == 5 and not set(ENTRIES) & set(_lib.parse_header(_lib.RAGGED_HEADER))
    assert lib.onet_abi_version() == 4
    # the header is a dependency of the build
    lib_t, st = os.path.getmtime(build.LIB), os.stat(_lib.RAGGED_SPLIT_HEADER)
    try:
        os.utime(_lib.RAGGED_SPLIT_HEADER, (lib_t + 10, lib_t + 10))
        assert build._stale()
    finally:
        os.utime(_lib.RAGGED_SPLIT_HEADER, ns=(st.st_atime_ns, st.st_mtime_ns))


def test_entries_refuse_and_reject_before_a_launch():
    """outside the ragged domain: 1, nothing dereferenced (16: a non-null, 16-byte aligned address nothing may read); bad arguments
    inside it: an error code, still without a launch.  Unlike the one-part entries, a_amax is taken."""
    from onet_amd import _lib
    lib = _lib.load()
    H, W, Cin, Cout = 24, 40, 32, 64
    n_in, n_out = Cin * H * W, Cout * H * W
    base = dict(xs=16, xs_bs=n_in, x_amax=16, scale_always=0, x_amax2=None, split_ch=0, wq=16, save=16, aP=16, aP_bs=n_out, aP_slots=16,
                a_amax=16, a=None, a_bs=0, yP=16, yP_bs=n_out // 4, y=None, y_bs=0, z=16, z_bs=n_out, L=16, L_bs=n_out, V=16, B=1, Cin=Cin,
                Cout=Cout, H=H, W=W, stream=None)
    for name in list(ENTRIES)[:4]:
        def f(**kw):
            return getattr(lib, name)(*[dict(base, **kw)[k] for k in ENTRIES[name]])
        assert f(H=23) == 1 and f(W=38) == 1 and f(Cin=24, xs_bs=24 * H * W) == 1 and f(Cout=96) == 1 and f(H=4096, W=4096) == 1, name
        assert f(xs=None) == -1 and b"null" in lib.onet_last_error(), name
        assert f(B=0) == -1 and b"bad shape" in lib.onet_last_error(), name
        assert f(xs=8) == -1 and b"aligned" in lib.onet_last_error(), name
        assert f(B=2, xs_bs=n_in - 4) == -1 and b"stride" in lib.onet_last_error(), name
        assert f(split_ch=16) == -1 and b"split_ch" in lib.onet_last_error(), name
    pool = "onet_conv3x3_split_fwd_pre_act_pool_ragged"
    assert getattr(lib, pool)(*[dict(base, yP=None, y=None)[k] for k in ENTRIES[pool]]) == -1 and b"pooled" in lib.onet_last_error()
    assert lib.onet_conv3x3_split_fwd_pre_head_ragged(*[dict(base, Cout=128)[k] for k in ENTRIES["onet_conv3x3_split_fwd_pre_head_ragged"]]) == 1
    # the one-part entries still refuse a record
    old = ["xs", "xs_bs", "wq", "save", "aP", "aP_bs", "a_amax", "a", "a_bs", "B", "Cin", "Cout", "H", "W", "stream"]
    assert lib.onet_conv3x3_plain16_fwd_pre_act_ragged(*[dict(base, xs_bs=n_in // 2, aP_bs=n_out // 2)[k] for k in old]) == -1
    assert b"a_amax" in lib.onet_last_error()
    t = dict(xP=16, xP_bs=128 * 14 * 14, x_amax=16, wP=16, bias=None, yP=16, yP_bs=64 * 4 * 14 * 14, y_amax=16, nparts=2, B=1, Cin=128, Ct=64,
             h=14, w=14, stream=None)

    def g(**kw):
        return lib.onet_convT2x2_fwd_slots_split_ragged(*[dict(t, **kw)[k] for k in ENTRIES["onet_convT2x2_fwd_slots_split_ragged"]])
    assert g(w=13) == 1 and g(Cin=96) == 1 and g(Cin=144) == 1 and g(Ct=48) == 1 and g(xP=8) == 1 and g(nparts=1) == 1
    assert g(xP=None) == -1 and g(B=0) == -1 and g(nparts=3) == -1
    assert g(B=2, xP_bs=128 * 14 * 14 - 4) == -1 and b"stride" in lib.onet_last_error()


def test_plan_table_is_the_recorded_one_and_equal_on_rerun():
    mod = _module("make_plan_table_ragged_fp16_t", "make_plan_table_ragged_fp16.py")
    got = mod.table()
    with open(mod.PATH) as f:
        assert got == json.load(f)
    assert got == mod.table()
    assert len(got) == 2 * 2 * len(mod.SHAPES) * 2
    # the acceptance shapes (floor of the predicate): 224 x 224 down to its 28-pixel level, 200 x 200 down to 100
    for conv in ("", "conv='split',"):
        key = "in_chns=1,bshare=True | " + conv + "fused_eval='%s' | %s | %s"
        p = got[key % (VALUE, "32x1x224x224", "fused")]
        assert p["fused"] and p["depth"] == 4 and p["operands"] == "fp16x2", p
        assert p["convt"] == {"up4": "slots", "up3": "slots", "up2": "slots", "up1": "fp32->slots"}, p
        assert p["layers"]["up4.c2"] == "fused+head" and p["layers"]["down3.c2"] == "fused+pool", p
        assert p["fallback_reason"].startswith("level 4: down4.c1") and p["fallback_reason"].endswith("ops.eval_layer_ok"), p
        p = got[key % (VALUE, "32x1x200x200", "None")]
        assert p["fused"] and p["depth"] == 2 and "W = 50" in p["fallback_reason"] and "ops.eval_layer_ok_ragged_fp16" in p["fallback_reason"], p
        p = got[key % (VALUE, "2x1x256x250", "None")]
        assert not p["fused"] and p["depth"] == 0 and "W = 250" in p["reason"], p
    p = got["in_chns=3,bshare=False | conv='split',fused_eval='%s' | 1x3x224x224 | None" % VALUE]
    assert p["fused"] and p["depth"] == 4 and p["convt"]["up1"] == "fp32->slots", p
    assert all(sorted(p) == ["batch", "convt", "depth", "fallback_reason", "fused", "layers", "operands", "reason"] for p in got.values())


def test_full_tile_shape_answers_as_fp16x2_pool():
    """4 x 1 x 256^2: the dictionaries of the new value == those of "fp16x2+pool", computed under that value by the same query"""
    mod = _module("make_plan_table_ragged_fp16_t2", "make_plan_table_ragged_fp16.py")
    shape = (4, 1, 256, 256)
    got = mod.table(shapes=(shape,))
    pooled = mod.table(settings=(dict(fused_eval="fp16x2+pool"), dict(conv="split", fused_eval="fp16x2+pool")), shapes=(shape,))
    assert len(got) == len(pooled) == 8
    for k, plan in got.items():
        assert plan == pooled[k.replace(VALUE, "fp16x2+pool")] and list(plan["layers"]) == list(pooled[k.replace(VALUE, "fp16x2+pool")]["layers"]), k
    assert {p["depth"] for p in got.values()} == {0, 2, 4}
