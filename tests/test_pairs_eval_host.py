"""Host side of the fused eval plan's bottom level on image-pair tiles (Settings.fused_eval = "bf16+pool+anymap+pairs"): the setting's
value, the layer predicate, the entry point's declaration and refusals, and the plan query against
tests/golden/fused_eval_plans_pairs.json (tests/golden/make_plan_table_pairs.py; compute units stubbed to 256).  No GPU."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import pytest

VALUE = "bf16+pool+anymap+pairs"
ANYMAP = "bf16+pool+anymap"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRY = "onet_conv3x3_plain16_fwd_pre_act_pairs"
ARGS = ["xs", "xs_bs", "wq", "save", "aP", "aP_bs", "a_amax", "a", "a_bs", "B", "Cin", "Cout", "H", "W", "stream"]


def _module(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_value_is_accepted_and_the_other_values_answer_as_before():
    import onet_amd
    from onet_amd import ops
    with ops.using(ops.Settings(fused_eval=VALUE)):
        assert (ops.fused_eval(), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged(), ops.fused_eval_anymap(),
                ops.fused_eval_pairs()) == (True, "bf16", True, True, True, True)
    for v in (None, False, True, "bf16", "fp16x2+pool", "bf16+pool", "bf16+pool+ragged", "fp16x2+ragged", ANYMAP):
        with ops.using(ops.Settings(fused_eval=v)):
            assert ops.fused_eval_pairs() is False, v
    with ops.using(ops.Settings(fused_eval=ANYMAP)):
        assert ops.fused_eval_anymap() is True
    s = ops.Settings(conv="bf16", fused_eval=VALUE)
    assert s.replace(twin=False).fused_eval == VALUE and f"fused_eval={VALUE!r}" in repr(s)
    m = onet_amd.Onet(in_chns=1, binit=True, bshare=True).eval()
    for bad in ("bf16+pool+anymap+pair", "bf16+pool+pairs", "bf16+pool+ragged+pairs", "fp16x2+pairs", "bf16+pool+anymap+pairs+", "bf16+pairs"):
        with ops.using(ops.Settings(fused_eval=bad)):
            with pytest.raises(ValueError, match="fused_eval"):
                ops.fused_eval_pairs()
        m.settings = ops.Settings(fused_eval=bad)
        with pytest.raises(ValueError, match="fused_eval"):
            onet_amd.fused_eval_plan(m, (2, 1, 256, 256))


def test_onet_flags_reach_the_value():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from onet_amd import ops; "
            "print(repr(ops.FUSED_EVAL), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged(), ops.fused_eval_anymap(), "
            "ops.fused_eval_pairs(), ops.PAIRS_MIN_W)" % root)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ONET_FLAGS="FUSED_EVAL=" + VALUE + ",PAIRS_MIN_W=13"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == f"{VALUE!r} bf16 True True True True 13", out.stdout


def test_layer_predicate():
    """eval_layer_ok_pairs: the entry's domain on PAIRS_MIN_W <= W <= 16, the fill rule on pair tiles under "auto", eval_layer_ok_anymap's
    answer on every W > 16; the older predicates answer as before"""
    from onet_amd import ops
    real = ops.n_cu
    ops.n_cu = lambda device=None: 256
    try:
        assert ops.PAIRS_MIN_W == 9
        with ops.using(ops.Settings(conv="bf16", fused_eval=VALUE)):
            ok = ops.eval_layer_ok_pairs
            for H, W in ((16, 16), (14, 14), (12, 12), (3, 12), (2, 16), (8, 9)):
                assert ok(1, 64, 64, H, W) and ok(3, 512, 1024, H, W), (H, W)
                assert not ops.eval_layer_ok_anymap(1, 64, 64, H, W) and not ops.eval_layer_ok_ragged(1, 64, 64, H, W), (H, W)
            for H, W in ((8, 8), (16, 8), (6, 6), (4, 4), (12, 1), (12, 0), (0, 12)):
                assert not ok(2, 64, 64, H, W), (H, W)
            assert not ok(2, 48, 64, 14, 14) and not ok(2, 64, 96, 14, 14) and not ok(2, 16, 64, 14, 14) and not ok(0, 64, 64, 14, 14)
        with ops.using(ops.Settings(conv="bf16", presplit=False, fused_eval=VALUE)):
            assert not ops.eval_layer_ok_pairs(4, 64, 64, 14, 14)
        # W > 16: the any-map predicate's answer, whatever it is
        for conv in ("auto", "bf16", "split", "direct"):
            with ops.using(ops.Settings(conv=conv, fused_eval=VALUE)):
                for B in (1, 4, 64):
                    for Cin, Cout in ((64, 64), (48, 64), (128, 96), (512, 1024)):
                        for H, W in ((16, 32), (32, 32), (25, 25), (12, 25), (28, 28), (12, 20), (13, 17), (14, 18), (50, 50), (256, 256), (16, 19)):
                            assert ops.eval_layer_ok_pairs(B, Cin, Cout, H, W) == ops.eval_layer_ok_anymap(B, Cin, Cout, H, W), (conv, B, Cin, Cout, H, W)
        with ops.using(ops.Settings(fused_eval=VALUE)):
            # "auto": cdiv(B, 2) cdiv(H, 16) Cout / 64 >= 192 -- down4 (Cout = 1024: 16 channel tiles): 12 pairs; B = 23 is 12 pairs, 22 is 11
            ok = ops.eval_layer_ok_pairs
            assert ok(24, 512, 1024, 14, 14) and ok(23, 1024, 1024, 14, 14) and not ok(22, 1024, 1024, 14, 14)
            assert ok(11, 512, 1024, 20, 12) and not ok(10, 512, 1024, 20, 12) and ok(12, 512, 1024, 17, 16)        # two row tiles: 6 pairs
            assert not ok(64, 64, 64, 16, 16) and ok(383, 64, 64, 16, 16) and not ok(382, 64, 64, 16, 16)           # one channel tile: 192 pairs
        floor = ops.PAIRS_MIN_W
        try:
            ops.PAIRS_MIN_W = 13                # the tools' switch: the 12-pixel level of a 200 x 200 input is left to the fall-back
            with ops.using(ops.Settings(conv="bf16", fused_eval=VALUE)):
                assert not ops.eval_layer_ok_pairs(2, 64, 64, 12, 12) and ops.eval_layer_ok_pairs(2, 64, 64, 14, 14)
                assert ops.eval_layer_ok_pairs(2, 64, 64, 12, 13) and ops.eval_layer_ok_pairs(2, 64, 64, 25, 25)
            ops.PAIRS_MIN_W = 5
            with ops.using(ops.Settings(conv="bf16", fused_eval=VALUE)):
                assert ops.eval_layer_ok_pairs(2, 64, 64, 6, 6) and not ops.eval_layer_ok_pairs(2, 64, 64, 4, 4)
        finally:
            ops.PAIRS_MIN_W = floor
    finally:
        ops.n_cu = real


def test_entry_point_declared_bound_and_the_old_headers_unchanged():
    from onet_amd import _lib, build
    protos = _lib.parse_header(_lib.PAIRS_HEADER)
    assert sorted(protos) == [ENTRY]
    lib, raw = _lib.load(), ctypes.CDLL(_lib.LIBPATH)
    assert protos[ENTRY][2] == ARGS and protos[ENTRY][0] is ctypes.c_int
    assert hasattr(raw, ENTRY) and len(getattr(lib, ENTRY).argtypes) == len(ARGS)
    # the argument list of the any-map entry
    anymap = _lib.parse_header(_lib.ANYMAP_HEADER)
    assert protos[ENTRY][1:] == anymap["onet_conv3x3_plain16_fwd_pre_act_anymap"][1:]
    main, ragged = _lib.parse_header(), _lib.parse_header(_lib.RAGGED_HEADER)
    assert (len(main), len(_lib.parse_header(_lib.EVAL_HEADER)), len(ragged), len(_lib.parse_header(_lib.RAGGED_SPLIT_HEADER)), len(anymap)) == \
        (108, 2, 5, 5, 2)
    assert ENTRY not in set(main) | set(ragged) | set(anymap)
    assert lib.onet_abi_version() == 4
    # the header is a dependency of the build
    lib_t, st = os.path.getmtime(build.LIB), os.stat(_lib.PAIRS_HEADER)
    try:
        os.utime(_lib.PAIRS_HEADER, (lib_t + 10, lib_t + 10))
        assert build._stale()
    finally:
        os.utime(_lib.PAIRS_HEADER, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert not build._stale()


def test_entry_refuses_and_rejects_before_a_launch():
    """outside the domain: 1, nothing dereferenced (16: a non-null, 16-byte aligned address nothing may read); bad arguments inside
    it: an error code, still without a launch"""
    from onet_amd import _lib
    lib = _lib.load()
    H, W, Cin, Cout = 14, 14, 32, 64
    n_in, n_out = Cin * H * W // 2, Cout * H * W // 2
    base = dict(xs=16, xs_bs=n_in, wq=16, save=16, aP=16, aP_bs=n_out, a_amax=None, a=None, a_bs=0, B=2, Cin=Cin, Cout=Cout, H=H, W=W, stream=None)

    def f(**kw):
        return getattr(lib, ENTRY)(*[dict(base, **kw)[k] for k in ARGS])
    assert f(W=17) == 1 and f(W=32, H=16) == 1 and f(Cin=48, xs_bs=48 * H * W // 2) == 1 and f(Cout=96) == 1 and f(a_amax=16) == 1
    assert f(a_amax=16, H=16, W=16) == 1
    # a pair beyond the buffer-resource range: the batch stride (4-byte units) plus one image must stay below 2 GiB
    assert f(xs_bs=1 << 29) == 1 and f(xs_bs=(1 << 29) - 4) == 1 and f(B=1, xs_bs=1 << 29) == 1
    assert f(xs=None) == -1 and b"null" in lib.onet_last_error()
    assert f(save=None) == -1 and b"null" in lib.onet_last_error()
    assert f(B=0) == -1 and b"bad shape" in lib.onet_last_error()
    assert f(H=0) == -1 and b"bad shape" in lib.onet_last_error()
    assert f(W=0) == -1 and b"bad shape" in lib.onet_last_error()
    assert f(xs=8) == -1 and b"aligned" in lib.onet_last_error()
    assert f(aP=24) == -1 and b"aligned" in lib.onet_last_error()
    assert f(a=18, a_bs=Cout * H * W) == -1 and b"aligned" in lib.onet_last_error()
    assert f(xs_bs=n_in - 4) == -1 and b"stride" in lib.onet_last_error()
    assert f(aP_bs=n_out - 4) == -1 and b"stride" in lib.onet_last_error()
    assert f(a=16, a_bs=Cout * H * W - 1) == -1 and b"stride" in lib.onet_last_error()


def test_plan_table_is_the_recorded_one_and_equal_on_rerun():
    mod = _module("make_plan_table_pairs_t", "make_plan_table_pairs.py")
    got = mod.table()
    with open(mod.PATH) as f:
        assert got == json.load(f)
    assert got == mod.table()
    assert len(got) == 2 * 2 * len(mod.SHAPES) * 2
    key = "in_chns=1,bshare=True | conv='bf16',fused_eval='%s' | %s | %s" % (VALUE, "%s", "%s")
    convt = {"32x1x200x200": {"up4": "slots", "up3": "slots", "up2": "fp32->slots", "up1": "fp32->slots"},      # 25 <- 12: padded, by `pack`
             "1x1x224x224": {"up4": "slots", "up3": "slots", "up2": "slots", "up1": "slots"},                   # 14 x 14: the ragged slot GEMM
             "4x1x256x256": {"up4": "slots", "up3": "slots", "up2": "slots", "up1": "slots"}}
    for shape, edges in convt.items():
        for head in ("None", "fused"):
            p = got[key % (shape, head)]
            assert p["fused"] and p["depth"] == 5 and p["fallback_reason"] is None and p["operands"] == "bf16", p
            assert "fallback" not in p["layers"].values() and "fallback" not in p["convt"].values(), p
            assert p["layers"]["down4.c1"] == p["layers"]["down4.c2"] == "fused" and p["layers"]["down3.c2"] == "fused+pool", p
            assert p["convt"] == edges, p
            assert p["layers"]["up4.c2"] == ("fused+head" if head == "fused" else "plain+head"), p
    # under "auto" the fill rule decides: a twin batch of 64 is 32 pair tiles x 16 channel tiles at level 4; 8 images are 4 x 16 < 192
    p = got["in_chns=1,bshare=True | fused_eval='%s' | 32x1x200x200 | None" % VALUE]
    assert p["fused"] and p["depth"] == 5 and p["fallback_reason"] is None, p
    assert got["in_chns=1,bshare=True | fused_eval='%s' | 4x1x256x256 | None" % VALUE]["depth"] < 5
    assert all(sorted(p) == ["batch", "convt", "depth", "fallback_reason", "fused", "layers", "operands", "reason"] for p in got.values())


def test_other_bottom_levels_answer_as_the_anymap_value():
    """512 x 512 (level 4: 32 x 32) and 96 x 96 (level 3: 12 x 12, a level the value does not add): the dictionaries of the new value ==
    those of "bf16+pool+anymap"; and that value still stops at depth 4 on the three resolutions, naming down4.c1"""
    mod = _module("make_plan_table_pairs_t2", "make_plan_table_pairs.py")
    shapes = ((1, 3, 512, 512), (4, 1, 96, 96), (2, 1, 64, 64), (2, 1, 128, 128))
    got = mod.table(shapes=shapes)
    with open(mod.PATH) as f:
        recorded = json.load(f)
    old = mod.table(settings=(dict(fused_eval=ANYMAP), dict(conv="bf16", fused_eval=ANYMAP)), shapes=shapes + mod.SHAPES[:3])
    assert len(got) == 2 * 2 * len(shapes) * 2
    hit = 0
    for k, plan in got.items():
        k_old = k.replace(VALUE, ANYMAP)
        assert plan == old[k_old] and list(plan["layers"]) == list(old[k_old]["layers"]), k
        if k in recorded:
            hit += 1
            assert plan == recorded[k], k
    assert hit == 2 * 2 * 2 * 2
    assert got["in_chns=3,bshare=False | conv='bf16',fused_eval='%s' | 1x3x512x512 | None" % VALUE]["depth"] == 5
    assert got["in_chns=1,bshare=True | conv='bf16',fused_eval='%s' | 4x1x96x96 | None" % VALUE]["depth"] == 3
    for shape, px in (("32x1x200x200", "12 x 12"), ("1x1x224x224", "14 x 14"), ("4x1x256x256", "16 x 16")):
        p = old["in_chns=1,bshare=True | conv='bf16',fused_eval='%s' | %s | None" % (ANYMAP, shape)]
        assert p["fused"] and p["depth"] == 4 and p["fallback_reason"].startswith("level 4: down4.c1") and px in p["fallback_reason"], p
