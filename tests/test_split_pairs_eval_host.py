"""Host side of the fp32-level fused eval plan's bottom level on image-pair tiles (Settings.fused_eval = "fp16x2+ragged+pairs"): the
setting's value, the layer predicate, the entry point's declaration and refusals, and the plan query against
tests/golden/fused_eval_plans_split_pairs.json (tests/golden/make_plan_table_split_pairs.py; compute units stubbed to 256).  No GPU."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import pytest

VALUE = "fp16x2+ragged+pairs"
RAGGED = "fp16x2+ragged"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRY = "onet_conv3x3_split_fwd_pre_act_pairs"
ARGS = ["xs", "xs_bs", "x_amax", "scale_always", "x_amax2", "split_ch", "wq", "save", "aP", "aP_bs", "aP_slots", "a_amax", "a", "a_bs",
        "B", "Cin", "Cout", "H", "W", "stream"]
# (fused_eval, operands, pool, ragged, anymap, pairs, upmap) of every value that existed before this one
BEFORE = {None: (False, None, False, False, False, False, False), False: (False, None, False, False, False, False, False),
          True: (True, "fp16x2", False, False, False, False, False), "bf16": (True, "bf16", False, False, False, False, False),
          "fp16x2+pool": (True, "fp16x2", True, False, False, False, False), "bf16+pool": (True, "bf16", True, False, False, False, False),
          "bf16+pool+ragged": (True, "bf16", True, True, False, False, False), "fp16x2+ragged": (True, "fp16x2", True, True, False, False, False),
          "bf16+pool+anymap": (True, "bf16", True, True, True, False, False),
          "bf16+pool+anymap+pairs": (True, "bf16", True, True, True, True, False),
          "bf16+pool+anymap+pairs+up": (True, "bf16", True, True, True, True, True)}


def _module(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _answers(ops):
    return (ops.fused_eval(), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged(), ops.fused_eval_anymap(),
            ops.fused_eval_pairs(), ops.fused_eval_upmap())


def test_value_is_accepted_and_the_other_values_answer_as_before():
    import onet_amd
    from onet_amd import ops
    with ops.using(ops.Settings(fused_eval=VALUE)):
        assert _answers(ops) == (True, "fp16x2", True, True, False, False, False)
        assert ops.fused_eval_pairs_fp16() is True
    assert sorted(ops._FUSED_EVAL_VALUES) == sorted([v for v in BEFORE if isinstance(v, str)] + [VALUE])
    for v, want in BEFORE.items():
        with ops.using(ops.Settings(fused_eval=v)):
            assert _answers(ops) == want, v
            assert ops.fused_eval_pairs_fp16() is False, v
    assert ops._FUSED_EVAL_VALUES[RAGGED] == ops._FusedEval("fp16x2", True, frozenset(("full", "ragged")), False)
    s = ops.Settings(conv="split", fused_eval=VALUE)
    assert s.replace(twin=False).fused_eval == VALUE and f"fused_eval={VALUE!r}" in repr(s)
    m = onet_amd.Onet(in_chns=1, binit=True, bshare=True).eval()
    for bad in ("fp16x2+ragged+pair", "fp16x2+pairs", "fp16x2+pool+pairs", "fp16x2+ragged+pairs+", "bf16+ragged+pairs", "FP16X2+RAGGED+PAIRS"):
        with ops.using(ops.Settings(fused_eval=bad)):
            with pytest.raises(ValueError, match="fused_eval"):
                ops.fused_eval_pairs_fp16()
        m.settings = ops.Settings(fused_eval=bad)
        with pytest.raises(ValueError, match="fused_eval"):
            onet_amd.fused_eval_plan(m, (2, 1, 256, 256))


def test_onet_flags_reach_the_value():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from onet_amd import ops; "
            "print(repr(ops.FUSED_EVAL), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged(), ops.fused_eval_anymap(), "
            "ops.fused_eval_pairs(), ops.fused_eval_upmap(), ops.fused_eval_pairs_fp16())" % root)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ONET_FLAGS="FUSED_EVAL=" + VALUE), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == f"{VALUE!r} fp16x2 True True False False False True", out.stdout


def test_layer_predicate():
    """eval_layer_ok_pairs_fp16: the entry's domain on PAIRS_MIN_W <= W <= 16, every such layer under "split", the fill rule on pair tiles
    under "auto", eval_layer_ok_ragged_fp16's answer on every W > 16; the older predicates answer as before"""
    from onet_amd import ops
    real = ops.n_cu
    ops.n_cu = lambda device=None: 256
    try:
        assert ops.PAIRS_MIN_W == 9
        ok = ops.eval_layer_ok_pairs_fp16
        with ops.using(ops.Settings(conv="split", fused_eval=VALUE)):
            for H, W in ((16, 16), (14, 14), (12, 12), (3, 12), (2, 16), (8, 9), (5, 14), (20, 12), (12, 13)):
                assert ok(1, 64, 64, H, W) and ok(3, 512, 1024, H, W) and ok(1, 16, 64, H, W) and ok(2, 48, 128, H, W), (H, W)
                assert not ops.eval_layer_ok_ragged_fp16(1, 64, 64, H, W) and not ops.eval_layer_ok(1, 64, 64, H, W), (H, W)
            for H, W in ((8, 8), (16, 8), (6, 6), (4, 4), (12, 1), (12, 0), (0, 12)):
                assert not ok(2, 64, 64, H, W), (H, W)
            assert not ok(2, 24, 64, 14, 14) and not ok(2, 64, 96, 14, 14) and not ok(2, 8, 64, 14, 14) and not ok(0, 64, 64, 14, 14)
        # no pre-split storage / one-part operands / the fp16 split path switched off
        for st in (ops.Settings(conv="split", presplit=False, fused_eval=VALUE), ops.Settings(conv="bf16", fused_eval=VALUE),
                   ops.Settings(conv="direct", fused_eval=VALUE), ops.Settings(conv="split", split_f16=False, fused_eval=VALUE)):
            with ops.using(st):
                assert not ok(64, 64, 64, 14, 14) and not ok(64, 512, 1024, 16, 16), st
        # W > 16: the ragged fp16 predicate's answer, whatever it is
        for conv in ("auto", "bf16", "split", "direct"):
            with ops.using(ops.Settings(conv=conv, fused_eval=VALUE)):
                for B in (1, 4, 64):
                    for Cin, Cout in ((64, 64), (48, 64), (128, 96), (512, 1024)):
                        for H, W in ((16, 32), (32, 32), (25, 25), (12, 25), (28, 28), (12, 20), (13, 17), (14, 18), (50, 50), (256, 256), (16, 19)):
                            assert ok(B, Cin, Cout, H, W) == ops.eval_layer_ok_ragged_fp16(B, Cin, Cout, H, W), (conv, B, Cin, Cout, H, W)
        with ops.using(ops.Settings(fused_eval=VALUE)):
            # "auto": cdiv(B, 2) cdiv(H, 16) Cout / 64 >= 192 -- down4 (Cout = 1024: 16 channel tiles): 12 pairs; B = 23 is 12 pairs, 22 is 11
            assert ok(24, 512, 1024, 14, 14) and ok(23, 1024, 1024, 14, 14) and not ok(22, 1024, 1024, 14, 14)
            assert ok(11, 512, 1024, 20, 12) and not ok(10, 512, 1024, 20, 12) and ok(12, 512, 1024, 17, 16)        # two row tiles: 6 pairs
            assert not ok(64, 64, 64, 16, 16) and ok(383, 64, 64, 16, 16) and not ok(382, 64, 64, 16, 16)           # one channel tile: 192 pairs
        floor = ops.PAIRS_MIN_W
        try:
            ops.PAIRS_MIN_W = 15                # the tools' switch: the 14-pixel level of a 224 x 224 input is left to the fall-back
            with ops.using(ops.Settings(conv="split", fused_eval=VALUE)):
                assert not ok(2, 64, 64, 14, 14) and ok(2, 64, 64, 16, 16) and ok(2, 64, 64, 14, 15)
        finally:
            ops.PAIRS_MIN_W = floor
    finally:
        ops.n_cu = real


def test_entry_point_declared_bound_and_the_old_headers_unchanged():
    from onet_amd import _lib, build
    protos = _lib.parse_header(_lib.SPLIT_PAIRS_HEADER)
    assert sorted(protos) == [ENTRY]
    lib, raw = _lib.load(), ctypes.CDLL(_lib.LIBPATH)
    assert protos[ENTRY][2] == ARGS and protos[ENTRY][0] is ctypes.c_int
    assert hasattr(raw, ENTRY) and len(getattr(lib, ENTRY).argtypes) == len(ARGS)
    # the argument list of the ragged entry
    ragged_split = _lib.parse_header(_lib.RAGGED_SPLIT_HEADER)
    assert protos[ENTRY][1:] == ragged_split["onet_conv3x3_split_fwd_pre_act_ragged"][1:]
    old = [_lib.parse_header(h) for h in (_lib.HEADER, _lib.EVAL_HEADER, _lib.RAGGED_HEADER, _lib.RAGGED_SPLIT_HEADER, _lib.ANYMAP_HEADER,
                                          _lib.PAIRS_HEADER, _lib.UPMAP_HEADER)]
    assert tuple(len(p) for p in old) == (108, 2, 5, 5, 2, 1, 1)
    assert all(ENTRY not in p for p in old)
    assert lib.onet_abi_version() == 4
    # the header is a dependency of the build
    lib_t, st = os.path.getmtime(build.LIB), os.stat(_lib.SPLIT_PAIRS_HEADER)
    try:
        os.utime(_lib.SPLIT_PAIRS_HEADER, (lib_t + 10, lib_t + 10))
        assert build._stale()
    finally:
        os.utime(_lib.SPLIT_PAIRS_HEADER, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert not build._stale()


def test_entry_refuses_and_rejects_before_a_launch():
    """outside the domain: 1, nothing dereferenced (16: a non-null, 16-byte aligned address nothing may read); bad arguments inside
    it: an error code, still without a launch"""
    from onet_amd import _lib
    lib = _lib.load()
    H, W, Cin, Cout = 14, 14, 32, 64
    n_in, n_out = Cin * H * W, Cout * H * W
    base = dict(xs=16, xs_bs=n_in, x_amax=None, scale_always=0, x_amax2=None, split_ch=0, wq=16, save=16, aP=16, aP_bs=n_out, aP_slots=16,
                a_amax=None, a=None, a_bs=0, B=2, Cin=Cin, Cout=Cout, H=H, W=W, stream=None)

    def f(**kw):
        return getattr(lib, ENTRY)(*[dict(base, **kw)[k] for k in ARGS])
    assert f(W=17) == 1 and f(W=32, H=16) == 1 and f(Cin=24, xs_bs=24 * H * W) == 1 and f(Cout=96) == 1
    assert f(W=17, a_amax=16) == 1 and f(W=20, H=12) == 1
    # a pair beyond the buffer-resource range: the batch stride (4-byte units) plus one image must stay below 2 GiB
    assert f(xs_bs=1 << 29) == 1 and f(xs_bs=(1 << 29) - 4) == 1 and f(B=1, xs_bs=1 << 29) == 1
    assert f(xs=None) == -1 and b"null" in lib.onet_last_error()
    assert f(save=None) == -1 and b"null" in lib.onet_last_error()
    assert f(aP_slots=None) == -1 and b"null" in lib.onet_last_error()
    assert f(B=0) == -1 and b"bad shape" in lib.onet_last_error()
    assert f(H=0) == -1 and b"bad shape" in lib.onet_last_error()
    assert f(W=0) == -1 and b"bad shape" in lib.onet_last_error()
    assert f(split_ch=16) == -1 and b"split_ch" in lib.onet_last_error()
    assert f(xs=8) == -1 and b"aligned" in lib.onet_last_error()
    assert f(aP=24) == -1 and b"aligned" in lib.onet_last_error()
    assert f(a=18, a_bs=n_out) == -1 and b"aligned" in lib.onet_last_error()
    assert f(xs_bs=n_in - 4) == -1 and b"stride" in lib.onet_last_error()
    assert f(aP_bs=n_out - 4) == -1 and b"stride" in lib.onet_last_error()
    assert f(a=16, a_bs=n_out - 1) == -1 and b"stride" in lib.onet_last_error()


def test_plan_table_is_the_recorded_one_and_equal_on_rerun():
    mod = _module("make_plan_table_split_pairs_t", "make_plan_table_split_pairs.py")
    got = mod.table()
    with open(mod.PATH) as f:
        assert got == json.load(f)
    assert got == mod.table()
    assert len(got) == 2 * 2 * len(mod.SHAPES) * 2
    full = {"up4": "slots", "up3": "slots", "up2": "slots", "up1": "slots"}
    cases = [("in_chns=1,bshare=True", "conv='split',", "32x1x224x224"), ("in_chns=1,bshare=True", "conv='split',", "32x1x256x256"),
             ("in_chns=3,bshare=False", "conv='split',", "16x3x224x224"),
             # under "auto" the fill rule decides: 32 images are 16 pair tiles x 16 channel tiles at level 4
             ("in_chns=1,bshare=True", "", "32x1x224x224"), ("in_chns=1,bshare=True", "", "32x1x256x256")]
    for model, conv, shape in cases:
        for head in ("None", "fused"):
            p = got["%s | %sfused_eval='%s' | %s | %s" % (model, conv, VALUE, shape, head)]
            assert p["fused"] and p["depth"] == 5 and p["fallback_reason"] is None and p["operands"] == "fp16x2", p
            assert "fallback" not in p["layers"].values() and "fallback" not in p["convt"].values(), p
            assert p["layers"]["down4.c1"] == p["layers"]["down4.c2"] == "fused" and p["layers"]["down3.c2"] == "fused+pool", p
            assert p["convt"] == full, p
            assert p["layers"]["up4.c2"] == ("fused+head" if head == "fused" else "plain+head"), p
    # ... 16 images are 8 x 16 < 192: level 4 stays a fall-back level, by the pair predicate's name
    p = got["in_chns=3,bshare=False | fused_eval='%s' | 16x3x224x224 | None" % VALUE]
    assert p["fused"] and p["depth"] == 4 and p["convt"]["up1"] == "fp32->slots", p
    assert p["fallback_reason"].startswith("level 4: down4.c1") and "14 x 14" in p["fallback_reason"] and "eval_layer_ok_pairs_fp16" in p["fallback_reason"], p
    assert all(sorted(p) == ["batch", "convt", "depth", "fallback_reason", "fused", "layers", "operands", "reason"] for p in got.values())


def test_other_inputs_answer_as_the_ragged_value():
    """200 x 200 (odd below level 2: the fp16 plan has no any-map levels), 2 x 1 x 64 x 64 (level 4 is 4 x 4, below the floor), 512 x 512
    (level 4 is 32 x 32) and 96 x 96 (level 3 is 12 x 12, a level the value does not add): the dictionaries of the new value == those
    of "fp16x2+ragged"; and that value still stops at depth 4 at 224 x 224 and 256 x 256, naming down4.c1"""
    mod = _module("make_plan_table_split_pairs_t2", "make_plan_table_split_pairs.py")
    shapes = ((32, 1, 200, 200), (2, 1, 64, 64), (1, 3, 512, 512), (4, 1, 96, 96), (2, 1, 256, 250))
    got = mod.table(shapes=shapes)
    with open(mod.PATH) as f:
        recorded = json.load(f)
    old = mod.table(settings=(dict(fused_eval=RAGGED), dict(conv="split", fused_eval=RAGGED)), shapes=shapes + mod.SHAPES[:2])
    assert len(got) == 2 * 2 * len(shapes) * 2
    hit = 0
    for k, plan in got.items():
        k_old = k.replace(VALUE, RAGGED)
        assert plan == old[k_old] and list(plan["layers"]) == list(old[k_old]["layers"]), k
        if k in recorded:
            hit += 1
            assert plan == recorded[k], k
    assert hit == 2 * 2 * 1 * 2
    assert got["in_chns=1,bshare=True | conv='split',fused_eval='%s' | 32x1x200x200 | None" % VALUE]["depth"] == 2
    assert got["in_chns=1,bshare=True | conv='split',fused_eval='%s' | 2x1x64x64 | None" % VALUE]["depth"] == 2        # (its 16-pixel level is level 2)
    assert got["in_chns=3,bshare=False | conv='split',fused_eval='%s' | 1x3x512x512 | None" % VALUE]["depth"] == 5
    with open(os.path.join(GOLDEN, "fused_eval_plans_ragged_fp16.json")) as f:
        ragged_table = json.load(f)
    k = "in_chns=1,bshare=True | conv='split',fused_eval='%s' | 32x1x200x200 | None"
    assert got[k % VALUE] == ragged_table[k % RAGGED]
    for shape, px in (("32x1x224x224", "14 x 14"), ("32x1x256x256", "16 x 16")):
        p = old["in_chns=1,bshare=True | conv='split',fused_eval='%s' | %s | None" % (RAGGED, shape)]
        assert p["fused"] and p["depth"] == 4 and p["fallback_reason"].startswith("level 4: down4.c1") and px in p["fallback_reason"], p
