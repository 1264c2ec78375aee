"""Host side of the fused eval plan's slot-operand ConvTranspose2d on maps of any size (Settings.fused_eval = "bf16+pool+anymap+pairs+up"):
the setting's value, the edge predicate, the entry point's declaration and refusals, and the plan query against
tests/golden/fused_eval_plans_upmap.json (tests/golden/make_plan_table_upmap.py; compute units stubbed to 256).  No GPU."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import pytest

VALUE = "bf16+pool+anymap+pairs+up"
PAIRS = "bf16+pool+anymap+pairs"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRY = "onet_convT2x2_fwd_slots_anymap"
ARGS = ["xP", "xP_bs", "wP", "bias", "yP", "yP_bs", "B", "Cin", "Ct", "h", "w", "Ho", "Wo", "stream"]
# (fused_eval, operands, pool, ragged, anymap, pairs, upmap) of every older value
OLDER = {None: (False, None, False, False, False, False, False), False: (False, None, False, False, False, False, False),
         True: (True, "fp16x2", False, False, False, False, False), "bf16": (True, "bf16", False, False, False, False, False),
         "fp16x2+pool": (True, "fp16x2", True, False, False, False, False), "bf16+pool": (True, "bf16", True, False, False, False, False),
         "bf16+pool+ragged": (True, "bf16", True, True, False, False, False), "fp16x2+ragged": (True, "fp16x2", True, True, False, False, False),
         "bf16+pool+anymap": (True, "bf16", True, True, True, False, False), PAIRS: (True, "bf16", True, True, True, True, False)}


def _module(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _queries(ops):
    return (ops.fused_eval(), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged(), ops.fused_eval_anymap(),
            ops.fused_eval_pairs(), ops.fused_eval_upmap())


def test_value_is_accepted_and_the_other_values_answer_as_before():
    import onet_amd
    from onet_amd import ops
    with ops.using(ops.Settings(fused_eval=VALUE)):
        assert _queries(ops) == (True, "bf16", True, True, True, True, True)
    for v, want in OLDER.items():
        with ops.using(ops.Settings(fused_eval=v)):
            assert _queries(ops) == want, v
    s = ops.Settings(conv="bf16", fused_eval=VALUE)
    assert s.replace(twin=False).fused_eval == VALUE and f"fused_eval={VALUE!r}" in repr(s)
    m = onet_amd.Onet(in_chns=1, binit=True, bshare=True).eval()
    for bad in ("bf16+pool+anymap+pairs+u", "bf16+pool+anymap+up", "bf16+pool+up", "fp16x2+up", "bf16+pool+anymap+pairs+up+", "bf16+up"):
        with ops.using(ops.Settings(fused_eval=bad)):
            with pytest.raises(ValueError, match="fused_eval"):
                ops.fused_eval_upmap()
        m.settings = ops.Settings(fused_eval=bad)
        with pytest.raises(ValueError, match="fused_eval"):
            onet_amd.fused_eval_plan(m, (2, 1, 200, 200))


def test_onet_flags_reach_the_value():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from onet_amd import ops; "
            "print(repr(ops.FUSED_EVAL), ops.fused_eval_operands(), ops.fused_eval_pool(), ops.fused_eval_ragged(), ops.fused_eval_anymap(), "
            "ops.fused_eval_pairs(), ops.fused_eval_upmap())" % root)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ONET_FLAGS="FUSED_EVAL=" + VALUE), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == f"{VALUE!r} bf16 True True True True True", out.stdout


def test_edge_predicate_on_its_domain_table():
    """convt_slots_ok_anymap: any w, Ho - 2h and Wo - 2w in {0, 1}, the channel conditions of the slot GEMM; off without pre-split storage"""
    from onet_amd import ops
    with ops.using(ops.Settings(conv="bf16", fused_eval=VALUE)):
        ok = ops.convt_slots_ok_anymap
        for h, w in ((6, 5), (6, 25), (12, 12), (3, 12), (5, 7), (14, 14), (1, 1), (25, 25), (8, 16)):        # odd and even w
            for ph in (0, 1):
                for pw in (0, 1):                                                                          # the four pad combinations
                    assert ok(2, 128, 64, h, w, 2 * h + ph, 2 * w + pw), (h, w, ph, pw)
                    assert ok(1, 1024, 512, h, w, 2 * h + ph, 2 * w + pw) and ok(3, 256, 128, h, w, 2 * h + ph, 2 * w + pw)
            assert not ok(2, 128, 64, h, w, 2 * h + 2, 2 * w) and not ok(2, 128, 64, h, w, 2 * h, 2 * w + 2), (h, w)
            assert not ok(2, 128, 64, h, w, 2 * h - 1, 2 * w) and not ok(2, 128, 64, h, w, 2 * h, 2 * w - 1), (h, w)
            assert not ok(2, 128, 64, h, w, h, w), (h, w)
        assert not ok(2, 144, 64, 6, 5, 12, 10) and not ok(2, 96, 64, 6, 5, 12, 10) and not ok(2, 64, 64, 6, 5, 12, 10)       # Cin % 32, Cin < 128
        assert not ok(2, 128, 48, 6, 5, 12, 10) and not ok(2, 128, 16, 6, 5, 12, 10)                                          # Ct % 32
        assert not ok(2, 128, 64, 0, 5, 0, 10) and not ok(2, 128, 64, 6, 0, 12, 0)
        assert not ok(1, 1024, 512, 1024, 1025, 2048, 2050)                       # Cin h w beyond the 2 GiB buffer-resource range
        # wherever the ragged predicate says yes, so does this one on the dense output
        for Cin, Ct in ((128, 64), (144, 64), (96, 64), (128, 48), (512, 256)):
            for h, w in ((6, 6), (12, 20), (14, 14), (8, 16)):
                assert ok(2, Cin, Ct, h, w, 2 * h, 2 * w) == ops.convt_slots_ok_ragged(2, Cin, Ct, h, w), (Cin, Ct, h, w)
    with ops.using(ops.Settings(conv="bf16", presplit=False, fused_eval=VALUE)):
        assert not ops.convt_slots_ok_anymap(2, 128, 64, 6, 5, 12, 10)


def test_entry_point_declared_bound_and_the_old_headers_unchanged():
    from onet_amd import _lib, build
    protos = _lib.parse_header(_lib.UPMAP_HEADER)
    assert sorted(protos) == [ENTRY]
    lib, raw = _lib.load(), ctypes.CDLL(_lib.LIBPATH)
    assert protos[ENTRY][2] == ARGS and protos[ENTRY][0] is ctypes.c_int
    assert hasattr(raw, ENTRY) and len(getattr(lib, ENTRY).argtypes) == len(ARGS)
    # the ragged entry's argument list with Ho, Wo in front of the stream
    ragged = _lib.parse_header(_lib.RAGGED_HEADER)
    r = ragged["onet_convT2x2_fwd_slots_ragged"]
    assert protos[ENTRY][2] == r[2][:-1] + ["Ho", "Wo", "stream"] and protos[ENTRY][1] == r[1][:-1] + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    main, anymap, pairs = _lib.parse_header(), _lib.parse_header(_lib.ANYMAP_HEADER), _lib.parse_header(_lib.PAIRS_HEADER)
    assert (len(main), len(_lib.parse_header(_lib.EVAL_HEADER)), len(ragged), len(_lib.parse_header(_lib.RAGGED_SPLIT_HEADER)), len(anymap),
            len(pairs)) == (108, 2, 5, 5, 2, 1)
    assert ENTRY not in set(main) | set(ragged) | set(anymap) | set(pairs)
    assert lib.onet_abi_version() == 4
    # the header is a dependency of the build
    lib_t, st = os.path.getmtime(build.LIB), os.stat(_lib.UPMAP_HEADER)
    try:
        os.utime(_lib.UPMAP_HEADER, (lib_t + 10, lib_t + 10))
        assert build._stale()
    finally:
        os.utime(_lib.UPMAP_HEADER, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert not build._stale()


def test_entry_refuses_and_rejects_before_a_launch():
    """outside the domain: 1, nothing dereferenced (16: a non-null, 16-byte aligned address nothing may read); bad arguments: an error
    code, still without a launch.  No call here lies inside the domain with good arguments: nothing is launched."""
    from onet_amd import _lib
    lib = _lib.load()
    h, w, Cin, Ct = 6, 5, 128, 64
    n_in, n_out = Cin * h * w // 2, (Ct // 8) * (2 * h + 1) * (2 * w + 1) * 4
    base = dict(xP=16, xP_bs=n_in, wP=16, bias=16, yP=16, yP_bs=n_out, B=2, Cin=Cin, Ct=Ct, h=h, w=w, Ho=2 * h + 1, Wo=2 * w + 1, stream=None)

    def f(**kw):
        return getattr(lib, ENTRY)(*[dict(base, **kw)[k] for k in ARGS])
    assert f(Ho=2 * h + 2) == 1 and f(Wo=2 * w + 2) == 1 and f(Ho=2 * h - 1) == 1 and f(Wo=2 * w - 1) == 1 and f(Ho=h, Wo=w) == 1
    assert f(Cin=144, xP_bs=144 * h * w // 2) == 1 and f(Cin=96) == 1 and f(Ct=48) == 1 and f(Ct=16) == 1
    assert f(xP=8) == 1 and f(yP=24) == 1 and f(wP=4) == 1 and f(xP_bs=n_in + 2) == 1 and f(yP_bs=n_out + 1) == 1      # alignment: not taken
    assert f(h=1 << 12, w=(1 << 12) + 1, Ho=1 << 13, Wo=(1 << 13) + 2) == 1                                             # beyond the 2 GiB range
    assert f(xP=None) == -1 and b"bad args" in lib.onet_last_error()
    assert f(wP=None) == -1 and b"bad args" in lib.onet_last_error()
    assert f(yP=None) == -1 and b"bad args" in lib.onet_last_error()
    for zero in ("B", "Cin", "Ct", "h", "w", "Ho", "Wo"):
        assert f(**{zero: 0}) == -1 and b"bad args" in lib.onet_last_error(), zero
        assert f(**{zero: -1}) == -1 and b"bad args" in lib.onet_last_error(), zero
    assert f(xP_bs=n_in - 4) == -1 and b"stride" in lib.onet_last_error()
    assert f(yP_bs=n_out - 4) == -1 and b"stride" in lib.onet_last_error()
    # the dense output's stride does not hold the padded map
    assert f(yP_bs=(Ct // 8) * (2 * h) * (2 * w) * 4) == -1 and b"stride" in lib.onet_last_error()
    assert f(Ho=2 * h, yP_bs=(Ct // 8) * (2 * h) * (2 * w) * 4) == -1 and b"stride" in lib.onet_last_error()


def test_plan_table_is_the_recorded_one_and_equal_on_rerun():
    mod = _module("make_plan_table_upmap_t", "make_plan_table_upmap.py")
    got = mod.table()
    with open(mod.PATH) as f:
        assert got == json.load(f)
    assert got == mod.table()
    assert len(got) == 2 * 2 * len(mod.SHAPES) * 2
    slots = dict.fromkeys(("up4", "up3", "up2", "up1"), "slots")
    for model, shape in (("in_chns=1,bshare=True", "32x1x200x200"), ("in_chns=1,bshare=True", "1x1x48x200"), ("in_chns=3,bshare=False", "1x3x40x200")):
        for head in ("None", "fused"):
            p = got["%s | conv='bf16',fused_eval='%s' | %s | %s" % (model, VALUE, shape, head)]
            assert p["fused"] and p["depth"] == 5 and p["fallback_reason"] is None and p["operands"] == "bf16", p
            assert p["convt"] == slots, p
            assert "fallback" not in p["layers"].values(), p
            assert p["layers"]["down4.c1"] == p["layers"]["down4.c2"] == "fused" and p["layers"]["down3.c2"] == "fused+pool", p
            assert p["layers"]["up4.c2"] == ("fused+head" if head == "fused" else "plain+head"), p
    p = got["in_chns=1,bshare=True | fused_eval='%s' | 32x1x200x200 | None" % VALUE]
    assert p["fused"] and p["depth"] == 5 and p["convt"] == slots, p
    assert all(sorted(p) == ["batch", "convt", "depth", "fallback_reason", "fused", "layers", "operands", "reason"] for p in got.values())
    # what the older value answers for the same three inputs: the two edges by `pack`
    old = mod.table(settings=(dict(conv="bf16", fused_eval=PAIRS),), shapes=mod.SHAPES[:3])
    for model, shape in (("in_chns=1,bshare=True", "32x1x200x200"), ("in_chns=1,bshare=True", "1x1x48x200"), ("in_chns=3,bshare=False", "1x3x40x200")):
        p = old["%s | conv='bf16',fused_eval='%s' | %s | None" % (model, PAIRS, shape)]
        q = got["%s | conv='bf16',fused_eval='%s' | %s | None" % (model, VALUE, shape)]
        assert p["convt"] == dict(slots, up2="fp32->slots", up1="fp32->slots") and p["depth"] == 5, p
        assert dict(p, convt=None) == dict(q, convt=None)


def test_inputs_without_such_an_edge_answer_as_the_pairs_value():
    """224 x 224, 256 x 256, 512 x 512 (and 96 x 96, 128 x 256): the dictionaries of the new value == those of "bf16+pool+anymap+pairs",
    which are the recorded ones of tests/golden/fused_eval_plans_pairs.json where that table holds the shape"""
    mod = _module("make_plan_table_upmap_t2", "make_plan_table_upmap.py")
    shapes = mod.SHAPES[3:] + ((4, 1, 96, 96), (1, 1, 128, 256))
    got = mod.table(shapes=shapes)
    old = mod.table(settings=(dict(fused_eval=PAIRS), dict(conv="bf16", fused_eval=PAIRS)), shapes=shapes)
    with open(os.path.join(GOLDEN, "fused_eval_plans_pairs.json")) as f:
        recorded = json.load(f)
    assert len(got) == len(old) == 2 * 2 * len(shapes) * 2
    hit = 0
    for k, plan in got.items():
        k_old = k.replace(VALUE, PAIRS)
        assert plan == old[k_old] and list(plan["layers"]) == list(old[k_old]["layers"]), k
        if k_old in recorded:
            hit += 1
            assert plan == recorded[k_old], k
    assert hit == 2 * 2 * 4 * 2
    assert got["in_chns=1,bshare=True | conv='bf16',fused_eval='%s' | 1x1x224x224 | None" % VALUE]["depth"] == 5


def test_keep_fp32_is_gone_from_the_plan_record():
    """_build_plan at 200 x 200 and 48 x 200: under the new value no unit keeps an fp32 copy and the two edges carry route "slots_anymap";
    under "bf16+pool+anymap+pairs" the last units of levels 4 and 3 keep one for the `pack` route"""
    import contextlib
    import torch
    import onet_amd
    from onet_amd import inference, ops
    real_n_cu, real_device = ops.n_cu, torch.cuda.device
    ops.n_cu = lambda device=None: 256
    torch.cuda.device = lambda device: contextlib.nullcontext()
    try:
        m = onet_amd.Onet(in_chns=1, bshare=True).eval()
        for shape in ((32, 1, 200, 200), (2, 1, 48, 200)):
            with ops.using(ops.Settings(conv="bf16", fused_eval=VALUE)):
                plan = inference._query(m.topu, shape, None, torch.device("cuda", 0))
            assert plan.reason is None and plan.depth == 5
            assert [lv.route for lv in plan.levels[:4]] == ["slots_ragged", "slots_ragged", "slots_anymap", "slots_anymap"], shape
            assert not any(u.keep_fp32 for lv in plan.levels for u in lv.enc + lv.dec)
            with ops.using(ops.Settings(conv="bf16", fused_eval=PAIRS)):
                plan = inference._query(m.topu, shape, None, torch.device("cuda", 0))
            assert [lv.route for lv in plan.levels[:4]] == ["slots_ragged", "slots_ragged", "pack", "pack"], shape
            assert [u.name for lv in plan.levels for u in lv.enc + lv.dec if u.keep_fp32] == ["up1.c2", "down4.c2"]
    finally:
        ops.n_cu, torch.cuda.device = real_n_cu, real_device
