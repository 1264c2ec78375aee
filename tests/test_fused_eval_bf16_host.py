"""Host side of the one-part (plain bf16) fused eval plan, Settings(fused_eval="bf16"): the setting's values, the new entry point's
declaration and argument checks, and the plan query on a model that never touches a device."""
import ctypes
import os
import subprocess
import sys


def test_setting_values_round_trip_and_select_the_operands():
    from onet_amd import ops
    slots = ("conv", "twin", "convt_bf16", "lazy_nan", "split", "bn_on_load", "split_f16", "grad_f16", "split_dgrad",
             "stem_fused", "sync_bn", "presplit", "z_bf16", "fused_eval")
    assert ops.Settings.__slots__ == slots                     # no field added: "bf16" is a VALUE of fused_eval
    assert ops.FUSED_EVAL is False
    b = ops.Settings(conv="bf16", fused_eval="bf16")
    r = b.replace(twin=False)
    assert r.fused_eval == "bf16" and r.conv == "bf16" and r.twin is False
    assert b.replace(fused_eval=True).fused_eval is True and b.fused_eval == "bf16"
    assert "fused_eval='bf16'" in repr(b) and "fused_eval='bf16'" in repr(r)
    with ops.using(b):
        assert ops.fused_eval() is True and ops.fused_eval_operands() == "bf16"
    with ops.using(ops.Settings(fused_eval="bf16")):
        assert ops.fused_eval() is True and ops.fused_eval_operands() == "bf16"
    with ops.using(ops.Settings(fused_eval=True)):
        assert ops.fused_eval() is True and ops.fused_eval_operands() == "fp16x2"
    with ops.using(ops.Settings(fused_eval=False)):
        assert ops.fused_eval() is False and ops.fused_eval_operands() is None
    with ops.using(ops.Settings()):
        assert ops.fused_eval() is False and ops.fused_eval_operands() is None


def test_onet_flags_switch_keeps_0_and_1_and_accepts_bf16():
    """ONET_FLAGS is read when onet_amd.ops is imported: a fresh process per value"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, %r); from onet_amd import ops; print(repr(ops.FUSED_EVAL), ops.fused_eval(), ops.fused_eval_operands())" % root
    for flags, want in (("FUSED_EVAL=0", "False False None"), ("FUSED_EVAL=1", "True True fp16x2"),
                        ("TWIN=0,FUSED_EVAL=bf16", "'bf16' True bf16")):
        env = dict(os.environ, ONET_FLAGS=flags)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip().splitlines()[-1] == want, (flags, out.stdout)


def test_entry_point_declared_and_exported():
    from onet_amd import _lib
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIBPATH) if os.path.exists(_lib.LIBPATH) else _lib.load()
    assert "onet_conv3x3_plain16_fwd_pre_act" in protos
    assert hasattr(lib, "onet_conv3x3_plain16_fwd_pre_act")
    restype, argtypes, names = protos["onet_conv3x3_plain16_fwd_pre_act"]
    assert len(argtypes) == 15, names
    assert names == ["xs", "xs_bs", "wq", "save", "aP", "aP_bs", "a_amax", "a", "a_bs", "B", "Cin", "Cout", "H", "W", "stream"], names
    # the neighbours keep their signatures, the ABI its version
    assert len(protos["onet_conv3x3_split_fwd_pre_act"][1]) == 20
    assert len(protos["onet_conv3x3_act_bound"][1]) == 9
    assert _lib.load().onet_abi_version() == 4


def test_bad_arguments_return_error_codes_without_a_device():
    from onet_amd import _lib
    lib = _lib.load()
    f = lib.onet_conv3x3_plain16_fwd_pre_act
    # (16: a non-null, 16-byte aligned address nothing may dereference)
    rc = f(None, 0, None, None, None, 0, None, None, 0, 1, 32, 64, 16, 32, None)
    assert rc == -1 and b"null" in lib.onet_last_error()
    for missing in range(4):                                   # each of xs, wq, save, aP on its own
        p = [16, 16, 16, 16]
        p[missing] = None
        rc = f(p[0], 32 * 16 * 32 // 2, p[1], p[2], p[3], 64 * 16 * 32 // 2, None, None, 0, 1, 32, 64, 16, 32, None)
        assert rc == -1 and b"null" in lib.onet_last_error(), missing
    rc = f(16, 0, 16, 16, 16, 0, None, None, 0, 0, 32, 64, 16, 32, None)
    assert rc == -1 and b"bad shape" in lib.onet_last_error()
    # outside the domain: refused (1) before anything is dereferenced or launched
    assert f(16, 0, 16, 16, 16, 0, None, None, 0, 1, 32, 64, 16, 48, None) == 1          # W = 48
    assert f(16, 0, 16, 16, 16, 0, None, None, 0, 1, 16, 64, 16, 32, None) in (1, -1)    # Cin = 16
    assert f(16, 0, 16, 16, 16, 0, None, None, 0, 1, 32, 96, 16, 32, None) == 1          # Cout = 96
    assert f(16, 0, 16, 16, 16, 0, None, None, 0, 1, 32, 64, 24, 32, None) == 1          # H = 24
    # inside the domain: misaligned slots and short batch strides are errors, still without a launch
    n_in, n_out = 32 * 16 * 32 // 2, 64 * 16 * 32 // 2
    rc = f(8, n_in, 16, 16, 16, n_out, None, None, 0, 1, 32, 64, 16, 32, None)
    assert rc == -1 and b"aligned" in lib.onet_last_error()
    rc = f(16, n_in, 16, 16, 8, n_out, None, None, 0, 1, 32, 64, 16, 32, None)
    assert rc == -1 and b"aligned" in lib.onet_last_error()
    rc = f(16, n_in - 4, 16, 16, 16, n_out, None, None, 0, 2, 32, 64, 16, 32, None)
    assert rc == -1 and b"stride" in lib.onet_last_error()
    rc = f(16, n_in, 16, 16, 16, n_out - 4, None, None, 0, 2, 32, 64, 16, 32, None)
    assert rc == -1 and b"stride" in lib.onet_last_error()
    rc = f(16, n_in, 16, 16, 16, n_out, None, 16, 2 * n_out - 4, 2, 32, 64, 16, 32, None)
    assert rc == -1 and b"stride" in lib.onet_last_error()
    rc = f(16, 8192 * 2048 * 2048 // 2, 16, 16, 16, 64 * 2048 * 2048 // 2, None, None, 0, 1, 8192, 64, 2048, 2048, None)
    assert rc == -1 and b"range" in lib.onet_last_error()


def test_layer_predicate_is_a_function_of_shapes_and_settings(monkeypatch):
    from onet_amd import ops
    monkeypatch.setattr(ops, "n_cu", lambda device=None: 256)
    with ops.using(ops.Settings(conv="bf16", fused_eval="bf16")):
        assert ops.eval_layer_ok_bf16(1, 32, 64, 16, 32)          # every legal layer under conv == "bf16"
        assert not ops.eval_layer_ok_bf16(1, 48, 64, 16, 32) and not ops.eval_layer_ok_bf16(1, 32, 96, 16, 32)
        assert not ops.eval_layer_ok_bf16(1, 32, 64, 24, 32) and not ops.eval_layer_ok_bf16(1, 32, 64, 16, 48)
        assert not ops.eval_layer_ok_bf16(1, 32, 64, 16, 16) and not ops.eval_layer_ok_bf16(1, 32, 64, 4096, 4096)
        assert ops.convt_slots_ok(4, 128, 64, 64, 64, parts=1) and ops.convt_slots_ok(4, 128, 64, 64, 64)
    with ops.using(ops.Settings(fused_eval="bf16")):               # conv == "auto": the fill rule, 192 tiles on 256 compute units
        assert ops.eval_layer_ok_bf16(4, 64, 128, 128, 128)       # 4 x 8 x 4 x 2 = 256 tiles
        assert not ops.eval_layer_ok_bf16(4, 128, 256, 64, 64)    # 4 x 4 x 2 x 4 = 128 tiles
        # explicit parts: the active conv ("auto": two parts) does not decide the one-part plan's byte range
        assert ops.convt_slots_ok(4, 128, 64, 64, 64, parts=1)
        assert ops.p16_empty(1, 8, 2, 2, "cpu", parts=1).dtype == ops.BF and ops.p16_empty(1, 8, 2, 2, "cpu", parts=1).shape[3] == 1
    with ops.using(ops.Settings(conv="direct", fused_eval="bf16")):     # no pre-split storage: nothing is taken
        assert not ops.eval_layer_ok_bf16(4, 64, 128, 128, 128)


def test_plan_on_cpu_model_reports_the_reason_and_the_operands():
    import onet_amd
    from onet_amd import ops
    m = onet_amd.Onet(in_chns=1, binit=True, bshare=True).eval()
    for st, want in ((ops.Settings(conv="bf16", fused_eval="bf16"), "bf16"), (ops.Settings(fused_eval="bf16"), "bf16"),
                     (ops.Settings(fused_eval=True), "fp16x2"), (ops.Settings(), None)):
        m.settings = st
        p = onet_amd.fused_eval_plan(m, (2, 1, 256, 256))
        assert p["fused"] is False and p["depth"] == 0 and "GPU" in p["reason"] and p["twin"] is True and p["batch"] == 4
        assert p["layers"] == {} and p["convt"] == {}
        assert "operands" in p and p["operands"] == want, (want, p)
