"""Host side of labels-only inference (onet_amd.scores, onet_amd.segment(head="fused")): the three entry points' declarations and
argument checks, the pins the feature must not move (ABI version, Settings fields, the neighbours' signatures) and the Python surface
on a model that never touches a device."""
import ctypes
import inspect
import os

import pytest

PLAIN = ["xs", "xs_bs", "wq", "save", "L", "L_bs", "V", "B", "Cin", "Cout", "H", "W", "stream"]
SPLIT = ["xs", "xs_bs", "x_amax", "scale_always", "x_amax2", "split_ch", "wq", "save", "L", "L_bs", "V", "B", "Cin", "Cout", "H", "W", "stream"]
LABELS = ["Vt", "Vd", "S", "Y", "B", "HW", "stream"]


def test_entry_points_declared_and_exported():
    from onet_amd import _lib
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIBPATH) if os.path.exists(_lib.LIBPATH) else _lib.load()
    for name, names in (("onet_conv3x3_plain16_fwd_pre_head", PLAIN), ("onet_conv3x3_split_fwd_pre_head", SPLIT),
                        ("onet_softmax2_labels", LABELS)):
        assert name in protos, name
        assert hasattr(lib, name), name
        assert protos[name][2] == names and len(protos[name][1]) == len(names), (name, protos[name][2])
        assert protos[name][0] is ctypes.c_int


def test_neighbours_abi_and_settings_unchanged():
    from onet_amd import _lib, ops
    protos = _lib.parse_header()
    assert len(protos["onet_conv3x3_plain16_fwd_pre_act"][1]) == 15
    assert len(protos["onet_conv3x3_split_fwd_pre_act"][1]) == 20
    assert _lib.load().onet_abi_version() == 4
    slots = ("conv", "twin", "convt_bf16", "lazy_nan", "split", "bn_on_load", "split_f16", "grad_f16", "split_dgrad",
             "stem_fused", "sync_bn", "presplit", "z_bf16", "fused_eval")
    assert ops.Settings.__slots__ == slots and ops.Settings.__slots__[-1] == "fused_eval"


def _calls(lib):
    """-> [(name, call(xs, xs_bs, wq, save, L, L_bs, V, B, Cin, Cout, H, W), slot elements per 4-byte unit divisor, Cin step)]"""
    fp, fs = lib.onet_conv3x3_plain16_fwd_pre_head, lib.onet_conv3x3_split_fwd_pre_head

    def plain(xs, xs_bs, wq, save, L, L_bs, V, B, Cin, Cout, H, W):
        return fp(xs, xs_bs, wq, save, L, L_bs, V, B, Cin, Cout, H, W, None)

    def split(xs, xs_bs, wq, save, L, L_bs, V, B, Cin, Cout, H, W):
        return fs(xs, xs_bs, None, 0, None, 0, wq, save, L, L_bs, V, B, Cin, Cout, H, W, None)

    return (("plain16", plain, 2), ("split", split, 1))


@pytest.mark.parametrize("which", [0, 1], ids=["plain16", "split"])
def test_conv_head_bad_arguments_return_error_codes_without_a_device(which):
    from onet_amd import _lib
    lib = _lib.load()
    name, f, div = _calls(lib)[which]
    err = lib.onet_last_error
    # (16: a non-null, 16-byte aligned address nothing may dereference)
    n_in, n_L = 32 * 16 * 32 // div, 64 * 16 * 32
    for missing in range(5):                                   # each of xs, wq, save, L, V on its own
        p = [16, 16, 16, 16, 16]
        p[missing] = None
        rc = f(p[0], n_in, p[1], p[2], p[3], n_L, p[4], 1, 32, 64, 16, 32)
        assert rc == -1 and b"null" in err(), (name, missing)
    rc = f(16, n_in, 16, 16, 16, n_L, 16, 0, 32, 64, 16, 32)
    assert rc == -1 and b"bad shape" in err()
    # outside the domain: refused (1) before anything is dereferenced or launched
    assert f(16, 0, 16, 16, 16, 0, 16, 1, 32, 64, 16, 48) == 1                # W = 48
    assert f(16, 0, 16, 16, 16, 0, 16, 1, 32, 64, 24, 32) == 1                # H = 24
    assert f(16, 0, 16, 16, 16, 0, 16, 1, 32, 128, 16, 32) == 1               # Cout = 128: two channel tiles per pixel
    assert f(16, 0, 16, 16, 16, 0, 16, 1, 32, 192, 16, 32) == 1
    if name == "plain16":
        assert f(16, 0, 16, 16, 16, 0, 16, 1, 16, 64, 16, 32) == 1            # Cin = 16 on 32-channel chunks
    else:
        assert f(16, 0, 16, 16, 16, 0, 16, 1, 8, 64, 16, 32) == 1             # Cin = 8 on 16-channel chunks
    # inside the domain: misaligned operands and short batch strides are errors, still without a launch
    rc = f(8, n_in, 16, 16, 16, n_L, 16, 1, 32, 64, 16, 32)
    assert rc == -1 and b"aligned" in err()
    rc = f(16, n_in, 16, 16, 8, n_L, 16, 1, 32, 64, 16, 32)
    assert rc == -1 and b"aligned" in err()
    rc = f(16, n_in, 16, 16, 16, n_L + 2, 16, 2, 32, 64, 16, 32)              # L_bs not a multiple of 4 elements
    assert rc == -1 and b"aligned" in err()
    rc = f(16, n_in - 4, 16, 16, 16, n_L, 16, 2, 32, 64, 16, 32)
    assert rc == -1 and b"stride" in err()
    rc = f(16, n_in, 16, 16, 16, n_L - 4, 16, 2, 32, 64, 16, 32)
    assert rc == -1 and b"stride" in err()
    rc = f(16, 8192 * 2048 * 2048 // div, 16, 16, 16, 64 * 2048 * 2048, 16, 1, 8192, 64, 2048, 2048)
    assert rc == -1 and b"range" in err()


def test_softmax2_labels_bad_arguments():
    from onet_amd import _lib
    lib = _lib.load()
    f = lib.onet_softmax2_labels
    assert f(None, 16, 16, 16, 1, 64, None) == -1 and b"null" in lib.onet_last_error()
    assert f(16, None, 16, 16, 1, 64, None) == -1 and b"null" in lib.onet_last_error()
    assert f(16, 16, None, None, 1, 64, None) == -1
    assert f(16, 16, 16, 16, 0, 64, None) == -1 and f(16, 16, 16, 16, 1, 0, None) == -1


def test_python_surface_on_a_cpu_model():
    import torch
    import onet_amd
    from onet_amd import ops
    sig = inspect.signature(onet_amd.segment)
    assert "head" in sig.parameters and sig.parameters["head"].default is None
    assert inspect.signature(onet_amd.fused_eval_plan).parameters["head"].default is None
    assert "scores" in onet_amd.__all__ and "segment" in onet_amd.__all__ and callable(onet_amd.scores)
    for fn in ("conv3x3_plain16_pre_head", "conv3x3_split_pre_head", "softmax2_labels"):
        assert callable(getattr(ops, fn))
    m = onet_amd.Onet(in_chns=1, binit=True, bshare=True).eval()
    X = torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError):
        onet_amd.segment(m, X, head="bogus")
    with pytest.raises(ValueError):
        onet_amd.fused_eval_plan(m, (2, 1, 256, 256), head="bogus")
    for st in (ops.Settings(conv="bf16", fused_eval="bf16"), ops.Settings(fused_eval=True), ops.Settings()):
        m.settings = st
        p0 = onet_amd.fused_eval_plan(m, (2, 1, 256, 256))
        p1 = onet_amd.fused_eval_plan(m, (2, 1, 256, 256), head="fused")
        assert p1["fused"] is False and "GPU" in p1["reason"]
        assert sorted(p1) == sorted(p0) and p1 == p0
