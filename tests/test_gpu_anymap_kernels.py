"""The entry points of include/onet_hip_anymap.h: the one-part (plain bf16) _act and _act_pool launches on maps of ANY H and W -- odd,
W % 4 != 0 -- with fp32 side outputs stored float by float and floor pooling.

The method is tests/test_gpu_ragged_kernels.py's as it stands (its helpers are imported): the reference of every case is the EXISTING
full-tile entry point on the zero-padded canvas, the valid region must be EQUAL value for value (`==`), and every output is a slice
of a sentinel-filled buffer with a batch stride above dense whose sentinel must be intact everywhere else.  The pooled valid region
is [: H // 2, : W // 2] of the canvas launch: a 2 x 2 window that is only partly inside an odd map is pooled nowhere.

Two cases are built so that they can fail for the right reason, and say so:
  * 25 x 25 pooled (12 x 12): the window of pooled row / column 12 is partly outside the map.  A store of it would land on element
    (yp + 1, 0) of the pooled row-major map -- for the last row of an image's last channel, in the sentinel gap behind the image.
    The test requires the canvas value of that window to differ from the value that belongs there (and it is finite: not the sentinel).
  * `a` at W = 25: the lane at x = 24 holds pixels 24 .. 27; a float4 store would put three floats on the next row (for the last row
    of the last channel: into the sentinel gap), and rows of 25 floats are not 16-byte aligned."""
import pytest
import torch

import test_gpu_ragged_kernels as rk
from test_gpu_ragged_kernels import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

B, S32 = rk.B, rk.S32
slots_out, f32_out, gap_intact, all_sentinel, same, conv_case = rk.slots_out, rk.f32_out, rk.gap_intact, rk.all_sentinel, rk.same, rk.conv_case


# ----------------------------------------------------------------------------------------------------------------- act
@pytest.mark.parametrize("Cin,Cout,H,W", [(32, 64, 25, 25), (32, 64, 18, 50), (32, 64, 13, 22), (32, 64, 3, 5), (96, 128, 25, 26)],
                         ids=["25x25", "18x50", "13x22", "3x5", "96to128-25x26"])
def test_act_anymap_equals_the_canvas(dev, Cin, Cout, H, W):
    """slots and the fp32 activation == the full-tile entry on the zero-padded canvas; 96 -> 128: three chunks, two channel tiles"""
    from onet_amd import ops
    assert not ops._ragged_map(H, W)
    c = conv_case(dev, Cin, Cout, H, W)
    ac = torch.empty((B, Cout, c["Hc"], c["Wc"]), device=dev)
    aPc = ops.conv3x3_plain16_pre_act(c["Pc"], c["wq"], Cout, c["save"], a=ac)
    assert aPc is not None
    aP, bigP = slots_out(Cout, H, W, dev)
    a, bigA = f32_out(Cout, H, W, dev)
    assert ops.conv3x3_plain16_pre_act_anymap(c["P"], c["wq"], Cout, c["save"], out=aP, a=a) is aP
    torch.cuda.synchronize()
    assert bool((ac[:, :, :H, :W] > 0).any()) and bool((ac[:, :, :H, :W] == 0).any())
    if W == 25:
        # what a float4 store at x = 24 would put on the next row differs from what belongs there, and is no sentinel
        stray, legit = ac[:, :, :H, W:W + 3], ac[:, :, 1:H + 1, :3]
        assert bool(torch.isfinite(stray).all()) and bool((stray != legit).any())
    assert same(aP, aPc[:, :, :H, :, :W]), "slots differ from the canvas"
    assert same(a, ac[:, :, :H, :W]), "fp32 activation differs from the canvas"
    assert gap_intact(bigP, Cout // 8) and gap_intact(bigA, Cout), "a store left the map"
    # without the optional fp32 tensor: the same slots
    aP2, bigP2 = slots_out(Cout, H, W, dev)
    assert ops.conv3x3_plain16_pre_act_anymap(c["P"], c["wq"], Cout, c["save"], out=aP2) is aP2
    torch.cuda.synchronize()
    assert torch.equal(aP2.contiguous().view(torch.int16), aP.contiguous().view(torch.int16)) and gap_intact(bigP2, Cout // 8)


# ----------------------------------------------------------------------------------------------------------------- act_pool
_POOL = {}


def _pool_canvas(dev, H, W):
    """the canvas launch of a pooled case (skip slots, fp32 L, pooled slots, pooled fp32), computed once and left unchanged"""
    from onet_amd import ops
    if (H, W) not in _POOL:
        Cout = 64
        c = conv_case(dev, 32, Cout, H, W)
        Hc, Wc = c["Hc"], c["Wc"]
        Lc = torch.empty((B, Cout, Hc, Wc), device=dev)
        yPc = torch.empty((B, Cout // 8, Hc // 2, 1, Wc // 2, 8), dtype=torch.bfloat16, device=dev)
        yc = torch.empty((B, Cout, Hc // 2, Wc // 2), device=dev)
        aPc = ops.conv3x3_plain16_pre_act_pool(c["Pc"], c["wq"], Cout, c["save"], a=Lc, yP=yPc, y=yc)
        assert aPc is not None
        torch.cuda.synchronize()
        _POOL[(H, W)] = (c, aPc, Lc, yPc, yc)
    return _POOL[(H, W)]


@pytest.mark.parametrize("dests", ["yP", "y", "both+a"])
@pytest.mark.parametrize("H,W", [(26, 50), (25, 25), (7, 9), (24, 42)], ids=["26x50", "25x25", "7x9", "24x42"])
def test_act_pool_anymap_equals_the_canvas(dev, H, W, dests):
    """skip slots, the pooled slots / pooled fp32 (rows of 25, 12, 4, 21 floats) and, with both, fp32 L == the full-tile entry on the
    canvas, the pooled region being [: H // 2, : W // 2] of it; a destination that is not given stays untouched"""
    from onet_amd import ops
    assert not ops._ragged_map(H, W)
    Cout, Hp, Wp = 64, H // 2, W // 2
    c, aPc, Lc, yPc, yc = _pool_canvas(dev, H, W)
    if (H, W) == (25, 25):
        # the window of pooled row / column 12 is partly outside the map: its canvas value differs from what belongs at the element
        # a store of it would hit -- (yp + 1, 0) for column 12, the next channel's row 0 for row 12 -- and is finite (no sentinel)
        col, row = yc[:, :, :Hp, Wp], yc[:, :, Hp, :Wp + 1]
        assert bool(torch.isfinite(col).all()) and bool(torch.isfinite(row).all())
        assert bool((col[:, :, :-1] != yc[:, :, 1:Hp, 0]).any()) and bool((row[:, :-1, :Wp] != yc[:, 1:, 0, :Wp]).any())
        assert bool((col > 0).any()) and bool((row > 0).any())
    aP, bigP = slots_out(Cout, H, W, dev)
    L, bigL = f32_out(Cout, H, W, dev)
    yP, bigyP = slots_out(Cout, Hp, Wp, dev)
    y, bigy = f32_out(Cout, Hp, Wp, dev)
    kw = dict(yP=yP) if dests == "yP" else dict(y=y) if dests == "y" else dict(yP=yP, y=y, a=L)
    assert ops.conv3x3_plain16_pre_act_pool_anymap(c["P"], c["wq"], Cout, c["save"], out=aP, **kw) is aP
    torch.cuda.synchronize()
    assert same(aP, aPc[:, :, :H, :, :W]) and gap_intact(bigP, Cout // 8), "skip slots"
    if "yP" in kw:
        assert same(yP, yPc[:, :, :Hp, :, :Wp]) and gap_intact(bigyP, Cout // 8), "pooled slots"
    else:
        assert all_sentinel(bigyP)
    if "y" in kw:
        assert same(y, yc[:, :, :Hp, :Wp]) and bool((y > 0).any()) and gap_intact(bigy, Cout), "pooled fp32"
    else:
        assert all_sentinel(bigy)
    if "a" in kw:
        assert same(L, Lc[:, :, :H, :W]) and gap_intact(bigL, Cout), "fp32 L"
    else:
        assert all_sentinel(bigL)


# ----------------------------------------------------------------------------------------------------------------- the ragged domain
def test_anymap_entries_on_a_ragged_map_are_the_ragged_entries(dev):
    """24 x 40: each new entry launches what its ragged sibling launches -- the same bits, the same launch kinds"""
    from onet_amd import ops
    Cin, Cout, H, W = 32, 64, 24, 40
    c = conv_case(dev, Cin, Cout, H, W)
    got = {}
    for tag, act, act_pool in (("ragged", ops.conv3x3_plain16_pre_act_ragged, ops.conv3x3_plain16_pre_act_pool_ragged),
                               ("anymap", ops.conv3x3_plain16_pre_act_anymap, ops.conv3x3_plain16_pre_act_pool_anymap)):
        aP, bigP = slots_out(Cout, H, W, dev)
        a, bigA = f32_out(Cout, H, W, dev)
        aP2, bigP2 = slots_out(Cout, H, W, dev)
        L, bigL = f32_out(Cout, H, W, dev)
        yP, bigyP = slots_out(Cout, H // 2, W // 2, dev)
        y, bigy = f32_out(Cout, H // 2, W // 2, dev)
        ops.profile_start(everything=False)
        try:
            assert act(c["P"], c["wq"], Cout, c["save"], out=aP, a=a) is aP
            assert act_pool(c["P"], c["wq"], Cout, c["save"], out=aP2, a=L, yP=yP, y=y) is aP2
            torch.cuda.synchronize()
        finally:
            kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
        got[tag] = (kinds, [t.clone() for t in (bigP, bigA, bigP2, bigL, bigyP, bigy)])
    assert got["ragged"][0] == got["anymap"][0] == {"conv3x3_pre16_act_kernel": 1, "conv3x3_pre16_act_pool_kernel": 1}, got
    for r, n in zip(got["ragged"][1], got["anymap"][1]):
        bits = torch.int16 if r.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(r.view(bits), n.view(bits))


# ----------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("Cin,Cout,amax", [(48, 64, False), (32, 96, False), (32, 64, True)], ids=["Cin%32", "Cout%64", "a_amax"])
def test_anymap_entries_refuse(dev, Cin, Cout, amax):
    """Cin % 32 != 0, Cout % 64 != 0, a non-NULL a_amax: both entries answer 1 (None from the wrapper, which hands no a_amax on) and
    write nothing"""
    from onet_amd import ops, _lib
    H, W = 25, 25
    P = ops.split_pack_act(rk.rnd(B, Cin, H, W, seed=760).to(dev), parts=1)
    wq = torch.zeros(Cin * 9 * Cout + 8, dtype=torch.bfloat16, device=dev)
    save = torch.zeros((4, Cout), device=dev)
    Hp, Wp = H // 2, W // 2
    Cb = -(-Cout // 8) * 8
    aP, bigP = slots_out(Cb, H, W, dev)
    a, bigA = f32_out(Cout, H, W, dev)
    yP, bigyP = slots_out(Cb, Hp, Wp, dev)
    y, bigy = f32_out(Cout, Hp, Wp, dev)
    slots = ops.new_amax(dev)
    before = slots.clone()
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    am = slots.data_ptr() if amax else None
    rc = lib.onet_conv3x3_plain16_fwd_pre_act_anymap(P.data_ptr(), P.stride(0) // 2, wq.data_ptr(), save.data_ptr(), aP.data_ptr(), aP.stride(0) // 2,
                                                     am, a.data_ptr(), a.stride(0), B, Cin, Cout, H, W, st)
    assert rc == 1
    rc = lib.onet_conv3x3_plain16_fwd_pre_act_pool_anymap(P.data_ptr(), P.stride(0) // 2, wq.data_ptr(), save.data_ptr(), aP.data_ptr(),
                                                          aP.stride(0) // 2, am, a.data_ptr(), a.stride(0), yP.data_ptr(), yP.stride(0) // 2,
                                                          y.data_ptr(), y.stride(0), B, Cin, Cout, H, W, st)
    assert rc == 1
    if not amax:
        assert ops.conv3x3_plain16_pre_act_anymap(P, wq, Cout, save, out=aP, a=a) is None
        assert ops.conv3x3_plain16_pre_act_pool_anymap(P, wq, Cout, save, out=aP, a=a, yP=yP, y=y) is None
    torch.cuda.synchronize()
    assert all_sentinel(bigP) and all_sentinel(bigA) and all_sentinel(bigyP) and all_sentinel(bigy)
    assert torch.equal(slots, before)
