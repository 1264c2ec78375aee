"""The entry point of include/onet_hip_pairs.h: the one-part (plain bf16) _act launch on IMAGE-PAIR tiles -- maps of any H and
0 < W <= 16, two images of the batch side by side in a tile's 32 columns, each with its own halo columns.

The method is tests/test_gpu_anymap_kernels.py's (its helpers are imported): every output is a slice of a sentinel-filled buffer with a
batch stride above dense whose sentinel must be intact everywhere else.  The reference of every case is the EXISTING any-map entry
(ops.conv3x3_plain16_pre_act_anymap: one image per tile) on the same operands, and slots and `a` must be EQUAL value for value (`==`):
both instances add the same chunks and taps in the same order per pixel on the same MFMA shape and apply the same epilogue
expressions, so a difference is a bug and there is no tolerance.

What a pair tile can get wrong, and how a case would show it:
  * the right halo of image 0 / the left halo of image 1: a horizontal tap reading the neighbour image changes column W - 1 of image 0
    and column 0 of image 1.  Valid only if image 1's first column is non-zero and finite, which every case asserts;
  * stores beyond the map: at W < 16 the accumulators at columns W .. 15 of a half are relu(bn(partial sums)) -- the convolution of
    the zero-padded map -- not zero.  A store of them lands on the next row (`a`: rows of W floats) or, for the last row of the last
    channel, in the sentinel gap.  Every case with W < 16 computes those accumulators (the any-map entry on the map padded to 16
    columns) and asserts that they are finite and not all zero;
  * an odd batch: the last tile holds one image, its second half must stage zeros and store nothing -- the sentinel image behind
    the batch stays intact."""
import pytest
import torch

import test_gpu_anymap_kernels as ak
from test_gpu_anymap_kernels import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

rk = ak.rk
slots_out, f32_out, gap_intact, all_sentinel, same = ak.slots_out, ak.f32_out, ak.gap_intact, ak.all_sentinel, ak.same

CASES = [(2, 32, 64, 16, 16), (2, 32, 64, 14, 14), (2, 32, 64, 12, 12), (3, 32, 64, 12, 13), (1, 32, 64, 16, 16), (2, 32, 64, 20, 12),
         (4, 96, 128, 3, 9), (2, 1024, 1024, 14, 14)]
IDS = ["full-pair", "14x14", "12x12", "b3-12x13", "b1-16x16", "20x12", "b4-96to128-3x9", "1024to1024-14x14"]

_REF = {}


def _case(dev, batch, Cin, Cout, H, W):
    """operands of one case, the any-map entry's outputs on them and -- W < 16 -- on the map padded to 16 columns; computed once and
    left unchanged"""
    from onet_amd import ops
    key = (batch, Cin, Cout, H, W)
    if key not in _REF:
        x = rk.rnd(batch, Cin, H, W, seed=800).to(torch.bfloat16).float()
        w = rk.rnd(Cout, Cin, 3, 3, seed=801, scale=(2.0 / (Cin * 9)) ** 0.5)
        gamma = (rk.rnd(Cout, seed=802).abs() + 0.5) * torch.where(rk.rnd(Cout, seed=803) > 0.5, -1.0, 1.0)
        save = ops.bn_eval_coeffs(gamma.to(dev), rk.rnd(Cout, seed=804, scale=0.3).to(dev), rk.rnd(Cout, seed=805, scale=0.1).to(dev),
                                  (rk.rnd(Cout, seed=806) ** 2 + 0.5).to(dev), 1e-5)
        P, wq = ops.split_pack_act(x.to(dev), parts=1), ops.pack3x3_plain16(w.to(dev))[0]
        a_ref = torch.empty((batch, Cout, H, W), device=dev)
        aP_ref = ops.conv3x3_plain16_pre_act_anymap(P, wq, Cout, save, a=a_ref)
        assert aP_ref is not None
        a16 = None
        if W < 16:
            x16 = torch.zeros(batch, Cin, H, 16)
            x16[..., :W] = x
            a16 = torch.empty((batch, Cout, H, 16), device=dev)
            assert ops.conv3x3_plain16_pre_act_anymap(ops.split_pack_act(x16.to(dev), parts=1), wq, Cout, save, a=a16) is not None
        torch.cuda.synchronize()
        _REF[key] = dict(P=P, wq=wq, save=save, aP=aP_ref, a=a_ref, a16=a16)
    return _REF[key]


@pytest.mark.parametrize("with_a", [True, False], ids=["a", "no-a"])
@pytest.mark.parametrize("batch,Cin,Cout,H,W", CASES, ids=IDS)
def test_act_pairs_equals_the_anymap_entry(dev, batch, Cin, Cout, H, W, with_a):
    """slots and the optional fp32 activation == the any-map entry's on the same operands, one launch of the pair kind, nothing written
    outside the map or behind the batch"""
    from onet_amd import ops
    c = _case(dev, batch, Cin, Cout, H, W)
    assert bool((c["a"] > 0).any()) and bool((c["a"] == 0).any())
    if batch > 1:
        col0 = c["a"][1, :, :, 0]
        assert bool(torch.isfinite(col0).all()) and bool((col0 != 0).any()), "image 1's first column must be able to show a halo fault"
    if W < 16:
        beyond = c["a16"][..., W:]
        assert bool(torch.isfinite(beyond).all()) and bool((beyond != 0).any()), "the accumulators beyond the map must be able to show a stray store"
        assert same(c["a16"][..., :W], c["a"])            # (the padded map's own columns: the same convolution)
    # one image more than the batch in every buffer: the second half of an odd batch's last tile must not reach it
    aP_big, bigP = slots_out(Cout, H, W, dev, batch=batch + 1)
    a_big, bigA = f32_out(Cout, H, W, dev, batch=batch + 1)
    aP, a = aP_big[:batch], (a_big[:batch] if with_a else None)
    ops.profile_start(everything=False)
    try:
        assert ops.conv3x3_plain16_pre_act_pairs(c["P"], c["wq"], Cout, c["save"], out=aP, a=a) is aP
        torch.cuda.synchronize()
    finally:
        kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
    assert kinds == {"conv3x3_pre16_act_pairs_kernel": 1}, kinds
    assert same(aP, c["aP"]), "slots differ from the any-map entry's"
    assert torch.equal(aP.contiguous().view(torch.int16), c["aP"].contiguous().view(torch.int16))
    assert gap_intact(bigP[:batch], Cout // 8) and all_sentinel(bigP[batch:]), "a slot store left the map"
    if with_a:
        assert same(a, c["a"]), "fp32 activation differs from the any-map entry's"
        assert gap_intact(bigA[:batch], Cout) and all_sentinel(bigA[batch:]), "an fp32 store left the map"
    else:
        assert all_sentinel(bigA)


@pytest.mark.parametrize("Cin,Cout,W,amax", [(32, 64, 17, False), (48, 64, 14, False), (32, 96, 14, False), (32, 64, 14, True)],
                         ids=["W=17", "Cin=48", "Cout=96", "a_amax"])
def test_pairs_entry_refuses(dev, Cin, Cout, W, amax):
    """W > 16, Cin % 32 != 0, Cout % 64 != 0, a non-NULL a_amax: the entry answers 1 (None from the wrapper, which hands no a_amax on)
    and writes nothing"""
    from onet_amd import ops, _lib
    batch, H = 2, 14
    P = ops.split_pack_act(rk.rnd(batch, Cin, H, W, seed=860).to(dev), parts=1)
    wq = torch.zeros(Cin * 9 * Cout + 8, dtype=torch.bfloat16, device=dev)
    save = torch.zeros((4, Cout), device=dev)
    Cb = -(-Cout // 8) * 8
    aP, bigP = slots_out(Cb, H, W, dev)
    a, bigA = f32_out(Cout, H, W, dev)
    slots = ops.new_amax(dev)
    before = slots.clone()
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    rc = lib.onet_conv3x3_plain16_fwd_pre_act_pairs(P.data_ptr(), P.stride(0) // 2, wq.data_ptr(), save.data_ptr(), aP.data_ptr(), aP.stride(0) // 2,
                                                    slots.data_ptr() if amax else None, a.data_ptr(), a.stride(0), batch, Cin, Cout, H, W, st)
    assert rc == 1
    if not amax:
        assert ops.conv3x3_plain16_pre_act_pairs(P, wq, Cout, save, out=aP, a=a) is None
    torch.cuda.synchronize()
    assert all_sentinel(bigP) and all_sentinel(bigA)
    assert torch.equal(slots, before)
