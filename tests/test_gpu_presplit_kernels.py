"""The pre-split convolution kernels of onet_amd/csrc/conv_split.hip, instance by instance, against fp64.

The default fp32 training step runs its 3x3 convolutions on these kernels: operands stored pre-split by their producers in the
slot layout [B][C/8][H][parts][W][8] -- fp16 (hi | mid), bf16 (hi | mid) (Settings(split_f16=False)) or one part of plain bf16
(conv == "bf16") -- and staged by LDS-DMA.  Every launchable instance is held here to the fp64 result of the same operation:
fp16 (hi | mid) to 2e-6 of the output scale (4e-6 where the reduction runs over more than 128 channels), bf16 (hi | mid) to 2e-5
(3e-5 for the weight gradient), plain bf16 to 2e-6 (4e-6 for the weight gradient) of the fp64 result of the bf16-ROUNDED operands.
Statistics records must finalise to the fp64 mean (within 2e-6 of the channel's standard deviation) and variance (1e-5 relative)
of the fp64 z, with counts of exactly B * H * W.

Forward, onet_conv3x3_split_fwd_pre -> launch_split_pre<ST, PM, W16>.  PM: 0 bf16 (hi | mid) pack, 1 fp16 (hi | mid) pack, 2 plain
bf16 pack (wq_f16 = 2); ST: a statistics buffer is passed (`stats=`); W16: W == 16 (even B, H % 16 == 0).  Kernel: conv3x3_pre16_kernel
where P16 = RD || PM == 2 || (ST && !W16), else conv3x3_split_pre_kernel (32x32x16).  Each instance runs on the shapes of
FWD_SHAPES[W16]; ragged: W = 48 with H = 20 (partial column tile and row band, ST = 0 only), Cout = 72 / 40 (partial Cout tile).
Those shapes have at most a few dozen tiles, one per persistent block; the multi-tile shapes (Cout = multi_tile_cout(..), derived from
the device's CU count) give the blocks two tiles or one, unevenly -- once per kernel and path that walks tiles, in the forward, fused-reduce
and pre-split-half tables here and in the fp32-in and fused-eval kernel tests of test_gpu_ops.py / test_gpu_fused_eval.py.

    ST PM W16  kernel       test
    0  0  0    split_pre    test_forward_instance[bf16x2-wide-*], test_presplit_entries_fuzz
    0  1  0    split_pre    test_forward_instance[fp16x2-wide-*], test_forward_guard_single_slot_set, test_forward_two_producer_concat
    0  2  0    pre16        test_forward_instance[plain-wide-*], test_presplit_entries_fuzz
    1  0  0    pre16        test_forward_instance[bf16x2-wide-*]
    1  1  0    pre16        test_forward_instance[fp16x2-wide-*], test_forward_guard_single_slot_set, test_forward_two_producer_concat
    1  2  0    pre16        test_forward_instance[plain-wide-*]
    0  0  1    split_pre    test_forward_instance[bf16x2-w16-*]
    0  1  1    split_pre    test_forward_instance[fp16x2-w16-*], test_forward_guard_single_slot_set, test_forward_two_producer_concat
    0  2  1    pre16        test_forward_instance[plain-w16-*]
    1  0  1    split_pre    test_forward_instance[bf16x2-w16-*]
    1  1  1    split_pre    test_forward_instance[fp16x2-w16-*], test_forward_guard_single_slot_set, test_forward_two_producer_concat
    1  2  1    pre16        test_forward_instance[plain-w16-*]

Input gradient with the fused BatchNorm-backward reduce, onet_conv3x3_split_dgrad_pre_bnreduce -> launch_split_pre<0, PM, W16, RD>
(conv3x3_pre16_kernel; wq_f16 selects PM; 16-pixel maps only with plain bf16 operands, else the entry returns 1):

    PM W16  test
    0  0    test_dgrad_bnreduce_instance[bf16x2-wide-*]
    1  0    test_dgrad_bnreduce_instance[fp16x2-wide-*]
    2  0    test_dgrad_bnreduce_instance[plain-wide-*]
    2  1    test_dgrad_bnreduce_instance[plain-w16-*]

Input gradient with a pre-split upper half, onet_conv3x3_split_dgrad_pre_slots -> launch_split_pre<0, 1, 0> (conv3x3_split_pre_kernel)
and launch_split_pre<0, 2, 0> (conv3x3_pre16_kernel) with SpPreArgs::zP set: test_dgrad_pre_slots_instance[fp16x2-*, plain-*].  The
entry takes only full 16 x 32 tiles and Cout, ch0 % 64 == 0, so no ragged shape exists; the two shapes differ in ch0 and tiles.

Weight gradient, onet_conv3x3_split_wgrad_pre -> ONET_SWP_LAUNCH(G, COT, F) = conv3x3_wgrad_pre16_kernel<G, COT, F>.  G: images per
unit (1: W >= 64, 2: W == 32, 4: W == 16); COT 128 where Cout % 128 == 0 and W >= 32, else 64; F: the operands' form (0 bf16
(hi | mid), 1 fp16 (hi | mid), 2 plain bf16).  Every F runs on every shape of WGRAD_SHAPES[(G, COT)]:

    G COT  test
    1  64  test_wgrad_instance[G1-COT64-*], test_wgrad_two_producer_concat
    1 128  test_wgrad_instance[G1-COT128-*], test_wgrad_two_producer_concat
    2  64  test_wgrad_instance[G2-COT64-*]
    2 128  test_wgrad_instance[G2-COT128-*], test_wgrad_two_producer_concat
    4  64  test_wgrad_instance[G4-COT64-*], test_wgrad_two_producer_concat
    4 128  compiled, not reachable (split_wgrad_cot takes COT = 128 only on maps >= 32 pixels wide)

test_presplit_entries_fuzz draws shapes from the entries' own ONET_REQUIRE domains and checks that the predicates
(onet_conv3x3_split_pre_nparts, onet_conv3x3_split_wgrad_pre_ok) agree with what the entries accept."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multi_tile import multi_tile_cout

pytestmark = pytest.mark.gpu

PM_NAMES = {0: "bf16x2", 1: "fp16x2", 2: "plain"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from onet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = np.random.Generator(np.random.PCG64([seed, *shape]))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def close(a, b, tol, what):
    """max |a - b| <= tol * max |b| (b: the fp64 reference)"""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max()) + 1e-300
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def tol_conv(pm, K):
    """forward / input-gradient tolerance for a reduction over K channels"""
    return {0: 2e-5, 1: 4e-6 if K > 128 else 2e-6, 2: 2e-6}[pm]


TOL_WGRAD = {0: 3e-5, 1: 2e-6, 2: 4e-6}


def packs(w, pm):
    """(forward pack, input-gradient pack) of w for operand form pm"""
    from onet_amd import ops
    if pm == 2:
        return ops.pack3x3_plain16(w)
    with ops.using(ops.Settings(conv="auto", split_f16=bool(pm), grad_f16=bool(pm))):
        qf, qd = ops.pack3x3_split(w)
    want = torch.float16 if pm == 1 else torch.bfloat16
    assert qd.dtype == want and (qf is None or qf.dtype == want)
    return qf, qd


def act(x, pm, **kw):
    """x pre-split in operand form pm"""
    from onet_amd import ops
    return ops.split_pack_act(x, f16=pm == 1, parts=1 if pm == 2 else 2, **kw)


def grad_operand(g, pm):
    """-> (pre-split g, kwargs for its consumer): fp16 parts scaled by the producers' `always` rule (max |.| in [2^13, 2^14))"""
    from onet_amd import ops
    if pm != 1:
        return act(g, pm), {}
    k = 13 - math.floor(math.log2(float(g.abs().max())))
    return ops.split_pack_act(g, f16=True, scale=2.0 ** k), dict(slots=ops.absmax_slots(g), always=True)


def ref_op(t, pm):
    """the fp64 operand the kernel's result is compared against: plain bf16 operands are rounded first"""
    t = t.detach().cpu()
    return t.to(torch.bfloat16).double() if pm == 2 else t.double()


def conv64(x, w):
    return F.conv2d(x, w, None, 1, 1)


def dgrad64(g, w):
    return F.conv2d(g, w.flip(2, 3).transpose(0, 1), None, 1, 1)


def wgrad64(x, g, shape):
    return torch.nn.grad.conv2d_weight(x, shape, g, padding=1)


def nan_out(B, C, H, W, dev, dtype=torch.float32):
    return torch.full((B, C, H, W), float("nan"), dtype=dtype, device=dev)


def fwd_pre(xP, wq, Cout, stats=None, **kw):
    """the forward entry into a NaN-filled output: a dropped store cannot hide behind a stale allocation"""
    B, _, H, _, W, _ = xP.shape
    from onet_amd import ops
    return ops.conv3x3_split_pre(xP, wq, Cout, out=nan_out(B, Cout, H, W, xP.device), stats=stats, **kw)


def new_stats(Cout, B, H, W, dev):
    from onet_amd import _lib
    nparts = int(_lib.load().onet_conv3x3_split_pre_nparts(B, H, W))
    assert nparts > 0
    return torch.full((Cout, nparts, 3), float("nan"), device=dev)


def check_stats(cm, z64, what):
    """the (n, mean, M2) records of every channel finalised in fp64 == the fp64 mean and variance of the fp64 z"""
    B, C, H, W = z64.shape
    r = cm.detach().cpu().double()
    assert torch.isfinite(r).all(), what
    n = r[:, :, 0].sum(1)
    assert float(n.min()) == float(n.max()) == B * H * W, (what, float(n.min()), float(n.max()))
    mean = (r[:, :, 0] * r[:, :, 1]).sum(1) / n
    var = (r[:, :, 2] + r[:, :, 0] * (r[:, :, 1] - mean[:, None]) ** 2).sum(1) / n
    zm, zv = z64.mean((0, 2, 3)), z64.var((0, 2, 3), unbiased=False)
    em = float(((mean - zm).abs() / zv.sqrt()).max())
    ev = float(((var - zv).abs() / zv).max())
    assert em <= 2e-6, f"{what}: mean off by {em:.3e} of std"
    assert ev <= 1e-5, f"{what}: variance off by {ev:.3e} relative"


def unsplit(P, scale=1.0):
    """pre-split slots [B][C/8][H][parts][W][8] -> fp64 [B][C][H][W] (the parts summed, the producer's scale undone)"""
    B, C8, H, _, W, _ = P.shape
    v = P.detach().cpu().double().sum(3)
    return v.permute(0, 1, 4, 2, 3).reshape(B, C8 * 8, H, W) / scale


# ----------------------------------------------------------------------------------------------------------- forward instances
# B, Cin, Cout, H, W, with statistics; Cin is a multiple of 32 so that every operand form takes the shape
FWD_SHAPES = {
    False: [(2, 64, 40, 20, 48, False),        # partial column tile, H % 16 != 0, partial Cout tile (no statistics: not full tiles)
            (2, 64, 72, 32, 64, True),         # partial Cout tile
            (1, 160, 64, 16, 96, True),        # three column tiles, > 128 channels
            (3, 32, None, 48, 96, True)],      # 27 spatial tiles, Cout = multi_tile_cout(27): more than one tile per block
    True: [(4, 64, 40, 16, 16, True),          # partial Cout tile
           (2, 160, 64, 32, 16, True),
           (6, 32, None, 48, 16, True)],       # 9 pair-tiles, Cout = multi_tile_cout(9)
}
# the multi-tile shapes run once per kernel and path that walks tiles: conv3x3_split_pre_kernel without (fp16 parts, wide) and with
# statistics (W16), conv3x3_pre16_kernel with statistics (fp16 parts, wide) and on plain bf16 operands (W16)
MULTI_TILE_FWD = {(1, False), (1, True), (2, True)}


FWD_CASES = [(pm, w16, i) for pm in (0, 1, 2) for w16 in (False, True) for i in range(len(FWD_SHAPES[w16]))
             if FWD_SHAPES[w16][i][2] is not None or (pm, w16) in MULTI_TILE_FWD]


@pytest.mark.parametrize("pm,w16,shape", FWD_CASES, ids=[f"{PM_NAMES[p]}-{'w16' if w else 'wide'}-{i}" for p, w, i in FWD_CASES])
def test_forward_instance(dev, pm, w16, shape):
    """launch_split_pre<ST, PM, W16> for ST = 0 and (where the map is made of full tiles) ST = 1 against the fp64 convolution;
    the statistics records against the fp64 mean and variance; both launches store the same z bit for bit."""
    from onet_amd import _lib
    B, Cin, Cout, H, W, st = FWD_SHAPES[w16][shape]
    if Cout is None:
        Cout = multi_tile_cout((B // 2 if w16 else B * (W // 32)) * (H // 16))
    x = rnd(B, Cin, H, W, seed=101)
    w = rnd(Cout, Cin, 3, 3, seed=102, scale=(2.0 / (Cin * 9)) ** 0.5)
    z64 = conv64(ref_op(x, pm), ref_op(w, pm))
    qf, _ = packs(w.to(dev), pm)
    xP = act(x.to(dev), pm)
    what = f"{PM_NAMES[pm]} forward {(B, Cin, Cout, H, W)}"
    z = fwd_pre(xP, qf, Cout)
    close(z, z64, tol_conv(pm, Cin), what)
    if not st:
        assert int(_lib.load().onet_conv3x3_split_pre_nparts(B, H, W)) == 0
        with pytest.raises(_lib.OnetHipError):
            fwd_pre(xP, qf, Cout, stats=torch.empty((Cout, 1, 3), device=dev))
        return
    cm = new_stats(Cout, B, H, W, dev)
    zs = fwd_pre(xP, qf, Cout, stats=cm)
    close(zs, z64, tol_conv(pm, Cin), what + " with statistics")
    check_stats(cm, z64, what)
    if pm == 2 or w16:      # (the same kernel with and without statistics: P16 does not depend on ST here)
        assert torch.equal(z, zs), "the statistics epilogue changes z"


# ------------------------------------------------------------------------------------- input gradient with the fused reduce
# B, Cd (reduction: the dz channels), Ca (output: da channels), H, W, statistics groups
RD_SHAPES = {
    (0, False): [(2, 64, 80, 32, 64, 1), (4, 128, 64, 16, 96, 2)],
    (1, False): [(2, 64, 80, 32, 64, 1), (4, 192, 64, 16, 96, 2)],
    (2, False): [(2, 128, 80, 32, 64, 1), (4, 160, 64, 16, 96, 2),
                 (3, 128, None, 48, 96, 3)],      # Ca = multi_tile_cout(27): more than one tile per block (four chunks: the entry's minimum)
    (2, True): [(4, 128, 48, 16, 16, 2), (2, 128, 64, 32, 16, 1)],
}


RD_CASES = [(pm, w16, i) for (pm, w16) in RD_SHAPES for i in range(len(RD_SHAPES[(pm, w16)]))]


@pytest.mark.parametrize("pm,w16,shape", RD_CASES, ids=[f"{PM_NAMES[p]}-{'w16' if w else 'wide'}-{i}" for p, w, i in RD_CASES])
def test_dgrad_bnreduce_instance(dev, pm, w16, shape):
    """launch_split_pre<0, PM, W16, RD>: da against the fp64 input gradient; the reduce records -- (hi, lo) pairs per tile -- against
    the fp64 sums of dy = da * (relu mask) and dy * xhat formed from the fp64 da, per statistics group (4e-6 of sum |dy|).  The
    first shape has a partial Cout tile (Ca % 64 != 0)."""
    from onet_amd import ops
    B, Cd, Ca, H, W, G = RD_SHAPES[(pm, w16)][shape]
    if Ca is None:
        Ca = multi_tile_cout(B * (W // 32) * (H // 16))
    dz = rnd(B, Cd, H, W, seed=111, scale=1e-3)
    w = rnd(Cd, Ca, 3, 3, seed=112, scale=(2.0 / (9 * Ca)) ** 0.5)
    zp = (rnd(B, Ca, H, W, seed=113) * 1.5 + 0.2).to(dev)
    gamma, beta = (1 + 0.1 * rnd(Ca, seed=114)).to(dev), (0.1 * rnd(Ca, seed=115)).to(dev)
    save = torch.empty(G, 4, Ca, device=dev)
    Bg = B // G
    for gi in range(G):
        ops.bn_train_coeffs(zp[gi * Bg:(gi + 1) * Bg], gamma, beta, None, None, 0.1, 1e-5, save=save[gi])
    da64 = dgrad64(ref_op(dz, pm), ref_op(w, pm))
    _, qd = packs(w.to(dev), pm)
    dzP, kw = grad_operand(dz.to(dev), pm)
    got = ops.conv3x3_split_dgrad_pre_bnreduce(dzP, qd, Ca, zp, save, want_amax=True, **kw)
    assert got is not None, "shape not taken by the fused kernel"
    da, rec4, am = got
    what = f"{PM_NAMES[pm]} RD {(B, Cd, Ca, H, W, G)}"
    close(da, da64, tol_conv(pm, Cd), what)
    r = rec4.double().view(G, -1, Ca, 4).sum(1).cpu()
    for gi in range(G):
        s_ = slice(gi * Bg, (gi + 1) * Bg)
        mean, inv, scl, sh = (save[gi, i].view(1, -1, 1, 1) for i in range(4))
        mask = (torch.addcmul(sh, zp[s_] - mean, scl) > 0).cpu()           # the kernel's fp32 expression
        dy = da64[s_] * mask
        xhat = ((zp[s_].double() - mean.double()) * inv.double()).cpu()
        s1, s2, n1 = dy.sum((0, 2, 3)), (dy * xhat).sum((0, 2, 3)), dy.abs().sum((0, 2, 3))
        assert float(((r[gi, :, 0] + r[gi, :, 1] - s1).abs() / n1).max()) <= 4e-6, what + ": sum dy"
        assert float(((r[gi, :, 2] + r[gi, :, 3] - s2).abs() / n1).max()) <= 4e-6, what + ": sum dy * xhat"
    assert float(torch.tensor(am.cpu().numpy().view("float32")).max()) == float(da.abs().max())
    if pm != 2 and shape == 0:
        # the entry declines (returns 1, nothing launched) 16-pixel maps in (hi | mid) parts: that instance is not built
        P16, kw16 = grad_operand(torch.full((4, Cd, 16, 16), 1e-3, device=dev), pm)
        assert ops.conv3x3_split_dgrad_pre_bnreduce(P16, qd, Ca, torch.zeros(4, Ca, 16, 16, device=dev), save[:1], **kw16) is None


# -------------------------------------------------------------------------------------- input gradient with a pre-split half
@pytest.mark.parametrize("pm", [1, 2], ids=lambda p: PM_NAMES[p])
@pytest.mark.parametrize("B,Cd,Ca,H,W,ch0", [(2, 64, 128, 16, 32, 64), (1, 96, 192, 32, 64, 64),
                                             (3, 32, None, 48, 96, None)])    # Ca = multi_tile_cout(27), ch0 = about half of it: blocks walk more than one tile
def test_dgrad_pre_slots_instance(dev, pm, B, Cd, Ca, H, W, ch0):
    """launch_split_pre<0, PM, 0> with SpPreArgs::zP: channels < ch0 of da as fp32, channels >= ch0 pre-split.  Both against the fp64
    input gradient: the fp32 half at the forward tolerance, the pre-split half unscaled by the bound's `always` scale (fp16 parts) or
    within one bf16 rounding of the fp64 value (plain bf16)."""
    from onet_amd import ops
    if Ca is None:
        Ca = multi_tile_cout(B * (W // 32) * (H // 16))
        ch0 = Ca // 128 * 64
    dz = rnd(B, Cd, H, W, seed=121, scale=1e-3)
    w = rnd(Cd, Ca, 3, 3, seed=122, scale=(2.0 / (9 * Ca)) ** 0.5)
    da64 = dgrad64(ref_op(dz, pm), ref_op(w, pm))
    _, qd = packs(w.to(dev), pm)
    dzP, kw = grad_operand(dz.to(dev), pm)
    bound = ops.conv3x3_dgrad_bound(w.to(dev), kw["slots"], ch0) if pm == 1 else None
    da, daP = ops.conv3x3_split_dgrad_pre_slots(dzP, qd, Ca, ch0, bound, **kw)
    what = f"{PM_NAMES[pm]} dgrad_pre_slots {(B, Cd, Ca, H, W, ch0)}"
    close(da[:, :ch0], da64[:, :ch0], tol_conv(pm, Cd), what + " fp32 half")
    up = da64[:, ch0:]
    if pm == 1:
        bv = float(torch.tensor(bound.cpu().numpy().view("float32")).max())
        kb = 13 - math.floor(math.log2(bv))
        close(unsplit(daP, 2.0 ** kb), up, tol_conv(pm, Cd), what + " pre-split half")
    else:
        err = (unsplit(daP) - up).abs()
        assert bool((err <= 2.0 ** -8 * up.abs() + 2e-6 * float(up.abs().max())).all()), what + " pre-split half"


# ------------------------------------------------------------------------------------------------------- weight gradient
# B, Cin, Cout, H, W per (G, COT); the first shape of each is ragged (W % 64 != 0, H odd, Cin / Cout % 64 != 0)
WGRAD_SHAPES = {
    (1, 64): [(2, 40, 72, 19, 80), (1, 64, 64, 16, 64)],
    (1, 128): [(2, 48, 128, 9, 100), (1, 64, 256, 16, 64)],
    (2, 64): [(4, 40, 64, 17, 32), (2, 64, 96, 16, 32)],
    (2, 128): [(4, 24, 128, 7, 32), (2, 64, 128, 16, 32)],
    (4, 64): [(8, 24, 40, 9, 16), (4, 64, 64, 16, 16)],
}


def wgrad_pre(x, g, pm):
    """the weight-gradient entry on pre-split x and dz (fp16 parts: dz scaled by the `always` rule) into a NaN-filled dw"""
    from onet_amd import ops
    gP, kw = grad_operand(g, pm)
    shape = (g.shape[1], x.shape[1], 3, 3)
    return ops.conv3x3_split_wgrad_pre(act(x, pm), gP, shape, out=torch.full(shape, float("nan"), device=x.device),
                                       dz_slots=kw.get("slots"))


WGRAD_CASES = [(G, COT, i) for (G, COT) in WGRAD_SHAPES for i in range(2)]


@pytest.mark.parametrize("G,COT,shape", WGRAD_CASES, ids=[f"G{g}-COT{c}-{i}" for g, c, i in WGRAD_CASES])
def test_wgrad_instance(dev, G, COT, shape):
    """conv3x3_wgrad_pre16_kernel<G, COT, F> for F = 0, 1, 2 against the fp64 weight gradient (fp16 parts: dz scaled by the
    producers' `always` rule, undone from dz_slots, as in the model)."""
    from onet_amd import _lib, ops
    B, Cin, Cout, H, W = WGRAD_SHAPES[(G, COT)][shape]
    assert (W >= 64 and G == 1) or W == 64 // G
    assert COT == (128 if Cout % 128 == 0 and W >= 32 else 64)
    assert _lib.load().onet_conv3x3_split_wgrad_pre_ok(B, Cin, Cout, H, W)
    x = rnd(B, Cin, H, W, seed=131)
    g = rnd(B, Cout, H, W, seed=132)
    for pm in (0, 1, 2):
        dw64 = wgrad64(ref_op(x, pm), ref_op(g, pm), (Cout, Cin, 3, 3))
        close(wgrad_pre(x.to(dev), g.to(dev), pm), dw64, TOL_WGRAD[pm], f"{PM_NAMES[pm]} wgrad {(B, Cin, Cout, H, W)}")


# ------------------------------------------------------------------------------------------------------- magnitude slots
@pytest.mark.parametrize("B,Cin,Cout,H,W,st", [(2, 64, 72, 32, 64, True), (2, 48, 40, 20, 48, False), (4, 64, 64, 16, 16, True),
                                               (4, 160, 40, 16, 16, False)])
def test_forward_guard_single_slot_set(dev, B, Cin, Cout, H, W, st):
    """fp16 (hi | mid) forward of an activation beyond fp16's range (bound >= 2^15, guard rule): scaled by its producer from its
    slots and unscaled by the kernel from the same slots, held to fp64; without the slots the parts overflow (the guard is what
    saves the result).  An ordinary tensor is untouched by the guard: bit-identical with and without its slots."""
    from onet_amd import ops
    x = rnd(B, Cin, H, W, seed=141)
    w = rnd(Cout, Cin, 3, 3, seed=142, scale=(2.0 / (Cin * 9)) ** 0.5)
    qf, _ = packs(w.to(dev), 1)
    xb = (x * 3e5).to(dev)
    assert float(xb.abs().max()) >= 2 ** 15
    sl = ops.absmax_slots(xb)
    z64 = conv64(xb.double().cpu(), w.double())
    cm = new_stats(Cout, B, H, W, dev) if st else None
    z = fwd_pre(ops.split_pack_act(xb, f16=True, slots=sl), qf, Cout, stats=cm, slots=sl)
    what = f"guarded forward {(B, Cin, Cout, H, W)}"
    close(z, z64, tol_conv(1, Cin), what)
    if st:
        check_stats(cm, z64, what)
    assert not torch.isfinite(fwd_pre(ops.split_pack_act(xb, f16=True), qf, Cout)).all()
    xd = x.to(dev)
    so = ops.absmax_slots(xd)
    cm0 = new_stats(Cout, B, H, W, dev) if st else None
    cm1 = new_stats(Cout, B, H, W, dev) if st else None
    z0 = fwd_pre(ops.split_pack_act(xd, f16=True), qf, Cout, stats=cm0)
    z1 = fwd_pre(ops.split_pack_act(xd, f16=True, slots=so), qf, Cout, stats=cm1, slots=so)
    assert torch.equal(z0, z1)
    assert not st or torch.equal(cm0, cm1)


def concat_operand(parts, sc, dev, pm=1):
    """the decoder's two-producer concat buffer: channels < sc from `parts[0]`, the rest from `parts[1]`, each pre-split by its own
    producer with its own slots (guard rule) -> (buffer, slots of the first group, slots of the second)"""
    from onet_amd import ops
    a, b = parts
    B, _, H, W = a.shape
    C = a.shape[1] + b.shape[1]
    P = torch.empty((B, C // 8, H, 2, W, 8), dtype=torch.float16, device=dev)
    s1, s2 = ops.absmax_slots(a), ops.absmax_slots(b)
    ops.split_pack_act(a, f16=True, slots=s1, out=P[:, :sc // 8])
    ops.split_pack_act(b, f16=True, slots=s2, out=P[:, sc // 8:])
    return P, s1, s2


@pytest.mark.parametrize("B,Cin,Cout,H,W,sc,st", [(2, 96, 40, 20, 48, 32, False), (2, 128, 64, 32, 64, 64, True),
                                                  (4, 192, 64, 16, 16, 96, True), (2, 128, 72, 16, 32, 64, False)])
def test_forward_two_producer_concat(dev, B, Cin, Cout, H, W, sc, st):
    """A concat buffer with two producers (skip half at ~1e5: guard exponent set; up-sampled half at ~1e-1: exponent 0; and the
    reverse), each half scaled by its own slots: the forward undoes each half with its own slots (x_amax below split_ch, x_amax2
    above).  The large half would hide an error in the small one at the output's scale, so each half is run alone -- the other
    half's weights zeroed -- and held to fp64 at its own scale; the statistics records of each run to the fp64 statistics."""
    from onet_amd import ops
    w = rnd(Cout, Cin, 3, 3, seed=152, scale=(2.0 / (Cin * 9)) ** 0.5)
    for big_first in (True, False):
        a = rnd(B, sc, H, W, seed=150) * (1e5 if big_first else 1e-1)
        b = rnd(B, Cin - sc, H, W, seed=151) * (1e-1 if big_first else 1e5)
        P, s1, s2 = concat_operand((a.to(dev), b.to(dev)), sc, dev)
        for half in (0, 1):
            wh = w.clone()
            if half == 0:
                wh[:, sc:] = 0
            else:
                wh[:, :sc] = 0
            qf, _ = packs(wh.to(dev), 1)
            z64 = conv64(torch.cat([a, b], 1).double(), wh.double())
            cm = new_stats(Cout, B, H, W, dev) if st else None
            z = fwd_pre(P, qf, Cout, stats=cm, slots=s1, slots2=s2, split_ch=sc)
            what = f"concat forward {(B, Cin, Cout, H, W, sc)}, {'large' if big_first == (half == 0) else 'small'} half {half}"
            close(z, z64, tol_conv(1, Cin), what)
            if st:
                check_stats(cm, z64, what)


@pytest.mark.parametrize("B,Cin,Cout,H,W,sc", [(2, 128, 72, 19, 80, 64), (2, 256, 128, 16, 64, 128), (4, 128, 128, 16, 32, 64),
                                               (4, 192, 64, 16, 16, 64)])
def test_wgrad_two_producer_concat(dev, B, Cin, Cout, H, W, sc):
    """conv3x3_wgrad_pre16_kernel on the slots: x a two-producer concat buffer (x_slots below split_ch, x_slots2 above, the guard
    rule) and dz scaled by the `always` rule from dz_slots.  dw's rows of input channels below and above split_ch are each held to
    fp64 at their own scale; and a single-slot-set x (split_ch = 0) beyond fp16's range."""
    from onet_amd import ops
    g = rnd(B, Cout, H, W, seed=162, scale=1e-4)
    gP, kw = grad_operand(g.to(dev), 1)
    for big_first in (True, False):
        a = rnd(B, sc, H, W, seed=160) * (1e5 if big_first else 1e-1)
        b = rnd(B, Cin - sc, H, W, seed=161) * (1e-1 if big_first else 1e5)
        P, s1, s2 = concat_operand((a.to(dev), b.to(dev)), sc, dev)
        dw64 = wgrad64(torch.cat([a, b], 1).double(), g.double(), (Cout, Cin, 3, 3))
        dw = ops.conv3x3_split_wgrad_pre(P, gP, (Cout, Cin, 3, 3), out=torch.full((Cout, Cin, 3, 3), float("nan"), device=dev),
                                         x_slots=s1, x_slots2=s2, split_ch=sc, dz_slots=kw["slots"])
        what = f"concat wgrad {(B, Cin, Cout, H, W, sc)}"
        close(dw[:, :sc], dw64[:, :sc], TOL_WGRAD[1], what + f" channels < {sc}")
        close(dw[:, sc:], dw64[:, sc:], TOL_WGRAD[1], what + f" channels >= {sc}")
    x = rnd(B, Cin, H, W, seed=163) * 3e5
    xd = x.to(dev)
    sl = ops.absmax_slots(xd)
    dw64 = wgrad64(x.double(), g.double(), (Cout, Cin, 3, 3))
    dw = ops.conv3x3_split_wgrad_pre(ops.split_pack_act(xd, f16=True, slots=sl), gP, (Cout, Cin, 3, 3), x_slots=sl,
                                     dz_slots=kw["slots"])
    close(dw, dw64, TOL_WGRAD[1], f"guarded wgrad {(B, Cin, Cout, H, W)}")


# ---------------------------------------------------------------------------------------------------------------- fuzz
MAC_BUDGET = 4e8            # per fp64 reference convolution (CPU time)


def _draw_fwd(rng, i):
    pm = i % 3
    while True:
        mult = 32 if pm == 2 else 16
        Cin = mult * int(rng.integers(1, 512 // mult + 1)) if rng.random() < 0.5 else mult * int(rng.integers(1, 128 // mult + 1))
        # any Cout; half of them a whole number of the input gradient's channel chunks (its reduction: Cout)
        Cout = int(rng.integers(1, 321)) if rng.random() < 0.5 else mult * int(rng.integers(1, 320 // mult + 1))
        if rng.random() < 0.25:
            W, B, H = 16, 2 * int(rng.integers(1, 4)), 16 * int(rng.integers(1, 5))
        else:
            W, B, H = int(rng.integers(17, 201)), int(rng.integers(1, 7)), int(rng.integers(1, 71))
            if pm == 2 and rng.random() < 0.8:      # (plain bf16: W % 4 == 0; the other widths are refused)
                W = 4 * int(rng.integers(5, 51))
            if rng.random() < 0.3:      # full 16 x 32 tiles: the statistics instances
                W, H = 32 * int(rng.integers(1, 7)), 16 * int(rng.integers(1, 5))
        if B * H * W * Cin * Cout * 9 <= MAC_BUDGET:
            return pm, B, Cin, Cout, H, W


def _draw_wgrad(rng, i):
    pm = i % 3
    while True:
        Cin, Cout = 8 * int(rng.integers(1, 65)), 8 * int(rng.integers(1, 41))
        if rng.random() < 0.2:
            Cout = 128 * int(rng.integers(1, 3))
        u = rng.random()
        if u < 0.2:
            W, B = 16, 4 * int(rng.integers(1, 3))
        elif u < 0.4:
            W, B = 32, 2 * int(rng.integers(1, 4))
        else:
            W, B = int(rng.integers(64, 201)), int(rng.integers(1, 7))
        H = int(rng.integers(1, 71))
        if B * H * W * Cin * Cout * 9 <= MAC_BUDGET:
            return pm, B, Cin, Cout, H, W


def _splitk(lib, B, Cin, Cout, H, W):
    """split-K factor the weight-gradient plan picks on this device (from the workspace it asks for)"""
    slabs = 1 if (Cout % 128 == 0 and W >= 32) else 2
    return int(lib.onet_conv3x3_split_wgrad_ws_bytes(B, Cin, Cout, H, W)) // (slabs * 9 * Cout * Cin * 4)


def test_presplit_entries_fuzz(dev):
    """Seeded shapes from each entry's own ONET_REQUIRE domain (not from what the model sends): Cin a multiple of 16 (32 for plain
    bf16) up to 512, any Cout, W = 16 (even B, H % 16 == 0) or W in 17 .. 200, H in 1 .. 70, B in 1 .. 6, all three operand forms.
    Forward without and -- where onet_conv3x3_split_pre_nparts > 0 -- with statistics, the input-gradient orientation, the weight
    gradient where onet_conv3x3_split_wgrad_pre_ok says yes, all against fp64; where a predicate says no, the entry refuses.  Plain
    bf16 operands need W % 4 == 0 (conv3x3_pre16_kernel stores 4-pixel vectors): other widths are refused by the entry."""
    from onet_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(20261016))
    seen = {"stats": 0, "refused_stats": 0, "dgrad": 0, "wgrad": 0, "refused_wgrad": 0, "refused_w4": 0}
    for i in range(30):
        pm, B, Cin, Cout, H, W = _draw_fwd(rng, i)
        tag = f"{PM_NAMES[pm]} {(B, Cin, Cout, H, W)}"
        x = rnd(B, Cin, H, W, seed=170 + i)
        w = rnd(Cout, Cin, 3, 3, seed=171 + i, scale=(2.0 / (Cin * 9)) ** 0.5)
        qf, qd = packs(w.to(dev), pm)
        xP = act(x.to(dev), pm)
        nparts = int(lib.onet_conv3x3_split_pre_nparts(B, H, W))
        if pm == 2 and W % 4:
            with pytest.raises(_lib.OnetHipError):
                fwd_pre(xP, qf, Cout)
            seen["refused_w4"] += 1
            continue
        z64 = conv64(ref_op(x, pm), ref_op(w, pm))
        close(fwd_pre(xP, qf, Cout), z64, tol_conv(pm, Cin), "fuzz forward " + tag)
        if nparts > 0:
            cm = new_stats(Cout, B, H, W, dev)
            close(fwd_pre(xP, qf, Cout, stats=cm), z64, tol_conv(pm, Cin), "fuzz forward with statistics " + tag)
            check_stats(cm, z64, "fuzz " + tag)
            seen["stats"] += 1
        else:
            with pytest.raises(_lib.OnetHipError):
                fwd_pre(xP, qf, Cout, stats=torch.empty((Cout, 1, 3), device=dev))
            seen["refused_stats"] += 1
        g = rnd(B, Cout, H, W, seed=172 + i, scale=1e-3)
        if Cout % (32 if pm == 2 else 16) == 0:
            gP, kw = grad_operand(g.to(dev), pm)
            dx = ops.conv3x3_split_pre(gP, qd, Cin, out=nan_out(B, Cin, H, W, dev), **kw)
            close(dx, dgrad64(ref_op(g, pm), ref_op(w, pm)), tol_conv(pm, Cout), "fuzz input gradient " + tag)
            seen["dgrad"] += 1
        if Cout % 8 == 0:
            if lib.onet_conv3x3_split_wgrad_pre_ok(B, Cin, Cout, H, W):
                close(wgrad_pre(x.to(dev), g.to(dev), pm), wgrad64(ref_op(x, pm), ref_op(g, pm), (Cout, Cin, 3, 3)), TOL_WGRAD[pm],
                      "fuzz wgrad " + tag)
                seen["wgrad"] += 1
            else:
                with pytest.raises(_lib.OnetHipError):
                    ops.conv3x3_split_wgrad_pre(xP, act(g.to(dev), pm), (Cout, Cin, 3, 3))
                seen["refused_wgrad"] += 1
    splitk = set()
    for i in range(30):
        pm, B, Cin, Cout, H, W = _draw_wgrad(rng, i)
        tag = f"{PM_NAMES[pm]} {(B, Cin, Cout, H, W)}"
        assert lib.onet_conv3x3_split_wgrad_pre_ok(B, Cin, Cout, H, W), tag
        splitk.add(_splitk(lib, B, Cin, Cout, H, W) > 1)
        x = rnd(B, Cin, H, W, seed=180 + i)
        g = rnd(B, Cout, H, W, seed=181 + i, scale=1e-3)
        close(wgrad_pre(x.to(dev), g.to(dev), pm), wgrad64(ref_op(x, pm), ref_op(g, pm), (Cout, Cin, 3, 3)), TOL_WGRAD[pm],
              "fuzz wgrad " + tag)
    # the weight-gradient entry refuses what its predicate refuses: widths 17 .. 63 other than 32, odd batches at 32, B % 4 at 16
    for B, C, H, W in ((2, 64, 8, 48), (3, 64, 8, 32), (2, 64, 16, 16)):
        assert not lib.onet_conv3x3_split_wgrad_pre_ok(B, C, C, H, W)
        t = act(torch.zeros(B, C, H, W, device=dev), 1)
        with pytest.raises(_lib.OnetHipError):
            ops.conv3x3_split_wgrad_pre(t, t, (C, C, 3, 3))
    assert splitk == {True, False}, "the fuzz must cover split-K > 1 and split-K == 1"
    assert all(v > 0 for k, v in seen.items() if k != "refused_w4"), seen
