"""The ConvTranspose2d(k=2, s=2) GEMMs of onet_amd/csrc/convt_gemm.hip, instance by instance, against fp64 at their edges.

The decoder's up-sampling runs on two kernel families: the fp32-input 128 x 128 GEMMs (forward with the pixel-shuffle epilogue, input
gradient, split-K weight gradient; operand precision PREC 0 fp32 MFMA, 1 bf16-rounded operands, 2 split bf16 operands) and the
slot-operand kernels (both operands pre-split: NP = 2 fp16 (hi | mid), NP = 1 plain bf16).  Every instance launched from the end of
convt_gemm.hip runs here on one well-formed shape and on the edge shapes of its entry's predicate, against
torch.nn.functional.conv_transpose2d and autograd in fp64 on the CPU.  The references are computed once per shape (ref64) and shared.

    instance                                 entry (ops wrapper)                        tests
    convt_gemm_kernel<0, 0 | 1 | 2>          onet_convT2x2_fwd (convT2x2_fwd)            test_f32in_forward[f32 | bf16 | split-*], test_dispatch_seams
                                             onet_convT2x2_fwd_p (convT2x2_fwd_p)        test_f32in_forward_presplit_epilogue
    convt_gemm_kernel<1, 0 | 1 | 2>          onet_convT2x2_dgrad_dbias (convT2x2_dgrad)  test_f32in_dgrad[f32 | bf16 | split-*]
    convt_wgrad_gemm_kernel<0 | 1 | 2>       onet_convT2x2_wgrad (convT2x2_wgrad)        test_f32in_wgrad[f32 | bf16 | split-*], test_dispatch_seams
    convt_slot_fwd_kernel<2 | 1>             onet_convT2x2_fwd_slots                     test_slot_forward[fp16x2 | plain-*], test_slot_strided_operands,
                                                                                         test_slot_guard_scales, test_predicates_agree
    convt_slot_dgrad_kernel<2 | 1>           onet_convT2x2_dgrad_slots                   test_slot_backward[fp16x2 | plain-*], test_slot_strided_operands,
                                                                                         test_slot_guard_scales, test_predicates_agree
    convt_slot_wgrad_kernel<2 | 1, BIG = 0>  onet_convT2x2_wgrad_slots                   test_slot_backward[*-(.., 128, ..) and (.., 256, 96, ..)]
    convt_slot_wgrad_kernel<2 | 1, BIG = 1>                                              test_slot_backward[*-(.., 256, 128 | 64, ..)]
    convt_pack_slots_kernel                  onet_convT2x2_pack_weights_slots            test_slot_weight_packs (bit for bit), every slot test
    convt_absmax_kernel                      ... (launched for the fp16 pack only)       test_slot_weight_packs[fp16x2]
    convt_out_bound_kernel                   onet_convT2x2_out_bound                     test_out_bound_per_channel, test_slot_guard_scales
    convt_wgrad_reduce_kernel                both weight-gradient entries                test_f32in_wgrad, test_slot_backward (splitK 1, 3 and 5)
    convt_dbias_reduce_kernel                dgrad_dbias and wgrad_slots entries         test_f32in_dgrad, test_slot_backward

Every compiled instance is reachable.  PREC is selected as the model does: ops.using(ops.Settings(conv=..., split=...)) with
ops.CONVT_SPLIT_MIN_BLOCKS = 0; each fp32-input test shows that its instance ran by the bits of its result differing from another
PREC's.  The slot entries pick NP from the operands' type and BIG from wgrad_slots_plan, which the tests restate (plan_slots) and
check against the workspace size the library reports.

Shapes (B, Cin, Ct, h, w) and the property each one is here for -- asserted from the plan arithmetic in check_property, so that a
change of the tiling un-tests nothing silently:

    grid1      1, 128,  32,  8,  16   smallest slot forward: one M tile, one block
    chunks     2, 160,  32,  8,  16   10 (fp16) / 5 (bf16) K chunks through the two-stage ring (forward only: the backward kernels need
                                      Cin % 128 == 0)
    mtiles3    3, 128,  96,  8,  16   three M tiles, 9 blocks (not a multiple of 8: the remainder branch of xcd_block_id), Ct != Cin / 2
    midrow     2, 128,  64, 32,  12   128-pixel tiles start and end inside rows (the slot weight gradient needs a power-of-two w: refused)
    rows64     1, 128,  32, 64,   2   a tile is 64 rows; lower edge of the slot weight gradient's shifts
    onerow     2, 128,  32,  1, 128   a tile is one row, h = 1; upper edge of those shifts
    notbig     2, 256,  96,  8,  16   slot weight gradient: the 128 x 128 configuration at Cin % 256 == 0
    big        1, 256,  64,  8,  16   slot weight gradient: the 256 x 256 configuration, smallest
    cin48      2,  48,  32,  8,  16   fp32-input forward with Cin < 128 (three K chunks)
    ct160      2, 128, 160,  8,  16   Ct > 64: convt_out_bound_kernel folds channels into slot co & 63
    splitk     split-K with a shorter last split and a split that starts in one image and ends in another, B odd.  No B in {3, 5} with
               a map of the rows above gives one: wgrad_plan and wgrad_slots_plan allow a split per 16 chunks of 32 pixels, and then
               k divides the chunk count (36 / 2, 60 / 3) or k = 1.  Nearest shapes that do: B = 7 on the 32 x 12 map for wgrad_plan
               (84 chunks, 5 splits of 17), B = 13 on the 8 x 16 map for wgrad_slots_plan in both configurations (52 chunks, 3 splits
               of 18), the latter also with the in-launch bias gradient.
The fp32-input weight-gradient ENTRY requires Ct % 64 == 0 (onet_convT2x2_wgrad), so its edge shapes take Ct = 64 (192 for several
N tiles with Ct != Cin / 2) where the rows above say 32 (96); the fp32-input input gradient takes Ct % 8 == 0 and runs them as listed.

Tolerances are those the tests of test_gpu_ops.py already hold these kernels to (named below with their provenance); the worst
error / tolerance per instance measured with this file is recorded in profiles/r13_convt_fp64.md."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# of the output scale (max |reference|), as the existing tests:
TOL_SLOT_FWD = 2e-6          # test_convT_slot_operands, fp16 (hi | mid)
TOL_SLOT_BWD = 4e-6          # test_convT_backward_slot_operands (both gradients, both operand forms; the bias gradient against
                             # the largest per-channel sum of |dy|)
TOL_SPLIT = 2e-5             # test_up_convT_cat_split_operands
TOL_BF16 = 1e-5              # test_up_convT_cat_bf16_operands, against the bf16-ROUNDED operands
TOL_BF16_DBIAS = 1e-4        # ... its bias gradient (summed from the unrounded fp32 rows, by the same code under every PREC)
TOL_PLAIN_OUT = 2.0 ** -8    # test_convT_slot_operands, plain bf16: one rounding of the output
TOL_F32 = 2e-4               # the `close` default of test_gpu_ops.py
TOL_F32_DW = 3e-4            # test_up_convT_cat: dW and dbias

NP_NAMES = {2: "fp16x2", 1: "plain"}
PREC_NAMES = {0: "f32", 1: "bf16", 2: "split"}
C2 = 16                      # skip channels of the concat buffers the outputs (and dy) are slices of


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
    """max |a - b| <= tol * max |b| (b: the fp64 reference); every element of a finite"""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert bool(torch.isfinite(a).all()), what + ": not finite"
    scale = float(b.abs().max()) + 1e-300
    err = float((a - b).abs().max())
    print(f"RATIO {what}: err/tol {err / (tol * scale):.3f}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


# ---------------------------------------------------------------------------------------------------------------- references
_REF = {}


def ref64(shape, rounded=False):
    """Operands (fp32, seeded by the shape) and the fp64 ConvTranspose2d results of the (rounded: bf16-rounded) operands, computed
    once per shape and shared: x (post-ReLU, as the producer writes it), w, bias, dy; y, dx, dw, db (db: of the unrounded dy too)."""
    key = (tuple(shape), bool(rounded))
    if key not in _REF:
        B, Cin, Ct, h, w = shape
        x = torch.relu(rnd(B, Cin, h, w, seed=301))
        wt, bias = rnd(Cin, Ct, 2, 2, seed=302, scale=0.05), rnd(Ct, seed=303)
        dy = rnd(B, Ct, 2 * h, 2 * w, seed=304, scale=3e-5)
        rb = (lambda t: t.to(torch.bfloat16).double()) if rounded else (lambda t: t.double())
        xr, wr = rb(x).requires_grad_(True), rb(wt).requires_grad_(True)
        y = F.conv_transpose2d(xr, wr, bias.double(), stride=2)
        (y * rb(dy)).sum().backward()
        _REF[key] = dict(x=x, w=wt, bias=bias, dy=dy, y=y.detach(), dx=xr.grad, dw=wr.grad, db=rb(dy).sum((0, 2, 3)),
                         db_f32rows=dy.double().sum((0, 2, 3)), db_l1=rb(dy).abs().sum((0, 2, 3)))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------- plans
def plan_f32(B, Cin, Ct, h, w):
    """wgrad_plan of convt_gemm.hip -> (splitK, chunks per split, chunks); a chunk is 32 pixels"""
    chunks = B * h * w // 32
    tiles = (Cin // 128) * (Ct // 32)
    k = max(1, -(-512 // tiles))
    k = min(k, max(1, chunks // 16))
    k = min(k, max(1, (256 << 20) // (Cin * 4 * Ct * 4)))
    per = -(-chunks // k)
    return -(-chunks // per), per, chunks


def plan_slots(B, Cin, Ct, h, w):
    """wgrad_slots_plan -> (big, splitK, chunks per split, chunks)"""
    big = Cin % 256 == 0 and Ct % 64 == 0
    chunks = B * h * w // 32
    tiles = (Cin // 256) * (Ct // 64) if big else (Cin // 128) * (Ct // 32)
    k = max(1, -(-(256 if big else 512) // tiles))
    k = min(k, max(1, chunks // 16))
    k = min(k, max(1, (256 << 20) // (Cin * 4 * Ct * 4)))
    per = -(-chunks // k)
    return big, -(-chunks // per), per, chunks


def slots_ws_bytes(shape):
    from onet_amd import _lib
    return int(_lib.load().onet_convT2x2_wgrad_slots_ws_bytes(*shape))


def check_split_edges(splitK, per, chunks, B, hw, what):
    """the last split is shorter, and a split starts in one image and ends in another, with B odd"""
    assert B % 2 == 1 and splitK > 1 and splitK * per != chunks and (splitK - 1) * per < chunks, (what, splitK, per, chunks)
    cpi = hw // 32
    assert any((k * per) // cpi != (min((k + 1) * per, chunks) - 1) // cpi and (k * per) % cpi for k in range(1, splitK)), what


def check_property(prop, shape, family):
    """the reason a shape is in a table, from the kernels' own arithmetic; family: "slot_fwd", "slot_bwd", "f32_fwd", "f32_dgrad", "f32_wgrad" """
    B, Cin, Ct, h, w = shape
    hw = h * w
    assert hw % 128 == 0 or (prop == "hw32" and hw % 32 == 0), shape
    if family in ("slot_fwd", "f32_fwd"):
        grid = (4 * Ct // 128) * (B * hw // 128)
    elif family in ("slot_bwd", "f32_dgrad"):
        grid = (Cin // 128) * (B * hw // 128)
    else:
        grid = plan_f32(*shape)[0] * (Cin // 128) * (Ct // 32)
    if prop == "well":
        assert Ct == Cin // 2 and w & (w - 1) == 0 and 8 <= w <= 64
    elif prop == "grid1":
        assert grid == 1 and (family not in ("slot_fwd", "f32_fwd") or 4 * Ct == 128)
    elif prop == "chunks":
        n16, n32 = Cin // 16, Cin // 32
        assert n16 & (n16 - 1) and n32 & (n32 - 1) and n32 % 2 == 1
    elif prop == "mtiles3":
        assert Ct != Cin // 2 and grid % 8 != 0
        assert {"slot_fwd": 4 * Ct // 128, "f32_fwd": 4 * Ct // 128, "slot_bwd": Ct // 32, "f32_dgrad": B * hw // 128,
                "f32_wgrad": Ct // 32}[family] >= 3
    elif prop == "midrow":
        assert 128 % w != 0 and w & (w - 1) != 0 and w % 2 == 0
    elif prop == "rows64":
        assert w == 2 and 128 // w == 64
    elif prop == "onerow":
        assert h == 1 and w == 128
    elif prop == "notbig":
        assert Cin % 256 == 0 and not plan_slots(*shape)[0]
    elif prop == "big":
        assert plan_slots(*shape)[0] and (Cin // 256) * (Ct // 64) == 1
    elif prop == "cin48":
        assert Cin < 128 and Cin % 16 == 0 and Cin % 32 != 0
    elif prop == "ct160":
        assert Ct > 64 and Ct % 64 != 0
    elif prop == "k32":
        assert 4 * Ct == 32          # two K chunks of the fp32-input input gradient
    elif prop == "hw32":
        assert hw == 32              # the fp32-input weight gradient takes maps of 32 k pixels
    elif prop.startswith("splitk"):
        if family == "f32_wgrad":
            k, per, chunks = plan_f32(*shape)
        else:
            big, k, per, chunks = plan_slots(*shape)
            assert big == (prop == "splitk-big") and (prop != "splitk-notbig" or Cin % 256 == 0)
        check_split_edges(k, per, chunks, B, hw, shape)
    else:
        raise AssertionError(prop)


def ids(rows):
    return ["%s-%s" % (p, "x".join(map(str, s))) for p, s in rows]


# ---------------------------------------------------------------------------------------------------------------- slot operands
def nchw(P):
    v = P.float().sum(3) if P.shape[3] == 2 else P[:, :, :, 0].float()
    return v.permute(0, 1, 4, 2, 3).reshape(P.shape[0], P.shape[1] * 8, P.shape[2], P.shape[4])


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def guard_k(slots):
    """the exponent the forward guard rule reads from magnitude slots: 2^k scales the tensor when its bound reaches 2^15"""
    bound = float(slots.view(torch.float32).max())
    e = math.floor(math.log2(bound))
    return 13 - e if e >= 15 else 0


def slice_of_wider(t, fill=1.0e4):
    """t as the upper channel groups of a buffer with twice the groups, the other half `fill`: the batch stride is twice the contiguous one"""
    wide = torch.full((t.shape[0], 2 * t.shape[1]) + tuple(t.shape[2:]), fill, dtype=t.dtype, device=t.device)
    wide[:, t.shape[1]:] = t
    return wide[:, t.shape[1]:]


def slot_forward(dev, shape, parts, gain=1.0, strided=False):
    """-> (y as fp64 NCHW on the CPU with the output guard scale undone, the pre-split output bits, k of the output guard)"""
    from onet_amd import ops
    B, Cin, Ct, h, w = shape
    r = ref64(shape, rounded=parts == 1)
    xd = (r["x"] * gain).to(dev)
    x_slots = ops.absmax_slots(xd) if parts == 2 else None
    xP = ops.split_pack_act(xd, f16=True, parts=parts, slots=x_slots)
    if strided:
        xP = slice_of_wider(xP)
    wP = ops.packT2x2_slots(r["w"].to(dev), parts)
    y_slots = ops.convT2x2_out_bound(r["w"].to(dev), r["bias"].to(dev), x_slots) if parts == 2 else None
    cat = torch.full((B, (C2 + Ct) // 8, 2 * h, parts, 2 * w, 8), float("nan"), dtype=xP.dtype, device=dev)
    cat[:, :C2 // 8] = 1234.0
    skip = bits(cat[:, :C2 // 8]).clone()
    assert ops.convT2x2_fwd_slots(xP, wP, r["bias"].to(dev), cat[:, C2 // 8:], Ct, x_slots=x_slots, slots=y_slots)
    assert torch.equal(bits(cat[:, :C2 // 8]), skip), "the skip groups of the concat buffer changed"
    k = guard_k(y_slots) if parts == 2 else 0
    return nchw(cat[:, C2 // 8:]).double().cpu() * 2.0 ** -k, bits(cat[:, C2 // 8:]), k


def check_slot_forward(got, shape, parts, what, gain=1.0):
    ref = ref64(shape, rounded=parts == 1)["y"]
    if gain != 1.0:            # (the guard case only, fp16 parts: x * gain is exact, so is the reference of the scaled input)
        r = ref64(shape)
        ref = F.conv_transpose2d((r["x"] * gain).double(), r["w"].double(), r["bias"].double(), stride=2)
    close(got, ref, TOL_SLOT_FWD if parts == 2 else TOL_PLAIN_OUT, what)


SLOT_FWD = [("well", (2, 256, 128, 16, 16)), ("grid1", (1, 128, 32, 8, 16)), ("chunks", (2, 160, 32, 8, 16)), ("mtiles3", (3, 128, 96, 8, 16)),
            ("midrow", (2, 128, 64, 32, 12)), ("rows64", (1, 128, 32, 64, 2)), ("onerow", (2, 128, 32, 1, 128)), ("ct160", (2, 128, 160, 8, 16))]


@pytest.mark.parametrize("prop,shape", SLOT_FWD, ids=ids(SLOT_FWD))
@pytest.mark.parametrize("parts", [2, 1], ids=lambda p: NP_NAMES[p])
def test_slot_forward(dev, parts, prop, shape):
    """convt_slot_fwd_kernel<NP>: the pre-split output (upper groups of a NaN-filled concat buffer whose skip groups must stay as
    they are) against fp64 -- fp16 (hi | mid): the unrounded operands, 2e-6; plain bf16: the rounded operands, one output rounding.
    The two instances must differ in their bits."""
    from onet_amd import ops
    check_property(prop, shape, "slot_fwd")
    with ops.using(ops.Settings(conv="auto", split=True)):
        assert ops.convt_slots_ok(*shape, parts=parts)
    got, _, k = slot_forward(dev, shape, parts)
    assert k == 0
    check_slot_forward(got, shape, parts, f"slot forward {NP_NAMES[parts]} {shape}")
    other, _, _ = slot_forward(dev, shape, 3 - parts)
    assert not torch.equal(got, other), "fp16 (hi | mid) and plain bf16 gave the same bits: one of them did not run"


def grad_operand(dev, shape, parts):
    """-> (dy pre-split as its producer writes it, its slots): fp16 parts under the `always` rule of a bound 20 x the maximum"""
    from onet_amd import ops
    dy = ref64(shape)["dy"]
    dyd = dy.to(dev)
    if parts == 1:
        return ops.split_pack_act(dyd, parts=1), None
    bound = ops.new_amax(dev)
    bound.view(torch.float32)[::32] = 20.0 * float(dy.abs().max())
    k = 13 - math.floor(math.log2(20.0 * float(dy.abs().max())))
    return ops.split_pack_act(dyd, f16=True, scale=2.0 ** k), bound


def dgrad_slots_into(dyP, wdP, Cin, dy_slots):
    """onet_convT2x2_dgrad_slots into the leading channels of a NaN-filled tensor with 8 channels more (ops.convT2x2_dgrad_slots
    allocates its own) -> (return code, dx view, the whole buffer)"""
    from onet_amd import _lib, ops
    B, C8, Ho, parts, Wo, _ = dyP.shape
    h, w = Ho // 2, Wo // 2
    buf = torch.full((B, Cin + 8, h, w), float("nan"), device=dyP.device)
    rc = _lib.load().onet_convT2x2_dgrad_slots(ops._p(dyP), ops._pbs(dyP), ops._p(dy_slots), ops._p(wdP), ops._p(buf), (Cin + 8) * h * w, parts,
                                               B, Cin, C8 * 8, h, w, ops._stream())
    assert rc >= 0, _lib.last_error()
    return rc, buf[:, :Cin], buf


def wgrad_slots_into(xP, dyP, shape, x_slots, dy_slots):
    """ops.convT2x2_wgrad_slots with the bias gradient, into NaN-filled tensors with a sentinel tail -> (dw, db) | None"""
    from onet_amd import ops
    B, Cin, Ct, h, w = shape
    dwb = torch.full((Cin + 1, Ct, 2, 2), float("nan"), device=xP.device)
    dbb = torch.full((Ct + 4,), float("nan"), device=xP.device)
    got = ops.convT2x2_wgrad_slots(xP, dyP, (Cin, Ct, 2, 2), x_slots=x_slots, dy_slots=dy_slots, want_dbias=True, out=dwb[:Cin], db_out=dbb[:Ct])
    assert bool(torch.isnan(dwb[Cin:]).all()) and bool(torch.isnan(dbb[Ct:]).all()), "the weight gradient wrote past its tensors"
    return got


def slot_backward(dev, shape, parts, strided=False, want_wgrad=True):
    from onet_amd import ops
    B, Cin, Ct, h, w = shape
    r = ref64(shape, rounded=parts == 1)
    dyP, bound = grad_operand(dev, shape, parts)
    xP = ops.split_pack_act(r["x"].to(dev), f16=True, parts=parts)
    if strided:
        dyP, xP = slice_of_wider(dyP), slice_of_wider(xP)
    rc, dx, buf = dgrad_slots_into(dyP, ops.packT2x2_slots(r["w"].to(dev), parts, dgrad=True)[1], Cin, bound)
    assert rc == 0, "the slot input gradient refused the shape"
    assert bool(torch.isnan(buf[:, Cin:]).all()), "the input gradient wrote past its channels"
    got = wgrad_slots_into(xP, dyP, shape, None, bound) if want_wgrad else None
    return dx, got


SLOT_BWD = [("well", (2, 256, 128, 16, 16)), ("grid1", (1, 128, 32, 8, 16)), ("mtiles3", (3, 128, 96, 8, 16)), ("midrow", (2, 128, 64, 32, 12)),
            ("rows64", (1, 128, 32, 64, 2)), ("onerow", (2, 128, 32, 1, 128)), ("notbig", (2, 256, 96, 8, 16)), ("big", (1, 256, 64, 8, 16)),
            ("splitk", (13, 128, 32, 8, 16)), ("splitk-notbig", (13, 256, 96, 8, 16)), ("splitk-big", (13, 256, 64, 8, 16))]


@pytest.mark.parametrize("prop,shape", SLOT_BWD, ids=ids(SLOT_BWD))
@pytest.mark.parametrize("parts", [2, 1], ids=lambda p: NP_NAMES[p])
def test_slot_backward(dev, parts, prop, shape):
    """convt_slot_dgrad_kernel<NP>, convt_slot_wgrad_kernel<NP, BIG> and the two reduce kernels: dx, dW and the in-launch bias
    gradient, written into NaN-filled tensors, against fp64 (4e-6; plain bf16: of the bf16-rounded operands).  The tile configuration
    and split-K the test states are the ones the library's workspace size implies."""
    B, Cin, Ct, h, w = shape
    check_property(prop, shape, "slot_bwd")
    pow2 = w & (w - 1) == 0
    big, k, per, chunks = plan_slots(*shape)
    assert slots_ws_bytes(shape) == (k * (Cin * 4 * Ct + 4 * Ct) * 4 if pow2 else 0), "plan_slots is not the library's plan any more"
    r = ref64(shape, rounded=parts == 1)
    dx, got = slot_backward(dev, shape, parts)
    what = f"{NP_NAMES[parts]} {shape}"
    close(dx, r["dx"], TOL_SLOT_BWD, "slot input gradient " + what)
    if not pow2:
        assert got is None, "the slot weight gradient takes power-of-two widths only"
        return
    assert got is not None
    close(got[0], r["dw"], TOL_SLOT_BWD, f"slot weight gradient (big {int(big)}, splitK {k}) " + what)
    assert bool(torch.isfinite(got[1]).all())
    err = float((got[1].double().cpu() - r["db"]).abs().max())
    print(f"RATIO slot bias gradient {what}: err/tol {err / (TOL_SLOT_BWD * float(r['db_l1'].max())):.3f}")
    assert err <= TOL_SLOT_BWD * float(r["db_l1"].max()), "bias gradient " + what
    if parts == 2:
        dx1, got1 = slot_backward(dev, shape, 1)
        assert not torch.equal(dx, dx1) and not torch.equal(got[0], got1[0]), "fp16 (hi | mid) and plain bf16 gave the same bits"


@pytest.mark.parametrize("parts", [2, 1], ids=lambda p: NP_NAMES[p])
def test_slot_strided_operands(dev, parts):
    """xP and dyP as channel-group slices of buffers with twice the groups (the other half 1e4: a read through the contiguous stride
    breaks the tolerance without an inf), as training passes them: bit-identical to the contiguous run -- forward on the odd chunk
    count, the gradients on three images (the weight gradient advances from image to image inside its K loop)."""
    fshape, bshape = (2, 160, 32, 8, 16), (3, 128, 96, 8, 16)
    got, raw, _ = slot_forward(dev, fshape, parts)
    got_s, raw_s, _ = slot_forward(dev, fshape, parts, strided=True)
    check_slot_forward(got_s, fshape, parts, f"strided slot forward {NP_NAMES[parts]}")
    assert torch.equal(raw, raw_s), "forward: strided xP"
    r = ref64(bshape, rounded=parts == 1)
    dx, (dw, db) = slot_backward(dev, bshape, parts)
    dx_s, (dw_s, db_s) = slot_backward(dev, bshape, parts, strided=True)
    close(dx_s, r["dx"], TOL_SLOT_BWD, "strided slot input gradient")
    close(dw_s, r["dw"], TOL_SLOT_BWD, "strided slot weight gradient")
    assert torch.equal(bits(dx), bits(dx_s)), "input gradient: strided dyP"
    assert torch.equal(bits(dw), bits(dw_s)) and torch.equal(bits(db), bits(db_s)), "weight gradient: strided xP / dyP"


def test_slot_guard_scales(dev):
    """Guard scales on the shape whose tiles start inside rows: an input gain of 3e4 (max |x| and max |y| beyond fp16's range: x is
    written under its guard scale, y needs one) for the forward, and -- on the 64-row shape, the slot weight gradient needing a
    power-of-two width -- for the weight gradient's x; the gradients' dy under the loose `always` bound (20 x its maximum), as in
    every test_slot_backward case."""
    from onet_amd import ops
    shape, gain = (2, 128, 64, 32, 12), 3.0e4
    got, _, k = slot_forward(dev, shape, 2, gain=gain)
    assert k < 0, "this case is meant to need the output guard scale"
    check_slot_forward(got, shape, 2, "slot forward under guard scales", gain=gain)
    dx, _ = slot_backward(dev, shape, 2, want_wgrad=False)
    close(dx, ref64(shape)["dx"], TOL_SLOT_BWD, "slot input gradient, loose `always` bound")
    wshape = (1, 128, 32, 64, 2)
    r = ref64(wshape)
    xd = (r["x"] * gain).to(dev)
    x_slots = ops.absmax_slots(xd)
    assert guard_k(x_slots) < 0
    dyP, bound = grad_operand(dev, wshape, 2)
    got = wgrad_slots_into(ops.split_pack_act(xd, f16=True, slots=x_slots), dyP, wshape, x_slots, bound)
    w0 = torch.zeros(128, 32, 2, 2, dtype=torch.float64, requires_grad=True)
    (F.conv_transpose2d((r["x"] * gain).double(), w0, None, stride=2) * r["dy"].double()).sum().backward()
    close(got[0], w0.grad, TOL_SLOT_BWD, "slot weight gradient, x under its guard scale")


@pytest.mark.parametrize("parts", [2, 1], ids=lambda p: NP_NAMES[p])
def test_slot_weight_packs(dev, parts):
    """convt_pack_slots_kernel (and, fp16, convt_absmax_kernel), bit for bit: wP [Cin/8][parts][4 Ct][8] with column 4 c + sub-pixel,
    wdP [(Ct/8) 4][parts][Cin][8] with K-slot 4 c8 + sub-pixel; fp16: parts of 2^k w with max |2^k w| in [2^13, 2^14), (2^k, 2^-k)
    behind the pack."""
    from onet_amd import ops
    Cin, Ct = 160, 96
    w = rnd(Cin, Ct, 2, 2, seed=311, scale=0.05)
    wP, wdP = ops.packT2x2_slots(w.to(dev), parts, dgrad=True)
    n = Cin * 4 * Ct
    fwd = w.view(Cin // 8, 8, 4 * Ct).permute(0, 2, 1)                         # [c8][m][kc]
    bwd = w.view(Cin, Ct // 8, 8, 4).permute(1, 3, 0, 2).reshape(Ct // 2, Cin, 8)    # [c8 * 4 + q][ci][kc]
    for P, v in ((wP, fwd), (wdP, bwd)):
        if parts == 1:
            want = v.to(torch.bfloat16).reshape(-1)
        else:
            k = 13 - math.floor(math.log2(float(w.abs().max())))
            vs = v * 2.0 ** k
            hi = vs.to(torch.float16)
            want = torch.stack([hi, (vs - hi.float()).to(torch.float16)], 1).reshape(-1)
            meta = P[n * 2:].cpu().view(torch.float32)
            assert meta.tolist() == [2.0 ** k, 2.0 ** -k]
        assert torch.equal(bits(P[:n * parts].cpu()), bits(want)), "pack"


@pytest.mark.parametrize("Cin,Ct", [(128, 160), (256, 96), (128, 32)])
def test_out_bound_per_channel(dev, Cin, Ct):
    """convt_out_bound_kernel: channel co's bound lands in slot co & 63 -- it must cover max |y[:, co]| of the fp64 output for EVERY
    channel (Ct > 64: two or three channels per slot), and the largest slot must not exceed the fp64 L1 bound by more than 1e-4 (the
    kernel's own 1.00001 and an fp32 sum of up to 1024 terms)."""
    from onet_amd import ops
    shape = (2, Cin, Ct, 8, 16)
    r = ref64(shape)
    for bias in (r["bias"], None):
        y = r["y"] if bias is not None else r["y"] - r["bias"].double().view(1, -1, 1, 1)
        x_slots = ops.absmax_slots(r["x"].to(dev))
        slots = ops.convT2x2_out_bound(r["w"].to(dev), None if bias is None else bias.to(dev), x_slots)
        got = slots.view(torch.float32)[::32].cpu().double()
        assert got.numel() == 64 and bool(torch.isfinite(got).all())
        ymax = y.abs().amax((0, 2, 3))
        l1 = r["w"].double().abs().sum(0).amax((1, 2)) * float(r["x"].abs().max()) + (0.0 if bias is None else bias.double().abs())
        for co in range(Ct):
            assert float(got[co & 63]) >= float(ymax[co]), f"channel {co}: slot {co & 63} holds {float(got[co & 63])}, max |y| {float(ymax[co])}"
        assert float(got.max()) <= float(l1.max()) * (1 + 1e-4)
        assert float(got.max()) >= float(l1.max()) * (1 - 1e-4)      # ... nor fall short of it: it is a bound


# ---------------------------------------------------------------------------------------------------------------- fp32 input
def prec_settings(prec):
    from onet_amd import ops
    return {0: ops.Settings(conv="auto", split=False), 1: ops.Settings(conv="bf16"), 2: ops.Settings(conv="auto", split=True)}[prec]


def with_prec(monkeypatch, prec, fn, B, h, w, Ct):
    """fn() under the settings that select PREC, as the model does; the dispatch must really say `prec`"""
    from onet_amd import ops
    monkeypatch.setattr(ops, "CONVT_SPLIT_MIN_BLOCKS", 0)
    with ops.using(prec_settings(prec)):
        assert ops.convt_operand_bf16(B, h, w, Ct) == prec
        return fn()


def tol_prec(prec, what="y"):
    if what == "db":
        return {0: TOL_F32_DW, 1: TOL_BF16_DBIAS, 2: TOL_BF16_DBIAS}[prec]
    return {0: TOL_F32_DW if what == "dw" else TOL_F32, 1: TOL_BF16, 2: TOL_SPLIT}[prec]


def f32_forward(dev, shape):
    from onet_amd import ops
    B, Cin, Ct, h, w = shape
    r = ref64(shape)
    cat = torch.full((B, C2 + Ct, 2 * h, 2 * w), float("nan"), device=dev)
    cat[:, :C2] = 1234.0
    ops.convT2x2_fwd(r["x"].to(dev), ops.packT2x2_fused(r["w"].to(dev)), r["bias"].to(dev), cat[:, C2:], Ct, 0, 0)
    assert bool((cat[:, :C2] == 1234.0).all()), "the skip half of the concat buffer changed"
    return cat[:, C2:].cpu()


F32_FWD = [("well", (2, 128, 64, 16, 16)), ("grid1", (1, 128, 32, 8, 16)), ("chunks", (2, 160, 32, 8, 16)), ("mtiles3", (3, 128, 96, 8, 16)),
           ("midrow", (2, 128, 64, 32, 12)), ("rows64", (1, 128, 32, 64, 2)), ("onerow", (2, 128, 32, 1, 128)), ("cin48", (2, 48, 32, 8, 16))]


@pytest.mark.parametrize("prop,shape", F32_FWD, ids=ids(F32_FWD))
@pytest.mark.parametrize("prec", [0, 1, 2], ids=lambda p: PREC_NAMES[p])
def test_f32in_forward(dev, prec, prop, shape, monkeypatch):
    """convt_gemm_kernel<0, PREC> writing the upper half of a NaN-filled concat buffer."""
    B, Cin, Ct, h, w = shape
    check_property(prop, shape, "f32_fwd")
    assert Cin % 16 == 0 and Ct % 32 == 0 and (h * w) % 128 == 0 and w % 2 == 0          # convt_gemm_fwd's predicate
    got = with_prec(monkeypatch, prec, lambda: f32_forward(dev, shape), B, h, w, Ct)
    close(got, ref64(shape, rounded=prec == 1)["y"], tol_prec(prec), f"forward {PREC_NAMES[prec]} {shape}")
    other = with_prec(monkeypatch, 0 if prec else 2, lambda: f32_forward(dev, shape), B, h, w, Ct)
    assert not torch.equal(got, other), f"PREC {prec} did not run: the bits are those of PREC {0 if prec else 2}"


@pytest.mark.parametrize("parts", [2, 1], ids=lambda p: NP_NAMES[p])
def test_f32in_forward_presplit_epilogue(dev, parts, monkeypatch):
    """convt_gemm_kernel<0, *> with the pre-split destination (out16_split 1: fp16 (hi | mid), 2: plain bf16) on the shape whose tiles
    start inside rows: bit-identical to splitting the fp32 output, skip groups untouched."""
    from onet_amd import ops
    shape = (2, 128, 64, 32, 12)
    B, Cin, Ct, h, w = shape
    r = ref64(shape)

    def run():
        cat = torch.full((B, (C2 + Ct) // 8, 2 * h, parts, 2 * w, 8), float("nan"), dtype=torch.float16 if parts == 2 else torch.bfloat16, device=dev)
        cat[:, :C2 // 8] = 1234.0
        skip = bits(cat[:, :C2 // 8]).clone()
        assert ops.convT2x2_fwd_p(r["x"].to(dev), ops.packT2x2_fused(r["w"].to(dev)), r["bias"].to(dev), cat[:, C2 // 8:], Ct, 0, 0)
        assert torch.equal(bits(cat[:, :C2 // 8]), skip)
        return cat[:, C2 // 8:]

    for prec in (0, 2):
        got = with_prec(monkeypatch, prec, run, B, h, w, Ct)
        y = with_prec(monkeypatch, prec, lambda: f32_forward(dev, shape), B, h, w, Ct)
        assert torch.equal(bits(got), bits(ops.split_pack_act(y.to(dev), f16=True, parts=parts))), PREC_NAMES[prec]


def dy_window(dev, shape):
    """dy as the upper half of a concat gradient whose skip half holds 1e4"""
    B, Cin, Ct, h, w = shape
    dcat = torch.full((B, C2 + Ct, 2 * h, 2 * w), 1.0e4, device=dev)
    dcat[:, C2:] = ref64(shape)["dy"].to(dev)
    return dcat[:, C2:]


def f32_dgrad(dev, shape):
    from onet_amd import ops
    B, Cin, Ct, h, w = shape
    dbb = torch.full((Ct + 4,), float("nan"), device=dev)
    dx, db = ops.convT2x2_dgrad(dy_window(dev, shape), ops.packT2x2(ref64(shape)["w"].to(dev))[1], Cin, h, w, 0, 0, want_dbias=True, db_out=dbb[:Ct])
    assert db is not None, "the 128 x 128 input-gradient GEMM (with the bias gradient) refused the shape"
    assert bool(torch.isnan(dbb[Ct:]).all())
    return dx.cpu(), db.cpu()


F32_DGRAD = [("well", (2, 128, 64, 16, 16)), ("grid1", (1, 128, 32, 8, 16)), ("mtiles3", (3, 128, 96, 8, 16)), ("midrow", (2, 128, 64, 32, 12)),
             ("rows64", (1, 128, 32, 64, 2)), ("onerow", (2, 128, 32, 1, 128)), ("k32", (2, 128, 8, 8, 16))]


@pytest.mark.parametrize("prop,shape", F32_DGRAD, ids=ids(F32_DGRAD))
@pytest.mark.parametrize("prec", [0, 1, 2], ids=lambda p: PREC_NAMES[p])
def test_f32in_dgrad(dev, prec, prop, shape, monkeypatch):
    """convt_gemm_kernel<1, PREC> with the bias gradient from the staged rows (convt_dbias_reduce_kernel), dy a strided window whose
    other half holds 1e4 (ops.convT2x2_dgrad allocates dx itself: only the bias gradient goes into a NaN-filled tensor)."""
    B, Cin, Ct, h, w = shape
    check_property(prop, shape, "f32_dgrad")
    assert Cin % 128 == 0 and Ct % 4 == 0 and (h * w) % 128 == 0 and w % 2 == 0          # convt_gemm_dgrad's predicate
    r = ref64(shape, rounded=prec == 1)
    dx, db = with_prec(monkeypatch, prec, lambda: f32_dgrad(dev, shape), B, h, w, Ct)
    what = f"{PREC_NAMES[prec]} {shape}"
    close(dx, r["dx"], tol_prec(prec), "input gradient " + what)
    close(db, r["db_f32rows"], tol_prec(prec, "db"), "bias gradient " + what)
    other = with_prec(monkeypatch, 0 if prec else 2, lambda: f32_dgrad(dev, shape), B, h, w, Ct)
    assert not torch.equal(dx, other[0]), f"PREC {prec} did not run"


def f32_wgrad(dev, shape):
    from onet_amd import ops
    B, Cin, Ct, h, w = shape
    dwb = torch.full((Cin + 1, Ct, 2, 2), float("nan"), device=dev)
    dw, _ = ops.convT2x2_wgrad(ref64(shape)["x"].to(dev), dy_window(dev, shape), (Cin, Ct, 2, 2), 0, 0, False, out=dwb[:Cin])
    assert bool(torch.isnan(dwb[Cin:]).all())
    return dw.cpu()


F32_WGRAD = [("well", (2, 128, 64, 16, 16)), ("mtiles3", (3, 128, 192, 8, 16)), ("midrow", (2, 128, 64, 32, 12)), ("rows64", (1, 128, 64, 64, 2)),
             ("onerow", (2, 128, 64, 1, 128)), ("hw32", (2, 128, 64, 4, 8)), ("splitk", (7, 128, 64, 32, 12))]


@pytest.mark.parametrize("prop,shape", F32_WGRAD, ids=ids(F32_WGRAD))
@pytest.mark.parametrize("prec", [0, 1, 2], ids=lambda p: PREC_NAMES[p])
def test_f32in_wgrad(dev, prec, prop, shape, monkeypatch):
    """convt_wgrad_gemm_kernel<PREC> + convt_wgrad_reduce_kernel, dy a strided window, dW into a NaN-filled tensor."""
    B, Cin, Ct, h, w = shape
    check_property(prop, shape, "f32_wgrad")
    assert Cin % 128 == 0 and Ct % 64 == 0 and (h * w) % 32 == 0 and w % 2 == 0          # onet_convT2x2_wgrad + convt_gemm_wgrad
    got = with_prec(monkeypatch, prec, lambda: f32_wgrad(dev, shape), B, h, w, Ct)
    close(got, ref64(shape, rounded=prec == 1)["dw"], tol_prec(prec, "dw"), f"weight gradient {PREC_NAMES[prec]} {shape} (splitK {plan_f32(*shape)[0]})")
    other = with_prec(monkeypatch, 0 if prec else 2, lambda: f32_wgrad(dev, shape), B, h, w, Ct)
    assert not torch.equal(got, other), f"PREC {prec} did not run"


# ---------------------------------------------------------------------------------------------------------------- dispatch seams
def gemm_takes(Cin, Ct, h, w):
    """which of UpConvTCatFn's three fp32-input passes the 128 x 128 GEMMs take (no F.pad): (forward, input gradient, weight gradient).
    The backward reaches them only where ops.convT2x2_bwd_fusable(Ct) (Ct % 64 == 0); else space-to-depth + the 1 x 1 kernels."""
    hw, even = h * w, w % 2 == 0
    fus = Ct % 64 == 0
    return (Cin % 16 == 0 and Ct % 32 == 0 and hw % 128 == 0 and even,
            fus and Cin % 128 == 0 and Ct % 4 == 0 and hw % 128 == 0 and even,
            fus and Cin % 128 == 0 and Ct % 32 == 0 and hw % 32 == 0 and even)


SEAMS = [((48, 32, 8, 16), (True, False, False)),       # the GEMM forward, the fallback backward
         ((128, 32, 4, 8), (False, False, False)),      # the fallback forward; Ct % 64 != 0 keeps UpConvTCatFn's backward off the GEMMs too
         ((128, 64, 4, 8), (False, False, True))]       # ... with Ct = 64: fallback forward and input gradient, the GEMM weight gradient


@pytest.mark.parametrize("layer,takes", SEAMS, ids=["x".join(map(str, s)) for s, _ in SEAMS])
@pytest.mark.parametrize("prec", [0, 2], ids=lambda p: PREC_NAMES[p])
def test_dispatch_seams(dev, prec, layer, takes, monkeypatch):
    """Fn.UpConvTCatFn forward and backward on layers whose three passes do not all take the same kernel family, under the settings that
    select fp32 MFMA and split operands: out, dx1, dx2, dW, dbias against fp64.  A pass on the 128 x 128 GEMM under split operands is held
    to the split tolerance, every other pass to the fp32 kernels'."""
    from onet_amd import functional as Fn
    from onet_amd import ops
    Cin, Ct, h, w = layer
    B = 2
    assert gemm_takes(*layer) == takes
    r = ref64((B, Cin, Ct, h, w))
    x2, g = rnd(B, C2, 2 * h, 2 * w, seed=321), rnd(B, C2 + Ct, 2 * h, 2 * w, seed=322)
    a, c, d = r["x"].double().requires_grad_(True), r["w"].double().requires_grad_(True), r["bias"].double().requires_grad_(True)
    ref = torch.cat([x2.double(), F.conv_transpose2d(a, c, d, stride=2)], 1)
    ref.backward(g.double())

    def run():
        A, Bt, Cw, Db = [t.to(dev).requires_grad_(True) for t in (r["x"], x2, r["w"], r["bias"])]
        out = Fn.UpConvTCatFn.apply(A, Bt, Cw, Db, (ops.packT2x2_fused(Cw), ops.packT2x2(Cw)[1]))
        out.backward(g.to(dev))
        return out.detach(), A.grad, Bt.grad, Cw.grad, Db.grad

    out, dx1, dx2, dw, db = with_prec(monkeypatch, prec, run, B, h, w, Ct)
    tol = lambda gemm, f32: TOL_SPLIT if (gemm and prec == 2) else f32
    what = f"{PREC_NAMES[prec]} {layer}"
    assert torch.equal(out[:, :C2].cpu(), x2), "the skip half is a copy"
    close(out[:, C2:], ref[:, C2:], tol(takes[0], TOL_F32), "seam out " + what)
    close(dx1, a.grad, tol(takes[1], TOL_F32), "seam dx1 " + what)
    assert torch.equal(dx2.cpu(), g[:, :C2]), "dx2 is a copy"
    close(dw, c.grad, tol(takes[2], TOL_F32_DW), "seam dW " + what)
    close(db, d.grad, TOL_F32_DW, "seam dbias " + what)


# ---------------------------------------------------------------------------------------------------------------- predicates
# every dimension mostly inside the predicates, with the values around their boundaries mixed in: at most half of the draws may be
# refused by all three entries (asserted)
FUZZ_CIN = (128, 160, 192, 256, 384, 512) * 2 + (96, 136)             # Cin % 32, Cin >= 128 (forward), Cin % 128 (gradients); 136: % 8 only
FUZZ_CT = (32, 64, 96, 160) * 3 + (16, 48)                            # Ct % 32
FUZZ_MAP = ((64, 2), (8, 16), (1, 128), (16, 8), (4, 32), (32, 4), (2, 64), (192, 2), (12, 32), (96, 4)) * 2 + \
    ((32, 12), (64, 6), (16, 24), (128, 1), (128, 3), (8, 4), (4, 16), (8, 12))   # h w in {32, 64, 96, 128, 384}; odd, non-power-of-two w


def fuzz_draws():
    rng = np.random.Generator(np.random.PCG64(20261019))
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    return [(int(rng.integers(1, 4)), pick(FUZZ_CIN), pick(FUZZ_CT)) + pick(FUZZ_MAP) + (int(rng.integers(1, 3)),) for _ in range(200)]


def fuzz_predicates(B, Cin, Ct, h, w):
    """(forward, input gradient, weight gradient) as the entries of convt_gemm.hip state them"""
    hw = h * w
    common = Ct % 32 == 0 and hw % 128 == 0
    return (common and Cin % 32 == 0 and Cin >= 128 and w % 2 == 0, common and Cin % 128 == 0 and w % 2 == 0,
            common and Cin % 128 == 0 and w & (w - 1) == 0 and w >= 2)


def test_predicates_agree(dev):
    """200 seeded shapes from a lattice around the predicate boundaries, all inside every entry's ONET_REQUIRE domain (C % 8 == 0,
    positive sizes): ops.convt_slots_ok agrees with ops.convT2x2_fwd_slots, onet_convT2x2_wgrad_slots_ws_bytes > 0 with
    ops.convT2x2_wgrad_slots returning a result, a refusing entry writes nothing.  Operand contents do not matter (constants)."""
    from onet_amd import ops
    draws = fuzz_draws()
    none = sum(not any(fuzz_predicates(*d[:5])) for d in draws)
    assert none <= len(draws) // 2, f"{none} of {len(draws)} draws are refused by every predicate"
    seen = {"fwd": [0, 0], "dgrad": [0, 0], "wgrad": [0, 0]}
    with ops.using(ops.Settings(conv="auto", split=True)):
        assert ops.presplit() and ops.CONVT_SLOTS and ops.CONVT_BF16, "the test needs the default switches"
        for B, Cin, Ct, h, w, parts in draws:
            tag = str((B, Cin, Ct, h, w, parts))
            dt = torch.float16 if parts == 2 else torch.bfloat16
            want = fuzz_predicates(B, Cin, Ct, h, w)
            xP = torch.full((B, Cin // 8, h, parts, w, 8), 0.5, dtype=dt, device=dev)
            dyP = torch.full((B, Ct // 8, 2 * h, parts, 2 * w, 8), 0.5, dtype=dt, device=dev)
            wP = torch.zeros(Cin * 4 * Ct * parts + 4, dtype=dt, device=dev)
            outP = torch.full((B, Ct // 8, 2 * h, parts, 2 * w, 8), float("nan"), dtype=dt, device=dev)
            ok = ops.convT2x2_fwd_slots(xP, wP, None, outP, Ct)
            assert ok == want[0] == ops.convt_slots_ok(B, Cin, Ct, h, w, parts=parts), "forward " + tag
            assert bool(torch.isnan(outP).all()) != ok, "forward: refused but wrote, or accepted and wrote nothing " + tag
            rc, _, buf = dgrad_slots_into(dyP, wP, Cin, None)
            assert (rc == 0) == want[1], "input gradient " + tag
            assert bool(torch.isnan(buf[:, :Cin]).all()) == (rc != 0) and bool(torch.isnan(buf[:, Cin:]).all()), "input gradient wrote " + tag
            need = slots_ws_bytes((B, Cin, Ct, h, w))
            got = wgrad_slots_into(xP, dyP, (B, Cin, Ct, h, w), None, None)
            assert (need > 0) == want[2], "onet_convT2x2_wgrad_slots_ws_bytes " + tag
            assert (got is not None) == (need > 0), "weight gradient: workspace query and entry disagree " + tag
            for k, v in zip(("fwd", "dgrad", "wgrad"), (ok, rc == 0, got is not None)):
                seen[k][int(v)] += 1
    assert all(min(v) >= 20 for v in seen.values()), seen
