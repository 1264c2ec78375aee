"""CPU tests of tests/conv_refs.py: the fp64 references against PyTorch's float64 operators, the Winograd restatement against the
direct form, the float32 emulations against the bounds the GPU tests use (test_gpu_fp32_conv_kernels.py), and planted defects that
the per-element bound must see -- one of which the old 2e-4 max-norm does not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_refs as cr

T = torch.from_numpy


def t64(a):
    return T(np.asarray(a, np.float64))


def ratio(got, ref, mag):
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.maximum(cr.U * mag, 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("ks", [1, 3])
def test_fp64_references_equal_torch(ks):
    B, Cin, Cout, H, W = 3, 5, 7, 9, 11
    x, w, dz = cr.graded(B, Cin, H, W, 1), cr.weights(Cout, Cin, ks, 2), cr.gaussian(B, Cout, H, W, 3)
    xt, wt = t64(x).requires_grad_(True), t64(w).requires_grad_(True)
    z = F.conv2d(xt, wt, None, 1, ks // 2)
    z.backward(t64(dz))
    for got, ref in ((cr.conv_fwd(x, w)[0], z.detach()), (cr.conv_dgrad(dz, w)[0], xt.grad), (cr.conv_wgrad(x, dz, ks)[0], wt.grad),
                     (cr.conv_wgrad(x, dz, ks)[0], torch.nn.grad.conv2d_weight(t64(x), w.shape, t64(dz), padding=ks // 2))):
        assert np.abs(got - ref.numpy()).max() <= 1e-12 * np.abs(ref.numpy()).max()
    mag = F.conv2d(t64(np.abs(x)), t64(np.abs(w)), None, 1, ks // 2).numpy()
    assert np.abs(cr.conv_fwd(x, w)[1] - mag).max() <= 1e-12 * mag.max()
    prior = cr.gaussian(1, Cout, Cin, ks * ks, 4).reshape(Cout, Cin, ks, ks)
    dw, m = cr.conv_wgrad(x, dz, ks, prior)
    assert np.allclose(dw, wt.grad.numpy() + prior, rtol=1e-12, atol=0) and (m >= np.abs(prior)).all()


def test_twin_batch_is_the_complement_in_float32():
    x = np.clip(cr.gaussian(2, 1, 5, 7, 5), -0.5, 1.5)
    t = cr.twin_batch(x, 0.25)
    assert t.dtype == np.float32 and np.array_equal(t[:2], x)
    assert np.array_equal(t[2:], torch.clamp((1 - T(x)) + 0.25, 0, 1).numpy())


@pytest.mark.parametrize("shape", [(2, 5, 6, 9, 11), (1, 3, 4, 16, 32), (3, 4, 2, 3, 5)])
def test_winograd_restatement_equals_the_direct_form(shape):
    """proves the matrices G, B^T, A^T and the structure of the magnitude formula"""
    B, Cin, Cout, H, W = shape
    x, w = cr.graded(B, Cin, H, W, 6), cr.weights(Cout, Cin, 3, 7)
    z, mag = cr.conv_fwd(x, w)
    zw, magw = cr.wino4_fwd(x, w)
    assert np.abs(zw - z).max() <= 1e-12 * np.abs(z).max()
    assert (magw >= np.abs(z) * (1 - 1e-12)).all() and (magw >= mag * (1 - 1e-12)).all()    # |sum| <= sum |.|, term by term
    Uw = cr.wino4_pack(w)
    assert np.allclose(Uw[:, :, 0, 0], np.asarray(w, np.float64)[:, :, 0, 0] / 16) and np.allclose(Uw[:, :, 5, 5], w[:, :, 2, 2])


def test_pack_index_maps():
    w = np.arange(5 * 3 * 9, dtype=np.float32).reshape(5, 3, 3, 3)
    wf, wd = cr.pack3x3_fwd(w), cr.pack3x3_dgrad(w)
    for co, ci, t in ((0, 0, 0), (4, 2, 8), (3, 1, 5)):
        assert wf[(ci * 9 + t) * 5 + co] == w[co, ci, t // 3, t % 3] == wd[(co * 9 + 8 - t) * 3 + ci]
    # a forward convolution with the input-gradient pack read as [Cin_out][Cout_in] weights is the input gradient
    assert np.array_equal(cr.pack3x3_dgrad(w), cr.pack3x3_fwd(cr.dgrad_weights(w)))
    wt = np.arange(3 * 5 * 4, dtype=np.float32).reshape(3, 5, 2, 2)
    f, d, q = cr.packT2x2(wt)
    assert f[2 * 20 + 3 * 5 + 4] == wt[2, 4, 1, 1] == d[(3 * 5 + 4) * 3 + 2] == q[2 * 20 + 4 * 4 + 3]
    P = cr.wino4_pack_layout(np.arange(70 * 2 * 36, dtype=np.float64).reshape(70, 2, 6, 6), fwd=True)
    assert P.shape == (2, 36, 128)
    for co in (0, 1, 16, 17, 63, 64, 69):        # channel 16 g + i of a 64-block at float 4 i + g
        blk, g, i = co // 64, (co % 64) // 16, co % 16
        assert P[1, 7, 64 * blk + 4 * i + g] == (co * 2 + 1) * 36 + 7
    assert np.count_nonzero(P[:, :, 64:]) == 2 * 36 * 6


def test_restated_plans_match_the_library():
    from onet_amd import _lib
    lib = _lib.load()
    for prop, shape, ks, lay in cr.DW_SHAPES:
        cr.check_dw_property(prop, shape, ks, lay)
        assert int(lib.onet_conv_wgrad_ws_bytes(*shape, ks)) == cr.wgrad_ws_bytes(*shape, ks), shape
    for shape, ks in (((2, 1, 10, 33, 64), 3), ((4, 3, 64, 32, 260), 3), ((7, 640, 192, 33, 70), 3), ((1, 2048, 2048, 8, 8), 3), ((9, 8, 8, 300, 300), 1)):
        assert int(lib.onet_conv_wgrad_ws_bytes(*shape, ks)) == cr.wgrad_ws_bytes(*shape, ks), shape
    for prop, shape in cr.FWD_SHAPES:
        cr.check_fwd_property(prop, shape)
    for prop, shape in cr.WINO_SHAPES:
        cr.check_wino_property(prop, shape)


def test_dispatch_refuses_an_image_beyond_the_buffer_range():
    """ops.conv3x3_algo used to fall back to "direct" for operands beyond 2 GiB, "because the direct kernel addresses with 64-bit
    pointers": it stages through a 32-bit buffer resource like the others.  Such a shape now raises; between the two ranges (a concat
    buffer of twice the channels would not fit, one image does) the direct kernel still takes it."""
    from onet_amd import ops
    with ops.using(ops.Settings(conv="auto")):
        with pytest.raises(ValueError, match="2 GiB"):
            ops.conv3x3_algo(1, 64, 64, 4096, 4096)            # 80 channels x 64 MiB
        with pytest.raises(ValueError, match="2 GiB"):
            ops.conv3x3_algo(1, 8192, 8192, 8, 8)              # the packed weight
        assert ops.conv3x3_algo(1, 64, 64, 2048, 2048) == "direct"          # (64 + 16) x 16 MiB fits, (2 x 64 + 16) x 16 MiB does not


# ---------------------------------------------------------------------------------------------------------------- emulations size the bounds
def sized(worst, K, what):
    """K is the smallest power of two at or above twice the emulation's worst ratio"""
    print(f"EMUL {what}: worst err / (u mag) {worst:.4f}, K {K}")
    assert K / 4 < worst <= K / 2, (what, worst, K)


def fwd_cases(table, seed):
    """the GPU tests' own operands (same makers, same seeds), whole: an outlier sits in one channel of an image, and a channel subset
    would mostly miss it"""
    for _, (B, Cin, Cout, H, W) in table:
        for maker, name in ((cr.gaussian, "gauss"), (cr.graded, "graded")):
            yield (B, Cin, Cout, H, W), maker(B, Cin, H, W, seed), name


def test_direct_emulation_is_within_half_the_bound():
    """chunked (two-level) accumulation over the GPU test's shapes and operands, 3x3 and 1x1; the plain sequential chain printed as
    the envelope"""
    worst, seq = 0.0, 0.0
    for prop, shape in cr.FWD_SHAPES:
        for name in cr.fwd_inputs(prop):
            for ks in (1, 3):
                x, dz, w = cr.fwd_operands(shape, ks, name)                     # what the GPU test runs, whole
                for src, wt in ((x, w), (dz, cr.dgrad_weights(w))):             # forward; input gradient
                    z, mag = cr.conv_fwd(src, wt)
                    worst = max(worst, ratio(cr.direct_emul(src, wt), z, mag))
                    if src.shape[1] <= 64:
                        seq = max(seq, ratio(cr.direct_emul(src, wt, fold=False), z, mag))
    print(f"EMUL direct sequential envelope (Cin <= 64): {seq:.4f}")
    sized(worst, cr.K_DIRECT, "direct fwd/dgrad")


def test_direct_dw_emulation_is_within_half_the_bound():
    worst = 0.0
    for _, shape, ks, _ in cr.DW_SHAPES:
        B, Cin, Cout, H, W = shape
        for maker, name in ((cr.gaussian, "gauss"), (cr.graded, "graded")):
            x, dz = maker(B, Cin, H, W, 111), cr.gaussian(B, Cout, H, W, 112)[:, :8]     # the GPU test's x, whole; a SUBSET of its dz and prior: 8 of Cout channels (Gaussian, each independent)
            prior = cr.normal(Cout, Cin, ks, ks, seed=113)[:8]
            for pr in (None, prior):
                dw, mag = cr.conv_wgrad(x, dz, ks, pr)
                worst = max(worst, ratio(cr.direct_dw_emul_full(x, dz, ks, shape, pr), dw, mag))
    sized(worst, cr.K_DIRECT_DW, "direct dW")


def test_winograd_emulation_is_within_half_the_bound():
    worst, worst_gauss, worst_direct, worst_pack = 0.0, 0.0, 0.0, 0.0
    for shape, x, name in fwd_cases(cr.WINO_SHAPES, 131):
        B, Cin, Cout, H, W = shape
        w = cr.weights(Cout, Cin, 3, 133)
        dz = dict(gauss=cr.gaussian, graded=cr.graded)[name](B, Cout, H, W, 132)
        for src, wt in ((x, w), (dz, cr.dgrad_weights(w))):                 # forward; input gradient
            z, mag = cr.wino4_fwd(src, wt)
            got = cr.wino4_emul(src, wt)
            worst = max(worst, ratio(got, z, mag))
            if name == "gauss":
                worst_gauss = max(worst_gauss, ratio(got, z, mag))
                worst_direct = max(worst_direct, ratio(got, z, cr.conv_fwd(src, wt)[1]))
    for Cout, Cin in cr.WINO_PACK_SHAPES:
        w = cr.graded(Cout, Cin, 3, 3, 123)
        for wt in (w, w[:, :, ::-1, ::-1]):
            worst_pack = max(worst_pack, ratio(cr.wino4_pack(wt, lambda v: cr.r32(v).astype(np.float64)), cr.wino4_pack(wt), cr.wino4_pack(wt, absval=True)))
    print(f"EMUL F(4x4), Gaussian data alone: {worst_gauss:.4f} of u mag = {worst_direct:.2f} of u conv(|x|, |w|); on the graded data an output whose "
          "own receptive field is all zeros still carries the rounding of its tile: the magnitude is per tile")
    sized(worst, cr.K_WINO4, "F(4x4,3x3) fwd/dgrad")
    sized(worst_pack, cr.K_WINO4_PACK, "F(4x4,3x3) pack")


def test_winograd_wgrad_restatement_and_emulation():
    """F(3x3,4x4): the fp64 restatement equals the direct weight gradient (G', B^T, A'^T, the tile order of wide maps and of image pairs);
    the restated plan equals the library's; the float32 emulation sizes K"""
    from onet_amd import _lib
    lib = _lib.load()
    worst = 0.0
    for prop, shape in cr.W4W_SHAPES:
        cr.check_w4w_property(prop, shape)
        B, Cin, Cout, H, W = shape
        assert int(lib.onet_conv3x3_winograd4_wgrad_ok(*shape)) == 1
        assert int(lib.onet_conv3x3_winograd4_wgrad_ws_bytes(*shape)) == cr.wino4w_ws_bytes(*shape)
        for maker in (cr.gaussian, cr.graded):
            x, dz, prior = maker(B, Cin, H, W, 151), cr.gaussian(B, Cout, H, W, 152), cr.normal(Cout, Cin, 3, 3, seed=153)   # the GPU test's operands
            ref = cr.conv_wgrad(x, dz, 3)[0]
            for pr in (None, prior):
                dw, mag = cr.wino4w_wgrad(x, dz, pr)
                assert np.abs(dw - (ref if pr is None else ref + pr)).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
                worst = max(worst, ratio(cr.wino4w_emul(x, dz, shape, pr), dw, mag))
    sized(worst, cr.K_WINO4W, "F(3x3,4x4) dW")


def test_bn_on_load_reference_is_the_batchnorm_relu_backward():
    """bn_case's dz against autograd of relu(batch_norm(z)) in float64, per statistics group (to the float32 rounding of the saved
    statistics and coefficients)"""
    B, C, H, W, G = 4, 5, 6, 7, 2
    z, da = cr.gaussian(B, C, H, W, 41), cr.gaussian(B, C, H, W, 42)
    save, coef, dz = cr.bn_case(z, da, G, 43)
    gamma, beta = 1 + 0.1 * cr.normal(C, seed=43).astype(np.float64), 0.1 * cr.normal(C, seed=44).astype(np.float64)
    for g in range(G):
        s = slice(2 * g, 2 * g + 2)
        zt = t64(z[s]).requires_grad_(True)
        torch.relu(F.batch_norm(zt, None, None, t64(gamma), t64(beta), True, 0.0, 1e-5)).backward(t64(da[s]))
        assert np.abs(dz[s] - zt.grad.numpy()).max() <= 1e-5 * np.abs(zt.grad.numpy()).max()
    assert cr.bn_case(z, da, G, 43, train=False)[1] is None


def test_stem_dw_emulation_is_within_half_the_bound():
    cr.check_stem_shapes()
    worst = 0.0
    for B, Cin, Cout, H, W in cr.STEM_SHAPES:
        x = cr.twin_batch(np.clip(cr.graded(B // 2, Cin, H, W, 141), -0.5, 1.5), 0.25)                   # the GPU test's operands
        z, da = cr.gaussian(B, Cout, H, W, 142), cr.gaussian(B, Cout, H, W, 143)
        prior = cr.normal(Cout, Cin, 3, 3, seed=144)
        for dz in (da, cr.bn_case(z, da, 2, 145)[2]):          # plain: dz given; on load: dz in fp64 from (da, z), rounded once by the kernel
            for pr in (None, prior):
                dw, mag = cr.conv_wgrad(x, dz, 3, pr)
                worst = max(worst, ratio(cr.stem_dw_emul(x, dz, pr), dw, mag))
    sized(worst, cr.K_STEM_DW, "stem dW")


# ---------------------------------------------------------------------------------------------------------------- planted defects
def test_bound_sees_the_lost_two_level_fold():
    """(a) on the "fold" rows of the GPU test's own table -- its operands of one sign at Cin = 1024 and 4096, 3x3 forward -- the single
    sequential chain of 9 Cin terms leaves the bound that the folded accumulation keeps with room: a conv_fwd_kernel without its
    second accumulator set fails test_direct_fwd_dgrad[fold-*-3].  At Cin = 1024 the margin is thin (K is set by the 2^8 outlier of the
    graded rows), at 4096 it is more than twofold.  On the signed rows neither form comes near: those rows cannot see this defect."""
    rows = [shape for prop, shape in cr.FWD_SHAPES if prop == "fold"]
    assert [s[1] for s in rows] == [1024, 4096]
    for shape, factor in zip(rows, (1.0, 2.0)):
        assert cr.fwd_inputs("fold") == ("onesign",)
        x, _, w = cr.fwd_operands(shape, 3, "onesign")
        z, mag = cr.conv_fwd(x, w)
        with_fold, without = ratio(cr.direct_emul(x, w), z, mag), ratio(cr.direct_emul(x, w, fold=False), z, mag)
        print(f"DEFECT (a) no fold, {shape}: {without:.1f} of u mag without, {with_fold:.2f} with, K {cr.K_DIRECT}")
        assert with_fold <= cr.K_DIRECT / 4 and without > factor * cr.K_DIRECT
    x, _, w = cr.fwd_operands(rows[0], 3, "gauss")
    z, mag = cr.conv_fwd(x, w)
    assert ratio(cr.direct_emul(x, w, fold=False), z, mag) < cr.K_DIRECT / 8


def test_bound_sees_one_winograd_position_in_bf16():
    """(b) the transformed weights of one of the 36 positions rounded to bf16"""
    x, w = cr.gaussian(1, 16, 16, 32, 23), cr.weights(8, 16, 3, 24)
    z, mag = cr.wino4_fwd(x, w)

    def bf16(Uw):
        Uw = Uw.copy()
        Uw[:, :, 2, 3] = T(Uw[:, :, 2, 3].astype(np.float32)).to(torch.bfloat16).double().numpy()
        return Uw
    r = ratio(cr.wino4_emul(x, w, defect=bf16), z, mag)
    print(f"DEFECT (b) one position bf16: {r:.1f} of u mag, K {cr.K_WINO4}")
    assert (np.abs(cr.wino4_emul(x, w, defect=bf16) - z) > cr.bound(cr.K_WINO4, mag)).mean() > 0.5


def test_bound_sees_operands_cut_to_ten_mantissa_bits():
    """(c) the 'xf32' mistake: operands truncated to a 10-bit mantissa"""
    x, w = cr.gaussian(1, 9, 5, 17, 25), cr.weights(8, 9, 3, 26)
    z, mag = cr.conv_fwd(x, w)
    assert (np.abs(cr.direct_emul(x, w, trunc=10) - z) > cr.bound(cr.K_DIRECT, mag)).mean() > 0.9


def test_bound_sees_a_halo_element_the_old_max_norm_does_not():
    """(d) at the top border one tap reads the row inside the image instead of zero, at a column where the graded input is about 2^-12
    of its typical value: far outside the per-element bound, far inside 2e-4 of the output scale -- the reason for these tests"""
    B, Cin, Cout, H, W = 1, 9, 8, 5, 17
    x, w = cr.graded(B, Cin, H, W, 27), cr.weights(Cout, Cin, 3, 28)
    col = 0                                                        # row 0, columns 0 and 1 lie in a non-zero square of the checkerboard
    assert (x[0, :, 0, col] != 0).all() and np.abs(x[0, :, 0, col]).max() < 2.0 ** -8 and np.abs(x).max() == 256.0
    z, mag = cr.conv_fwd(x, w)
    bad = cr.direct_emul(x, w, halo=(0, 0, col, 0, 1))             # tap (ky 0, kx 1) of output pixel (0, col) lies in row -1
    err = np.abs(bad - z)
    assert np.unravel_index(err.argmax(), err.shape)[2:] == (0, col)
    r = float((err / cr.bound(cr.K_DIRECT, mag)).max())
    old = float(err.max() / (2e-4 * np.abs(z).max()))
    print(f"DEFECT (d) halo: {r:.0f} x the per-element bound, {old:.3f} x the 2e-4 max-norm")
    assert r > 100 and old < 0.5
    assert (np.abs(cr.direct_emul(x, w) - z) <= cr.bound(cr.K_DIRECT / 2, mag)).all()
