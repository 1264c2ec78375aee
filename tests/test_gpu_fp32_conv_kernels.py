"""The fp32 matrix-core convolution kernels, instance by instance, against fp64 PER ELEMENT at their edges.

Every comparison is |got - ref64| <= K u mag per element (tests/conv_refs.py: the references, the magnitudes, and how each K is set from
a float32 emulation on the CPU -- none comes from a GPU figure; tests/test_conv_refs_host.py shows what each bound sees).  The round-1
tests of test_gpu_ops.py hold the same kernels to 2e-4 of the output's max-norm against fp32 CPU results: they stay, these are tighter.

kernel instance                                   entry                                   tests here
conv_fwd_kernel<3,2,2,1,4,32> / <..,16>           onet_conv_fwd ks 3, W > 16 / <= 16      test_direct_fwd_dgrad[*-3] ([fold-*]: the two-level
                                                                                          accumulation), test_range_refusal
conv_fwd_kernel<1,2,2,1,4,32> / <..,16>           onet_conv_fwd ks 1                      test_direct_fwd_dgrad[*-1]
conv_fwd_kernel<1,..,MODE 1 | 2>                  onet_convT2x2_fwd / _dgrad fallbacks    test_gpu_convt_kernels.py::test_dispatch_seams,
                                                                                          test_range_refusal_convT_fallbacks[fwd | dgrad]
conv_wgrad_kernel<3,32> / <3,16> / <1,32> / <1,16> onet_conv_wgrad                        test_direct_wgrad (accumulate 0 | 1; out_layout 1 at ks 1)
conv_wgrad_kernel<1,PW,S2D>                       onet_convT2x2_wgrad fallback            test_gpu_convt_kernels.py::test_dispatch_seams,
                                                                                          test_range_refusal_convT_fallbacks[wgrad]
wgrad_reduce_kernel                               every weight-gradient entry             test_direct_wgrad, test_stem_wgrad
conv3x3_stem_wgrad_kernel<1,4|2,2|3,2|4,1,false>  onet_conv_wgrad, Cin <= 4, ks 3         test_stem_wgrad[plain-*] (accumulate 0 | 1)
conv3x3_stem_wgrad_kernel<.., true>               onet_conv3x3_stem_wgrad_bn              test_stem_wgrad[bn-*] (accumulate 0 | 1, twin batch, groups)
pack3x3_kernel, packT2x2_kernel                   onet_conv3x3_pack_weights,              test_packs_bit_for_bit
                                                  onet_convT2x2_pack_weights(_fused)
pack3x3_wino4_kernel (fwd 1 | 0)                  onet_conv3x3_pack_weights_winograd4     test_winograd4_pack
conv_wino4_kernel<8,0> / <4,0>                    onet_conv3x3_winograd4_fwd, W > 16 / <= 16   test_winograd4_fwd_dgrad
conv_wino4_kernel<8,1>                            onet_conv3x3_winograd4_fwd_stats        test_winograd4_fwd_stats
conv_wino4_kernel<8,2>                            onet_conv3x3_winograd4_dgrad_bnreduce   test_winograd4_dgrad_bnreduce_direct_call
conv_wino4_wgrad_kernel<0> / <1>, wino4w_fold_kernel   onet_conv3x3_winograd4_wgrad       test_winograd4_wgrad (accumulate 0 | 1)
predicates                                        onet_conv3x3_winograd4_wgrad_ok, _nparts, onet_conv3x3_stem_nparts   test_predicates_agree_with_entries

Two environment switches remain inside these files and are read once per process, so no test flips them: ONET_W4W_BLOCKS (the
F(3x3,4x4) block target) and ONET_CONVT_GEMM (0: the ConvTranspose2d GEMMs on the direct kernels).

The harness (every test): operands are views inside NaN-filled buffers -- a channel offset as inside a concat buffer, a batch stride
larger than C H W, guard floats behind; whatever lies outside a result must still be NaN afterwards, and a result must be finite, so a
read past the channel range (the kernels lean on the buffer resource's range check for their zero padding) or a slab that is reduced
before it is written shows.  Workspaces are the test's own, exactly the reported size, NaN-filled, NaN guard behind.  Split-K results
are computed twice and must be bitwise equal."""
import numpy as np
import pytest
import torch

import conv_refs as cr

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from onet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def call(name, *args):
    from onet_amd import _lib
    return _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def host(t):
    return t.detach().cpu().numpy()


def within(got, ref, K, mag, what):
    return cr.within(host(got), ref, cr.bound(K, mag), what, report=print)


class Plane:
    """[B, C, H, W] as channels `before` .. `before + C` of a NaN-filled [B, before + C + after, H, W] buffer with GUARD floats behind"""

    def __init__(self, dev, B, C, H, W, data=None, before=1, after=2, off=0):
        self.n = B * (before + C + after) * H * W
        self.buf = torch.full((off + self.n + GUARD,), NAN, dtype=torch.float32, device=dev)       # off: the base `off` floats past alignment
        self.v = self.buf[off:off + self.n].view(B, before + C + after, H, W)[:, before:before + C]
        self.bs = (before + C + after) * H * W
        self.ptr = self.v.data_ptr()
        if data is not None:
            self.v.copy_(T(data, dev))

    def take(self, what):
        """-> the result; asserts that everything around it is still NaN"""
        got = self.v.clone()
        self.v.fill_(NAN)
        assert bool(torch.isnan(self.buf).all()), what + ": written outside the result"
        return got


class Flat:
    """n floats, NaN-filled (or data), with a NaN guard behind"""

    def __init__(self, dev, n, data=None):
        self.n = n
        self.buf = torch.full((n + GUARD,), NAN, dtype=torch.float32, device=dev)
        self.v = self.buf[:n]
        self.ptr = self.v.data_ptr()
        if data is not None:
            self.v.copy_(T(data, dev).reshape(-1))

    def guard_ok(self, what):
        assert bool(torch.isnan(self.buf[self.n:]).all()), what + ": the guard behind the buffer changed"

    def take(self, what):
        got = self.v.clone()
        self.guard_ok(what)
        return got


_REF = {}


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


INPUTS = (("gauss", cr.gaussian), ("graded", cr.graded))


# ---------------------------------------------------------------------------------------------------------------- direct forward / dgrad
def direct_case(shape, ks, name):
    def make():
        x, dz, w = cr.fwd_operands(shape, ks, name)
        return dict(x=x, dz=dz, w=w, z=cr.conv_fwd(x, w), dx=cr.conv_dgrad(dz, w))
    return cached(("direct", shape, ks, name), make)


@pytest.mark.parametrize("ks", [3, 1])
@pytest.mark.parametrize("prop,shape", cr.FWD_SHAPES, ids=["%s-%s" % (p, "x".join(map(str, s))) for p, s in cr.FWD_SHAPES])
def test_direct_fwd_dgrad(dev, prop, shape, ks):
    """conv_fwd_kernel<KS,2,2,1,4,TW> through onet_conv_fwd, forward (pack [ci][tap][co]) and input gradient (pack [co][8 - tap][ci]);
    3x3 packs by onet_conv3x3_pack_weights, 1x1 packs are the two transposes.  The "fold" rows run operands of one sign at
    Cin = 1024 and 4096: there a kernel without the two-level accumulation leaves the bound (conv_refs.fwd_inputs; the host test
    test_bound_sees_the_lost_two_level_fold shows it on these very operands)."""
    cr.check_fwd_property(prop, shape)
    B, Cin, Cout, H, W = shape
    for name in cr.fwd_inputs(prop):
        r = direct_case(shape, ks, name)
        w = T(r["w"], dev)
        if ks == 3:
            wf, wd = Flat(dev, Cin * 9 * Cout), Flat(dev, Cout * 9 * Cin)
            call("onet_conv3x3_pack_weights", w.data_ptr(), wf.ptr, wd.ptr, Cout, Cin)
            wf.guard_ok("pack"), wd.guard_ok("pack")
        else:
            wf, wd = Flat(dev, Cin * Cout, r["w"].reshape(Cout, Cin).T), Flat(dev, Cin * Cout, r["w"].reshape(Cout, Cin))
        for what, src, pack, Ci, Co, ref in (("fwd", r["x"], wf, Cin, Cout, r["z"]), ("dgrad", r["dz"], wd, Cout, Cin, r["dx"])):
            xin, out = Plane(dev, B, Ci, H, W, src), Plane(dev, B, Co, H, W, before=2, after=1)
            call("onet_conv_fwd", xin.ptr, xin.bs, pack.ptr, out.ptr, out.bs, None, B, Ci, Co, H, W, ks)
            within(out.take(what), ref[0], cr.K_DIRECT, ref[1], f"direct {what} ks{ks} {name} {shape}")


# ---------------------------------------------------------------------------------------------------------------- direct weight gradient
def dw_case(shape, ks, name):
    def make():
        B, Cin, Cout, H, W = shape
        x, dz = dict(INPUTS)[name](B, Cin, H, W, 111), cr.gaussian(B, Cout, H, W, 112)
        prior = cr.normal(Cout, Cin, ks, ks, seed=113)
        return dict(x=x, dz=dz, prior=prior, dw=cr.conv_wgrad(x, dz, ks), dwacc=cr.conv_wgrad(x, dz, ks, prior))
    return cached(("dw", shape, ks, name), make)


def convT_layout(dw, Cout):
    """[co = q Ct + c][ci] (1x1) -> nn.ConvTranspose2d's [ci][c][q]: out_layout 1 of wgrad_reduce_kernel"""
    return np.ascontiguousarray(dw.reshape(4, Cout // 4, -1).transpose(2, 1, 0))


def run_wgrad(dev, entry_args, n_dw, ws_bytes, prior, what):
    """-> dW (flat) of one call with the test's own workspace; prior: the accumulate = 1 operand"""
    ws, dw = Flat(dev, ws_bytes // 4), Flat(dev, n_dw, prior)
    entry_args(dw, ws, 0 if prior is None else 1)
    got = dw.take(what)
    ws.guard_ok(what + " workspace")
    return got


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("prop,shape,ks,lay", cr.DW_SHAPES, ids=["%s-%s-ks%d-lay%d" % (p, "x".join(map(str, s)), k, l) for p, s, k, l in cr.DW_SHAPES])
def test_direct_wgrad(dev, prop, shape, ks, lay, accumulate):
    """conv_wgrad_kernel<KS,PW> + wgrad_reduce_kernel through onet_conv_wgrad: accumulate = 1 against prior + dW with magnitude
    |prior| + mag; out_layout = 1 (the ConvTranspose2d parameter layout of a 1x1 GEMM over 4 Ct sub-pixel channels)"""
    from onet_amd import _lib
    cr.check_dw_property(prop, shape, ks, lay)
    B, Cin, Cout, H, W = shape
    need = int(_lib.load().onet_conv_wgrad_ws_bytes(B, Cin, Cout, H, W, ks))
    assert need == cr.wgrad_ws_bytes(B, Cin, Cout, H, W, ks)
    for name, _ in INPUTS:
        r = dw_case(shape, ks, name)
        x, dz = Plane(dev, B, Cin, H, W, r["x"]), Plane(dev, B, Cout, H, W, r["dz"], before=2, after=1)
        ref, mag = r["dwacc"] if accumulate else r["dw"]
        prior = r["prior"] if accumulate else None
        if lay == 1:          # a permutation of the elements: reference, magnitude and the prior on the device alike
            ref, mag, prior = convT_layout(ref, Cout), convT_layout(mag, Cout), (convT_layout(prior, Cout) if accumulate else None)
        ref, mag = ref.reshape(-1), mag.reshape(-1)

        def entry(dw, ws, acc):
            call("onet_conv_wgrad", x.ptr, x.bs, dz.ptr, dz.bs, dw.ptr, ws.ptr, need, B, Cin, Cout, H, W, ks, lay, acc)
        what = f"direct dW ks{ks} lay{lay} acc{accumulate} {name} {shape}"
        got = run_wgrad(dev, entry, ref.size, need, prior, what)
        within(got, ref, cr.K_DIRECT_DW, mag, what)
        assert torch.equal(got, run_wgrad(dev, entry, ref.size, need, prior, what)), what + ": not reproducible"


# ---------------------------------------------------------------------------------------------------------------- packs
@pytest.mark.parametrize("Cout,Cin", [(5, 3), (64, 72), (100, 1)])
def test_packs_bit_for_bit(dev, Cout, Cin):
    """pack3x3_kernel (either pack alone and both) and packT2x2_kernel (wf, wd, wq) against the numpy index maps"""
    w = cr.normal(Cout, Cin, 3, 3, seed=121)
    wd_ = T(w, dev)
    for want_f, want_d in ((1, 1), (1, 0), (0, 1)):
        f, d = Flat(dev, Cin * 9 * Cout), Flat(dev, Cout * 9 * Cin)
        call("onet_conv3x3_pack_weights", wd_.data_ptr(), f.ptr if want_f else None, d.ptr if want_d else None, Cout, Cin)
        gf, gd = host(f.take("pack3x3 fwd")), host(d.take("pack3x3 dgrad"))
        assert np.array_equal(gf, cr.pack3x3_fwd(w)) if want_f else np.isnan(gf).all()
        assert np.array_equal(gd, cr.pack3x3_dgrad(w)) if want_d else np.isnan(gd).all()
    wt = cr.normal(Cin, Cout, 2, 2, seed=122)                  # nn.ConvTranspose2d: [Cin][Cout][2][2]
    f, d, q = (Flat(dev, Cin * Cout * 4) for _ in range(3))
    call("onet_convT2x2_pack_weights", T(wt, dev).data_ptr(), f.ptr, d.ptr, Cin, Cout)
    call("onet_convT2x2_pack_weights_fused", T(wt, dev).data_ptr(), q.ptr, Cin, Cout)
    for got, ref, what in zip((f, d, q), cr.packT2x2(wt), ("wf", "wd", "wq")):
        assert np.array_equal(host(got.take("packT2x2 " + what)), ref), what


def wino_packs(dev, w):
    """-> (Flat wq_fwd [Cin][36][CoutP], Flat wq_dgrad [Cout][36][CinP]) written by pack3x3_wino4_kernel into NaN-filled buffers"""
    Cout, Cin = w.shape[:2]
    qf, qd = Flat(dev, Cin * 36 * ((Cout + 63) & ~63)), Flat(dev, Cout * 36 * ((Cin + 63) & ~63))
    call("onet_conv3x3_pack_weights_winograd4", T(w, dev).data_ptr(), qf.ptr, qd.ptr, Cout, Cin)
    qf.guard_ok("wino pack"), qd.guard_ok("wino pack")
    return qf, qd


@pytest.mark.parametrize("Cout,Cin", cr.WINO_PACK_SHAPES)
def test_winograd4_pack(dev, Cout, Cin):
    """pack3x3_wino4_kernel: G g G^T within K u |G| |g| |G^T| per element; the padded channels exactly zero (their bound is zero);
    the permutation inside 64-blocks as its comment states (conv_refs.wino4_pack_layout)"""
    w = cr.graded(Cout, Cin, 3, 3, 123)
    qf, qd = wino_packs(dev, w)
    U64, Umag = cr.wino4_pack(w), cr.wino4_pack(w, absval=True)
    within(qf.v, cr.wino4_pack_layout(U64, True).reshape(-1), cr.K_WINO4_PACK, cr.wino4_pack_layout(Umag, True).reshape(-1), f"wino pack fwd {Cout}x{Cin}")
    wflip = w[:, :, ::-1, ::-1]
    within(qd.v, cr.wino4_pack_layout(cr.wino4_pack(wflip), False).reshape(-1), cr.K_WINO4_PACK,
           cr.wino4_pack_layout(cr.wino4_pack(wflip, absval=True), False).reshape(-1), f"wino pack dgrad {Cout}x{Cin}")


# ---------------------------------------------------------------------------------------------------------------- F(4x4, 3x3)
def wino_case(shape, name):
    def make():
        B, Cin, Cout, H, W = shape
        maker = dict(INPUTS)[name]
        x, dz, w = maker(B, Cin, H, W, 131), maker(B, Cout, H, W, 132), cr.weights(Cout, Cin, 3, 133)
        return dict(x=x, dz=dz, w=w, z=cr.wino4_fwd(x, w), dx=cr.wino4_fwd(dz, cr.dgrad_weights(w)))
    return cached(("wino", shape, name), make)


@pytest.mark.parametrize("prop,shape", cr.WINO_SHAPES, ids=["%s-%s" % (p, "x".join(map(str, s))) for p, s in cr.WINO_SHAPES])
def test_winograd4_fwd_dgrad(dev, prop, shape):
    """conv_wino4_kernel<8,0> (W > 16) / <4,0> (W <= 16, image pairs) with both packs of pack3x3_wino4_kernel"""
    cr.check_wino_property(prop, shape)
    B, Cin, Cout, H, W = shape
    for name, _ in INPUTS:
        r = wino_case(shape, name)
        qf, qd = wino_packs(dev, r["w"])
        for what, src, pack, Ci, Co, ref in (("fwd", r["x"], qf, Cin, Cout, r["z"]), ("dgrad", r["dz"], qd, Cout, Cin, r["dx"])):
            xin, out = Plane(dev, B, Ci, H, W, src), Plane(dev, B, Co, H, W, before=2, after=1)
            call("onet_conv3x3_winograd4_fwd", xin.ptr, xin.bs, pack.ptr, out.ptr, out.bs, B, Ci, Co, H, W)
            within(out.take(what), ref[0], cr.K_WINO4, ref[1], f"F(4x4) {what} {name} {shape}")


@pytest.mark.parametrize("shape", [(1, 4, 4, 16, 32), (3, 8, 68, 32, 64)])
def test_winograd4_fwd_stats(dev, shape):
    """conv_wino4_kernel<8,1>: z bit-identical to <8,0> and within the bound; the (n, mean, M2) records merged in fp64 (Chan) against
    the fp64 statistics of the same z by the criteria of test_winograd4_fused_bn_statistics: mean to 2e-6 of std(z), 1 / sqrt(var + eps)
    to 1e-5 relative -- for the whole batch and for the batch slice [B // 2, B)"""
    from onet_amd import _lib
    B, Cin, Cout, H, W = shape
    r = wino_case(shape, "gauss")
    qf, _ = wino_packs(dev, r["w"])
    nparts = int(_lib.load().onet_conv3x3_winograd4_nparts(B, H, W))
    assert nparts == 2 * B * (W // 32) * (H // 16)
    xin = Plane(dev, B, Cin, H, W, r["x"] + np.float32(0.7))
    ref = cached(("wino-stats", shape), lambda: cr.wino4_fwd(r["x"] + np.float32(0.7), r["w"]))
    z0, z1, part = Plane(dev, B, Cout, H, W, before=2, after=1), Plane(dev, B, Cout, H, W, before=2, after=1), Flat(dev, Cout * nparts * 3)
    call("onet_conv3x3_winograd4_fwd", xin.ptr, xin.bs, qf.ptr, z0.ptr, z0.bs, B, Cin, Cout, H, W)
    call("onet_conv3x3_winograd4_fwd_stats", xin.ptr, xin.bs, qf.ptr, z1.ptr, z1.bs, part.ptr, B, Cin, Cout, H, W)
    g0, g1 = z0.take("fwd"), z1.take("fwd_stats")
    assert torch.equal(g0, g1), "z of the statistics kernel differs from the plain kernel's"
    within(g1, ref[0], cr.K_WINO4, ref[1], f"F(4x4) fwd_stats {shape}")
    rec = host(part.take("records")).astype(np.float64).reshape(Cout, nparts, 3)
    assert (rec[:, :, 0] == 256).all()
    z = host(g1).astype(np.float64)
    npi = nparts // B
    for lo in (0, B // 2):
        n, mean, m2 = rec[:, lo * npi:, 0], rec[:, lo * npi:, 1], rec[:, lo * npi:, 2]
        N = n.sum(1)
        mu = (n * mean).sum(1) / N
        var = (m2.sum(1) + (n * (mean - mu[:, None]) ** 2).sum(1)) / N
        zs = z[lo:]
        sd = zs.std()
        assert np.abs(mu - zs.mean((0, 2, 3))).max() <= 2e-6 * sd, "mean"
        ir = 1.0 / np.sqrt(zs.var((0, 2, 3)) + 1e-5)
        assert np.abs((1.0 / np.sqrt(var + 1e-5) - ir) / ir).max() <= 1e-5, "invstd"


# ---------------------------------------------------------------------------------------------------------------- stem weight gradient
TWIN_BIAS = 0.25


def stem_case(shape, G=None, train=True):
    def base():
        B, Cin, Cout, H, W = shape
        xh = np.clip(cr.graded(B // 2, Cin, H, W, 141), -0.5, 1.5)
        return dict(xh=xh, x=cr.twin_batch(xh, TWIN_BIAS), z=cr.gaussian(B, Cout, H, W, 142), da=cr.gaussian(B, Cout, H, W, 143),
                    prior=cr.normal(Cout, Cin, 3, 3, seed=144))
    r = cached(("stem", shape), base)
    if G is None:
        return r, cached(("stem-plain", shape), lambda: (cr.conv_wgrad(r["x"], r["da"], 3), cr.conv_wgrad(r["x"], r["da"], 3, r["prior"])))

    def bn():
        save, coef, dz = cr.bn_case(r["z"], r["da"], G, 145, train)
        return dict(save=save, coef=coef, ref=(cr.conv_wgrad(r["x"], dz, 3), cr.conv_wgrad(r["x"], dz, 3, r["prior"])))
    return r, cached(("stem-bn", shape, G, train), bn)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("shape", cr.STEM_SHAPES, ids=["x".join(map(str, s)) for s in cr.STEM_SHAPES])
def test_stem_wgrad(dev, shape, bn, accumulate):
    """conv3x3_stem_wgrad_kernel<CIN,COG,BN> + wgrad_reduce_kernel.  plain: through onet_conv_wgrad (Cin <= 4, ks 3), the gradient
    planes 16-byte aligned and one float past alignment (`vec` false).  bn: onet_conv3x3_stem_wgrad_bn -- dz formed on load from
    (da, z, save, coef), against the fp64 weight gradient of the fp64 dz of the same float32 statistics; one group (group_images 0)
    and two (B / 2), the twin batch [X ; clip(1 - X + bias, 0, 1)] formed on load from its first half, train and eval coefficients."""
    from onet_amd import _lib
    cr.check_stem_shapes()
    B, Cin, Cout, H, W = shape
    need = int(_lib.load().onet_conv_wgrad_ws_bytes(B, Cin, Cout, H, W, 3))
    assert need == cr.stem_blocks(B, H) * 9 * Cout * Cin * 4
    variants = [(None, False, off, True) for off in (0, 1)] if not bn else \
        [(1, False, 0, True), (2, True, 0, True), (2, True, 1, True), (1, True, 0, False)]
    for G, twin, off, train in variants:
        r, c = stem_case(shape, G, train)
        ref, mag = (c if not bn else c["ref"])[accumulate]
        x = Plane(dev, B // 2, Cin, H, W, r["xh"]) if twin else Plane(dev, B, Cin, H, W, r["x"])
        da = Plane(dev, B, Cout, H, W, r["da"], before=2, after=1, off=off)
        what = f"stem dW bn{int(bn)} G{G} twin{int(twin)} off{off} train{int(train)} acc{accumulate} {shape}"
        if bn:
            z = Plane(dev, B, Cout, H, W, r["z"])
            save, coef = Flat(dev, G * 4 * Cout, c["save"]), (Flat(dev, G * 4 * Cout, c["coef"]) if train else None)

            def entry(dw, ws, acc):
                call("onet_conv3x3_stem_wgrad_bn", x.ptr, x.bs, da.ptr, da.bs, z.ptr, z.bs, save.ptr, coef.ptr if coef else None,
                     0 if G == 1 else B // G, dw.ptr, ws.ptr, need, B, Cin, Cout, H, W, acc, B // 2 if twin else 0, TWIN_BIAS if twin else 0.0)
        else:
            def entry(dw, ws, acc):
                call("onet_conv_wgrad", x.ptr, x.bs, da.ptr, da.bs, dw.ptr, ws.ptr, need, B, Cin, Cout, H, W, 3, 0, acc)
        prior = r["prior"] if accumulate else None
        got = run_wgrad(dev, entry, ref.size, need, prior, what)
        within(got, ref.reshape(-1), cr.K_STEM_DW, mag.reshape(-1), what)
        assert torch.equal(got, run_wgrad(dev, entry, ref.size, need, prior, what)), what + ": not reproducible"


# ---------------------------------------------------------------------------------------------------------------- F(3x3, 4x4) weight gradient
def w4w_case(shape, name):
    def make():
        B, Cin, Cout, H, W = shape
        x, dz = dict(INPUTS)[name](B, Cin, H, W, 151), cr.gaussian(B, Cout, H, W, 152)
        prior = cr.normal(Cout, Cin, 3, 3, seed=153)
        return dict(x=x, dz=dz, prior=prior, ref=(cr.wino4w_wgrad(x, dz), cr.wino4w_wgrad(x, dz, prior)))
    return cached(("w4w", shape, name), make)


def run_w4w(dev, shape, x, dz, prior, what):
    from onet_amd import _lib
    B, Cin, Cout, H, W = shape
    need = int(_lib.load().onet_conv3x3_winograd4_wgrad_ws_bytes(*shape))
    assert need == cr.wino4w_ws_bytes(*shape)
    xin, dzin = Plane(dev, B, Cin, H, W, x), Plane(dev, B, Cout, H, W, dz, before=2, after=1)

    def entry(dw, ws, acc):
        call("onet_conv3x3_winograd4_wgrad", xin.ptr, xin.bs, dzin.ptr, dzin.bs, dw.ptr, ws.ptr, need, B, Cin, Cout, H, W, acc)
    got = run_wgrad(dev, entry, Cout * Cin * 9, need, prior, what)
    assert torch.equal(got, run_wgrad(dev, entry, Cout * Cin * 9, need, prior, what)), what + ": not reproducible"
    return got


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("prop,shape", cr.W4W_SHAPES, ids=["%s-%s" % (p, "x".join(map(str, s))) for p, s in cr.W4W_SHAPES])
def test_winograd4_wgrad(dev, prop, shape, accumulate):
    """conv_wino4_wgrad_kernel<0> (W % 32 == 0) / <1> (W == 16, image pairs) + wino4w_fold_kernel: one unit, split-K dividing the units
    and not, Cout and Cin tile counts, accumulate = 1 against prior + dW"""
    cr.check_w4w_property(prop, shape)
    for name, _ in INPUTS:
        r = w4w_case(shape, name)
        ref, mag = r["ref"][accumulate]
        what = f"F(3x3,4x4) dW acc{accumulate} {name} {shape}"
        within(run_w4w(dev, shape, r["x"], r["dz"], r["prior"] if accumulate else None, what), ref.reshape(-1), cr.K_WINO4W, mag.reshape(-1), what)


# ---------------------------------------------------------------------------------------------------------------- F(4x4) dgrad + BN-backward reduce
@pytest.mark.parametrize("B,Cdz,Cda,H,W,G", [(2, 8, 8, 16, 32, 1), (4, 16, 68, 16, 64, 2), (3, 8, 8, 16, 32, 3)])
def test_winograd4_dgrad_bnreduce_direct_call(dev, B, Cdz, Cda, H, W, G):
    """conv_wino4_kernel<8,2> through onet_conv3x3_winograd4_dgrad_bnreduce itself: da within the F(4x4) bound; the records
    (sum dy, sum dy xhat) per 16 x 16-pixel tile half, summed per statistics group, against the fp64 sums formed from the SAME da and z
    by the criterion of test_dgrad_with_bn_backward_reduce_epilogue (2e-6 of sum |dy|)"""
    from onet_amd import _lib
    shape = (B, Cda, Cdz, H, W)                          # the layer: Cda -> Cdz channels; its input gradient: dz [Cdz] -> da [Cda]
    r = wino_case(shape, "gauss")
    zp = cr.gaussian(B, Cda, H, W, 161) * np.float32(1.5) + np.float32(0.2)
    save, _, _ = cr.bn_case(zp, zp, G, 162)
    nparts = int(_lib.load().onet_conv3x3_winograd4_nparts(B, H, W))
    assert nparts == cr.wino4_nparts(B, H, W) > 0
    _, qd = wino_packs(dev, r["w"])
    dz, z, da = Plane(dev, B, Cdz, H, W, r["dz"]), Plane(dev, B, Cda, H, W, zp), Plane(dev, B, Cda, H, W, before=2, after=1)
    sv, part = Flat(dev, G * 4 * Cda, save), Flat(dev, Cda * nparts * 2)
    call("onet_conv3x3_winograd4_dgrad_bnreduce", dz.ptr, dz.bs, qd.ptr, da.ptr, da.bs, z.ptr, z.bs, sv.ptr, B // G, part.ptr, B, Cdz, Cda, H, W)
    got = da.take("da")
    within(got, r["dx"][0], cr.K_WINO4, r["dx"][1], f"F(4x4) dgrad+bnreduce da {(B, Cdz, Cda, H, W, G)}")
    rec = host(part.take("records")).astype(np.float64).reshape(Cda, G, -1, 2).sum(2)
    da64, Bg = host(got).astype(np.float64), B // G
    for g in range(G):
        s = slice(g * Bg, (g + 1) * Bg)
        mean, inv, sc, sh = (save[g, i].astype(np.float64)[None, :, None, None] for i in range(4))
        zc32 = (zp[s] - save[g, 0][None, :, None, None]).astype(np.float64)         # the kernel's float32 z - mean
        dy = np.where(zc32 * sc + sh > 0, da64[s], 0.0)
        xhat = (zp[s].astype(np.float64) - mean) * inv
        s1, s2, n1 = dy.sum((0, 2, 3)), (dy * xhat).sum((0, 2, 3)), np.abs(dy).sum((0, 2, 3))
        print(f"RATIO bnreduce records G{g}: {np.abs(rec[:, g, 0] - s1).max() / n1.min() / 2e-6:.3f} {np.abs(rec[:, g, 1] - s2).max() / n1.min() / 2e-6:.3f}")
        assert (np.abs(rec[:, g, 0] - s1) / n1).max() <= 2e-6, "sum dy"
        assert (np.abs(rec[:, g, 1] - s2) / n1).max() <= 2e-6, "sum dy * xhat"


# ---------------------------------------------------------------------------------------------------------------- predicates
def test_predicates_agree_with_entries(dev):
    """A seeded draw of 200 shapes: onet_conv3x3_winograd4_wgrad_ok, onet_conv3x3_winograd4_nparts and onet_conv3x3_stem_nparts
    against their restatements and against what the entries do -- an accepted shape runs (its results finite, nothing written
    outside them), a refused shape returns non-zero BEFORE any launch and writes nothing"""
    from onet_amd import _lib
    from onet_amd._lib import OnetHipError
    lib = _lib.load()
    g = cr.rng(171)
    seen = {k: [0, 0] for k in ("wgrad_ok", "wino_nparts", "stem_nparts")}

    def refused(name, outs, *args):
        with pytest.raises(OnetHipError):
            call(name, *args)
        torch.cuda.synchronize()
        for o in outs:
            assert bool(torch.isnan(o.buf).all()), name + ": a refused call wrote"

    for _ in range(200):
        B, H, W = int(g.integers(1, 5)), int(g.choice([3, 4, 8, 16, 16, 18, 32])), int(g.choice([8, 16, 24, 32, 64, 64, 128]))
        Cin, Cout = int(g.choice([1, 3, 4, 4, 5, 32, 32, 64])), int(g.choice([2, 4, 6, 8, 68]))
        x, dz = Plane(dev, B, Cin, H, W, cr.gaussian(B, Cin, H, W, 172)), Plane(dev, B, Cout, H, W, cr.gaussian(B, Cout, H, W, 173))
        # F(3x3,4x4) weight gradient
        ok = int(lib.onet_conv3x3_winograd4_wgrad_ok(B, Cin, Cout, H, W))
        assert ok == int(cr.wino4w_ok(B, Cin, Cout, H, W))
        seen["wgrad_ok"][ok] += 1
        if ok:
            need = int(lib.onet_conv3x3_winograd4_wgrad_ws_bytes(B, Cin, Cout, H, W))
            dw, ws = Flat(dev, Cout * Cin * 9), Flat(dev, need // 4)
            call("onet_conv3x3_winograd4_wgrad", x.ptr, x.bs, dz.ptr, dz.bs, dw.ptr, ws.ptr, need, B, Cin, Cout, H, W, 0)
            assert bool(torch.isfinite(dw.take("dW")).all())
            ws.guard_ok("workspace")
        else:
            dw, ws = Flat(dev, 64), Flat(dev, 64)
            refused("onet_conv3x3_winograd4_wgrad", (dw, ws), x.ptr, x.bs, dz.ptr, dz.bs, dw.ptr, ws.ptr, 1 << 40, B, Cin, Cout, H, W, 0)
        # F(4x4) forward with statistics
        n = int(lib.onet_conv3x3_winograd4_nparts(B, H, W))
        assert n == cr.wino4_nparts(B, H, W)
        if Cin % 4 == 0 and Cout % 4 == 0:
            seen["wino_nparts"][n > 0] += 1
            qf, _ = wino_packs(dev, cr.weights(Cout, Cin, 3, 174))
            if n:
                z, part = Plane(dev, B, Cout, H, W), Flat(dev, Cout * n * 3)
                call("onet_conv3x3_winograd4_fwd_stats", x.ptr, x.bs, qf.ptr, z.ptr, z.bs, part.ptr, B, Cin, Cout, H, W)
                assert bool(torch.isfinite(z.take("z")).all()) and bool(torch.isfinite(part.take("records")).all())
            else:
                z, part = Flat(dev, 64), Flat(dev, 64)
                refused("onet_conv3x3_winograd4_fwd_stats", (z, part), x.ptr, x.bs, qf.ptr, z.ptr, Cout * H * W, part.ptr, B, Cin, Cout, H, W)
        # stem forward with statistics
        n = int(lib.onet_conv3x3_stem_nparts(B, Cin, Cout, H, W))
        assert n == cr.stem_nparts(B, Cin, Cout, H, W)
        seen["stem_nparts"][n > 0] += 1
        w = T(cr.weights(Cout, Cin, 3, 175), dev)
        if n:
            z, part = Plane(dev, B, Cout, H, W), Flat(dev, Cout * n * 3)
            call("onet_conv3x3_stem_fwd_stats", x.ptr, x.bs, w.data_ptr(), z.ptr, z.bs, part.ptr, B, Cin, Cout, H, W, 0, 0.0)
            assert bool(torch.isfinite(z.take("z")).all()) and bool(torch.isfinite(part.take("records")).all())
        else:
            z, part = Flat(dev, 64), Flat(dev, 64)
            refused("onet_conv3x3_stem_fwd_stats", (z, part), x.ptr, x.bs, w.data_ptr(), z.ptr, Cout * H * W, part.ptr, B, Cin, Cout, H, W, 0, 0.0)
    print("PREDICATES (refused, accepted):", seen)
    assert all(min(v) >= 5 for v in seen.values()), seen          # the draw reaches both answers of every predicate


# ---------------------------------------------------------------------------------------------------------------- the 2 GiB range
@pytest.mark.parametrize("what,Cin,Cout,H,W,ks", [("image", 8, 8, 8192, 8192, 3), ("image", 8, 8, 8192, 8192, 1), ("weights", 8192, 8192, 1, 1, 3),
                                                  ("dz image", 8, 2000, 512, 512, 3)])
def test_range_refusal(dev, what, Cin, Cout, H, W, ks):
    """conv_fwd_kernel and conv_wgrad_kernel stage one image and the packed weights through 32-bit buffer resources with 32-bit byte
    offsets: onet_conv_fwd / onet_conv_wgrad refuse an operand of 2 GiB or more BEFORE any launch (small real tensors, the declared
    dimensions and strides beyond the range; nothing is allocated at that size and nothing may be written)"""
    from onet_amd._lib import OnetHipError
    x, w, out, ws = Flat(dev, 1024, np.ones(1024)), Flat(dev, 1024, np.ones(1024)), Flat(dev, 1024), Flat(dev, 1024)
    # the buffers are 4 KB: a declared shape INSIDE the range would be launched on them.  Hence the restated range first, per call.
    if what != "dz image":
        assert not cr.fwd_in_range(Cin, Cout, Cin, H * W, ks)
        with pytest.raises(OnetHipError, match="2 GiB buffer-resource range"):
            call("onet_conv_fwd", x.ptr, Cin * H * W, w.ptr, out.ptr, Cout * H * W, None, 1, Cin, Cout, H, W, ks)
    if what != "weights":
        assert not cr.dw_in_range(Cin, H * W, Cout, H * W) and not (ks == 3 and Cin <= 4)
        with pytest.raises(OnetHipError, match="2 GiB buffer-resource range"):
            call("onet_conv_wgrad", x.ptr, Cin * H * W, w.ptr, Cout * H * W, out.ptr, ws.ptr, 1 << 40, 1, Cin, Cout, H, W, ks, 0, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all()) and bool(torch.isnan(ws.buf).all()), "a refused call wrote"


@pytest.mark.parametrize("entry", ["fwd", "dgrad", "wgrad"])
def test_range_refusal_convT_fallbacks(dev, entry):
    """The ConvTranspose2d entries fall back to the same kernels (conv_fwd_kernel MODE 1 / MODE 2, conv_wgrad_kernel<1,PW,S2D>) where the
    128 x 128 GEMMs do not take the shape (here: Cin = 8): the fallback refuses an operand beyond the range before any launch too.
    MODE 2 and S2D gather from the [Ct][Ho][Wo] window: their range is that of Ct planes of Ho Wo floats."""
    from onet_amd._lib import OnetHipError
    Cin, h = 8, 8192
    Ct = 64 if entry == "wgrad" else 8
    small, big = Cin * h * h, Ct * 4 * h * h             # batch strides of x [Cin][h][w] and of y / dy [Ct][2h][2w]
    geom = (1, Cin, Ct, h, h, 2 * h, 2 * h, 0, 0, 0)
    # the buffers are 4 KB: a declared shape INSIDE the range would be launched on them.  Hence, before the call: the GEMM path does
    # not take the shape (Cin % 16 != 0), and the fallback's restated range refuses it
    assert Cin % 16 != 0
    assert not {"fwd": cr.fwd_in_range(Cin, 4 * Ct, Cin, h * h, 1), "dgrad": cr.fwd_in_range(4 * Ct, Cin, Ct, 4 * h * h, 1),
                "wgrad": cr.dw_in_range(Cin, h * h, Ct, 4 * h * h)}[entry]
    x, w, out, ws = Flat(dev, 1024, np.ones(1024)), Flat(dev, 1024, np.ones(1024)), Flat(dev, 1024), Flat(dev, 1024)
    with pytest.raises(OnetHipError, match="2 GiB buffer-resource range"):
        if entry == "fwd":
            call("onet_convT2x2_fwd", x.ptr, small, w.ptr, None, out.ptr, big, *geom)
        elif entry == "dgrad":
            call("onet_convT2x2_dgrad", x.ptr, big, w.ptr, out.ptr, small, *geom)
        else:
            call("onet_convT2x2_wgrad", x.ptr, small, w.ptr, big, out.ptr, ws.ptr, 1 << 40, *geom)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all()) and bool(torch.isnan(ws.buf).all()), "a refused call wrote"
