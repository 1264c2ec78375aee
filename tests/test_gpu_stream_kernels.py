"""The streaming kernels of onet_amd/csrc/spatial.hip, head_loss.hip and optim.hip against the fp64 references of tests/stream_refs.py,
element by element, at their path edges and beyond their grid caps.

Every bound is |got - ref| <= k u mag (+ floor), u = 2^-24, mag the reference's magnitude array (the same formula on absolute values),
floor = 2^-126 where a result may be subnormal; tests/test_stream_refs_host.py shows that correct fp32 arithmetic meets each of them on
these inputs (and that the textbook softmax backward does not).  Selections and copies are compared bit for bit.  The quirk function
is held to 4 u max(1, |f|) at its branch points and, on the two million random arguments of the grid-stride case, to 8 u
(stream_refs.K_QUIRK, derived there for exp and log accurate to 2 ulp).  Inputs and bounds live in stream_refs.py, shared with the
host test.

Which dispatch branch a case takes is restated here from the entry point's predicate (pool_fwd_float2, pool_bwd_v4, copy_v4) and the
case lists are asserted to hold both sides of every condition, one flipped at a time:

    onet_maxpool2_fwd      float2: W even, x_bs even, x 8-byte aligned         POOL_FWD: odd-W, odd-stride-slice, x+4B -> scalar; rest float2
    maxpool2_bwd_impl      v4: W % 4 == 0, H even, x_bs / dx_bs / add_bs / add2_bs % 4 == 0, dy_bs even, x / dx / add / add2 16-byte
                           and dy 8-byte aligned                               POOL_BWD_VARIANTS: base (2, 4, 8, 16) -> v4; each other
                                                                               entry flips one condition -> per-pixel kernel
    onet_copy_strided      float4: n % 4 == 0, both strides % 4 == 0, both pointers 16-byte aligned       COPY_CASES
    grid-stride loops      grid_for caps at 16384 blocks of 256, grid_px and onet_adam_step at 8192, jsd_fwd_kernel at 2048: every capped
                           kernel of the three files runs once with more elements than cap * 256 (test_*grid_stride*, the longest Adam
                           buffer, the two longest jsd pixel counts)

Operands that the ops wrappers cannot express (accumulate, batch strides, base pointers off by one float) go to the C entry points
through _lib.call on NaN-filled buffers, whose padding must stay NaN."""
import functools

import numpy as np
import pytest
import torch

import stream_refs as sr

pytestmark = pytest.mark.gpu

U, FLOOR = sr.U, sr.FLOOR
T = torch.from_numpy
CAP = 16384 * 256            # grid_for: elements of one sweep of the capped grid
CAP_PX = 8192 * 256          # grid_px, onet_adam_step (float4s)
CAP_JSD = sr.CAP_JSD


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from onet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def within(got, ref, bnd, what):
    """|got - ref| <= bnd per element, every element finite; prints the worst error / bound"""
    return sr.within(host(got), ref, bnd, what, report=print)


def same(got, ref, what):
    got, ref = host(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref.astype(got.dtype)), f"{what}: {int((got != ref).sum())} of {got.size} elements differ"


class Buf:
    """B rows of n floats at batch stride bs, the first row `off` floats past a 256-byte boundary, in a NaN-filled device buffer"""

    def __init__(self, dev, B, n, data=None, bs=None, off=0):
        self.B, self.n, self.bs, self.off = B, n, (n if bs is None else bs), off
        self.t = torch.full((off + B * self.bs + 8,), float("nan"), dtype=torch.float32, device=dev)
        assert self.t.data_ptr() % 256 == 0
        self.rows = self.t[off:off + B * self.bs].view(B, self.bs)[:, :n]
        if data is not None:
            self.rows.copy_(T(np.ascontiguousarray(data, np.float32).reshape(B, n)))
        self.ptr = self.t.data_ptr() + 4 * off

    def get(self, shape=None):
        a = self.rows.cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def padding_is_nan(self):
        m = torch.ones_like(self.t, dtype=torch.bool)
        m[self.off:self.off + self.B * self.bs].view(self.B, self.bs)[:, :self.n] = False
        return bool(torch.isnan(self.t[m]).all())


def sliced(dev, data, C2=2):
    """data [B, C, H, W] as the channel slice [:, C2:] of a NaN-filled concat buffer -> (view, buffer)"""
    B, C, H, W = data.shape
    buf = torch.full((B, C2 + C, H, W), float("nan"), dtype=torch.float32, device=dev)
    buf[:, C2:].copy_(T(np.ascontiguousarray(data, np.float32)))
    return buf[:, C2:], buf


# ================================================================================================================ max-pooling
def pool_fwd_float2(W, x_bs, x_off):
    return W % 2 == 0 and x_bs % 2 == 0 and x_off % 2 == 0


# name: shape, x offset (floats), x batch stride - CHW, y batch stride - C Ho Wo
POOL_FWD = {
    "odd-W": ((2, 3, 9, 11), 0, 0, 0),
    "odd-H": ((1, 4, 7, 10), 0, 0, 0),
    "one-window": ((2, 5, 2, 2), 0, 0, 0),
    "two-blocks": ((1, 64, 130, 34), 0, 0, 0),
    "slice": ((2, 4, 8, 10), 320, 640, 0),                 # [:, C:2C] of a tensor of 3C channels
    "slice-odd-stride": ((2, 4, 8, 10), 320, 641, 0),
    "x+4B": ((2, 4, 8, 10), 1, 0, 0),
    "strided-y": ((2, 4, 8, 10), 0, 0, 3),
}
assert {k for k, (s, off, xb, yb) in POOL_FWD.items() if not pool_fwd_float2(s[3], s[1] * s[2] * s[3] + xb, off)} == \
    {"odd-W", "slice-odd-stride", "x+4B"}


@pytest.mark.parametrize("name", POOL_FWD)
def test_maxpool_forward(dev, name):
    from onet_amd import _lib
    shape, off, xb, yb = POOL_FWD[name]
    B, C, H, W = shape
    n, no = C * H * W, C * (H // 2) * (W // 2)
    x = sr.pool_input(*shape)
    X, Y = Buf(dev, B, n, x, bs=n + xb, off=off), Buf(dev, B, no, bs=no + yb)
    _lib.call("onet_maxpool2_fwd", X.ptr, X.bs, Y.ptr, Y.bs, B, C, H, W, stream())
    same(Y.get((B, C, H // 2, W // 2)), sr.maxpool2_fwd(x), "maxpool fwd " + name)
    assert Y.padding_is_nan() and np.array_equal(X.get(), x.reshape(B, n))


def test_maxpool_forward_wrapper_on_a_channel_slice(dev):
    from onet_amd import ops
    x = sr.pool_input(2, 4, 8, 10)
    view, _ = sliced(dev, x, C2=4)
    same(ops.maxpool2_fwd(view), sr.maxpool2_fwd(x), "ops.maxpool2_fwd")


def pool_bwd_v4(shape, st, of, add, add2):
    B, C, H, W = shape
    al = lambda k, m: (4 * of[k]) % m == 0
    return W % 4 == 0 and H % 2 == 0 and st["x"] % 4 == 0 and st["dx"] % 4 == 0 and st["dy"] % 2 == 0 and \
        (not add or (st["add"] % 4 == 0 and al("add", 16))) and (not add2 or (st["add2"] % 4 == 0 and al("add2", 16))) and \
        al("x", 16) and al("dx", 16) and al("dy", 8)


# name: (shape, operand whose batch stride grows | None, by, operand whose base moves one float | None)
POOL_BWD_VARIANTS = {
    "base": ((2, 4, 8, 16), None, 0, None),
    "W18": ((2, 4, 8, 18), None, 0, None),
    "H9": ((2, 4, 9, 16), None, 0, None),
    "x_bs+2": ((2, 4, 8, 16), "x", 2, None),
    "dx_bs+2": ((2, 4, 8, 16), "dx", 2, None),
    "add_bs+2": ((2, 4, 8, 16), "add", 2, None),
    "add2_bs+2": ((2, 4, 8, 16), "add2", 2, None),
    "dy_bs+1": ((2, 4, 8, 16), "dy", 1, None),
    "x+4B": ((2, 4, 8, 16), None, 0, "x"),
    "dx+4B": ((2, 4, 8, 16), None, 0, "dx"),
    "add+4B": ((2, 4, 8, 16), None, 0, "add"),
    "add2+4B": ((2, 4, 8, 16), None, 0, "add2"),
    "dy+4B": ((2, 4, 8, 16), None, 0, "dy"),
    "odd": ((2, 3, 9, 11), None, 0, None),
    "odd-strided": ((2, 3, 9, 11), "dx", 5, None),
}
POOL_BWD_MODES = (("plain", 0, 0, 0), ("accumulate", 0, 0, 1), ("add", 1, 0, 0), ("add+add2", 1, 1, 0))      # name, add, add2, accumulate


def pool_bwd_layout(variant):
    shape, grow, by, moved = POOL_BWD_VARIANTS[variant]
    B, C, H, W = shape
    n, no = C * H * W, C * (H // 2) * (W // 2)
    st = dict(x=n, dx=n, add=n, add2=n, dy=no)
    of = dict(x=0, dx=0, add=0, add2=0, dy=0)
    if grow:
        st[grow] += by
    if moved:
        of[moved] = 1
    return shape, n, no, st, of


def test_pool_backward_cases_take_both_kernels():
    """with all three gradients present the base case is the only 2 x 4-patch one: every other entry flips exactly one condition"""
    v4 = set()
    for k in POOL_BWD_VARIANTS:
        s, n, no, st, of = pool_bwd_layout(k)
        if pool_bwd_v4(s, st, of, True, True):
            v4.add(k)
    assert v4 == {"base"}
    # ... and a variant of an operand that is absent does not leave the patch kernel
    s, n, no, st, of = pool_bwd_layout("add2+4B")
    assert pool_bwd_v4(s, st, of, True, False) and not pool_bwd_v4(s, st, of, True, True)


@pytest.mark.parametrize("mode", POOL_BWD_MODES, ids=[m[0] for m in POOL_BWD_MODES])
@pytest.mark.parametrize("variant", POOL_BWD_VARIANTS)
def test_maxpool_backward(dev, variant, mode):
    from onet_amd import _lib
    _, has_add, has_add2, acc = mode
    shape, n, no, st, of = pool_bwd_layout(variant)
    B, C, H, W = shape
    x = sr.pool_input(*shape)
    dy, add, add2, old = (sr.normal(*s, seed=k) for k, s in ((2, (B, C, H // 2, W // 2)), (3, shape), (4, shape), (5, shape)))
    X, DY = Buf(dev, B, n, x, st["x"], of["x"]), Buf(dev, B, no, dy, st["dy"], of["dy"])
    DX = Buf(dev, B, n, old if acc else None, st["dx"], of["dx"])
    A = Buf(dev, B, n, add, st["add"], of["add"]) if has_add else None
    A2 = Buf(dev, B, n, add2, st["add2"], of["add2"]) if has_add2 else None
    _lib.call("onet_maxpool2_bwd", X.ptr, X.bs, DY.ptr, DY.bs, A.ptr if A else None, A.bs if A else 0, A2.ptr if A2 else None,
              A2.bs if A2 else 0, DX.ptr, DX.bs, B, C, H, W, acc, stream())
    ref, mag = sr.maxpool2_bwd(x, dy, add if has_add else None, add2 if has_add2 else None, old if acc else None)
    got = DX.get(shape)
    within(got, ref, sr.bound(4, mag), f"maxpool bwd {variant} {mode[0]} ({'v4' if pool_bwd_v4(shape, st, of, has_add, has_add2) else 'per-pixel'})")
    assert not got[mag == 0].any()                           # exact zeros where no term is: the dropped odd row and column too
    if not (has_add or acc):
        assert not got[:, :, 2 * (H // 2):, :].any() and not got[:, :, :, 2 * (W // 2):].any()
    assert DX.padding_is_nan()


def test_maxpool_backward_refusals_and_wrapper(dev):
    from onet_amd import _lib, ops
    shape = (2, 4, 8, 16)
    B, C, H, W = shape
    n, no = C * H * W, C * (H // 2) * (W // 2)
    x = sr.pool_input(*shape)
    dy, add = sr.normal(B, C, H // 2, W // 2, seed=2), sr.normal(*shape, seed=3)
    X, DY, A, DX = Buf(dev, B, n, x), Buf(dev, B, no, dy), Buf(dev, B, n, add), Buf(dev, B, n)
    with pytest.raises(_lib.OnetHipError):                  # add2 without add
        _lib.call("onet_maxpool2_bwd", X.ptr, n, DY.ptr, no, None, 0, A.ptr, n, DX.ptr, n, B, C, H, W, 0, stream())
    with pytest.raises(_lib.OnetHipError):                  # add together with accumulate
        _lib.call("onet_maxpool2_bwd", X.ptr, n, DY.ptr, no, A.ptr, n, None, 0, DX.ptr, n, B, C, H, W, 1, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(DX.t).all())
    xv, _ = sliced(dev, x)
    av, _ = sliced(dev, add, C2=3)
    ref, mag = sr.maxpool2_bwd(x, dy, add)
    within(ops.maxpool2_bwd(xv, T(dy).to(dev), add=av), ref, sr.bound(4, mag), "ops.maxpool2_bwd on channel slices")


def test_maxpool_grid_stride(dev):
    """more outputs (forward, both kernels) and more patches / pixels (backward, both kernels) than the capped grid covers in one sweep"""
    from onet_amd import _lib
    Wo = CAP + 1000
    r = sr.rng(71)
    for W, f2 in ((2 * Wo, True), (2 * Wo + 1, False)):                 # one long two-row plane: Wo windows
        x = np.maximum(r.standard_normal((1, 1, 2, W), dtype=np.float32), 0)
        assert pool_fwd_float2(W, 2 * W, 0) == f2
        X, Y = Buf(dev, 1, 2 * W, x), Buf(dev, 1, Wo)
        _lib.call("onet_maxpool2_fwd", X.ptr, 2 * W, Y.ptr, Wo, 1, 1, 2, W, stream())
        same(Y.get((1, 1, 1, Wo)), sr.maxpool2_fwd(x), f"maxpool fwd grid stride W={W}")
        assert Y.padding_is_nan()
        del X, Y
    for W in (4 * Wo, Wo + 1):                                          # 8 (CAP + 1000) inputs in 2 x 4 patches; CAP + 1001 pixels one by one
        x = np.maximum(r.standard_normal((1, 1, 2, W), dtype=np.float32), 0)
        dy = r.standard_normal((1, 1, 1, W // 2), dtype=np.float32)
        assert (W % 4 == 0) == (W == 4 * Wo) and 2 * W // (8 if W % 4 == 0 else 1) > CAP
        X, DY, DX = Buf(dev, 1, 2 * W, x), Buf(dev, 1, W // 2, dy), Buf(dev, 1, 2 * W)
        _lib.call("onet_maxpool2_bwd", X.ptr, 2 * W, DY.ptr, W // 2, None, 0, None, 0, DX.ptr, 2 * W, 1, 1, 2, W, 0, stream())
        ref, _ = sr.maxpool2_bwd(x, dy)
        same(DX.get((1, 1, 2, W)), ref, f"maxpool bwd grid stride W={W}")          # one term per element: exact
        assert DX.padding_is_nan()
        del X, DY, DX


# ================================================================================================================ placement, copies
@pytest.mark.parametrize("geom", sr.PLACE)
def test_pixel_shuffle_space_to_depth_dbias(dev, geom):
    from onet_amd import _lib, ops
    h, w, Ho, Wo, pt, pl = geom
    sub, bias, dy = sr.place_case(h, w, Ho, Wo)
    B, C = dy.shape[:2]
    for b in (bias, None):
        out, buf = sliced(dev, np.full((B, C, Ho, Wo), np.nan, np.float32))
        ops.pixel_shuffle2_bias(T(sub).to(dev), None if b is None else T(b).to(dev), out, pt, pl)
        same(out, sr.pixel_shuffle2_bias(sub, b, Ho, Wo, pt, pl), "pixel_shuffle2_bias")
        assert bool(torch.isnan(buf[:, :2]).all())
    dyv, dybuf = sliced(dev, dy)
    db_ref, db_mag = sr.convT_dbias(dy, h, w, pt, pl)
    for want in (False, True):
        got, db = ops.space_to_depth2(dyv, h, w, pt, pl, want)
        same(got, sr.space_to_depth2(dy, h, w, pt, pl), "space_to_depth2")
        assert (db is None) == (not want)
        if want:
            within(db, db_ref, sr.bound(4, db_mag), "space_to_depth2 dbias")
    old = sr.normal(C, seed=34)
    scratch = torch.empty(B * C, dtype=torch.float64, device=dev)
    for acc in (0, 1):
        db = T(old.copy()).to(dev)
        _lib.call("onet_convT2x2_dbias", dyv.data_ptr(), dyv.stride(0), db.data_ptr(), scratch.data_ptr(), acc, B, C, h, w, Ho, Wo, pt, pl,
                  stream())
        within(db, db_ref + acc * old.astype(np.float64), sr.bound(4, db_mag + acc * np.abs(old)), f"convT2x2_dbias accumulate={acc}")
    assert bool(torch.isnan(dybuf[:, :2]).all()) and np.array_equal(host(dyv), dy)


def copy_v4(n, sbs, dbs, soff, doff):
    return n % 4 == 0 and sbs % 4 == 0 and dbs % 4 == 0 and soff % 4 == 0 and doff % 4 == 0


# name: B, n, source stride - n, destination stride - n, source offset, destination offset (floats)
COPY_CASES = {
    "float4": (3, 64, 0, 0, 0, 0),
    "float4-strided": (3, 64, 8, 64, 4, 8),
    "n%4": (3, 66, 0, 0, 0, 0),
    "src-odd-stride": (3, 64, 1, 0, 0, 0),
    "dst-stride%4": (3, 64, 0, 2, 0, 0),
    "src+4B": (3, 64, 0, 0, 1, 0),
    "dst+4B": (3, 64, 0, 0, 0, 1),
    "float4-grid-stride": (2, 2 * (CAP + 1000), 4, 0, 0, 0),
    "scalar-grid-stride": (1, CAP + 1001, 0, 0, 0, 0),
}
assert {k for k, (B, n, sb, db, so, do) in COPY_CASES.items() if copy_v4(n, n + sb, n + db, so, do)} == \
    {"float4", "float4-strided", "float4-grid-stride"}


@pytest.mark.parametrize("name", COPY_CASES)
def test_copy_strided(dev, name):
    from onet_amd import _lib
    B, n, sb, db, so, do = COPY_CASES[name]
    data = sr.rng(72, n).standard_normal((B, n), dtype=np.float32)
    S, D = Buf(dev, B, n, data, n + sb, so), Buf(dev, B, n, None, n + db, do)
    _lib.call("onet_copy_strided", S.ptr, S.bs, D.ptr, D.bs, B, n, stream())
    same(D.get(), data, "copy_strided " + name)
    assert D.padding_is_nan()


def test_fill_axpy_complement_clip(dev):
    from onet_amd import _lib, ops
    for n in (1, 257, CAP + 1000):
        t = torch.full((n + 8,), float("nan"), device=dev)
        ops.fill(t[:n], -2.5)
        assert bool((t[:n] == -2.5).all()) and bool(torch.isnan(t[n:]).all())
    for B, n, xb, yb in ((2, 1001, 3, 6), (1, CAP + 1000, 0, 0)):
        x, y = sr.rng(73, n).standard_normal((B, n), dtype=np.float32), sr.rng(74, n).standard_normal((B, n), dtype=np.float32)
        for a in (1.0, -0.37):
            for acc in (0, 1):
                X, Y = Buf(dev, B, n, x, n + xb), Buf(dev, B, n, y if acc else None, n + yb)
                _lib.call("onet_axpy", X.ptr, X.bs, Y.ptr, Y.bs, a, B, n, acc, stream())
                ref, mag = sr.axpy(a, x, y if acc else None)
                within(Y.get(), ref, sr.bound(2, mag), f"axpy a={a} accumulate={acc} n={n}")
                assert Y.padding_is_nan()
    edge = np.array([0.0, 1.0, 0.1, 1.1, -0.0, 0.5, 2.0, -1.0, 1.1 + 2.0 ** -20, 0.1 - 2.0 ** -24, 0.1 + 2.0 ** -26], np.float32)
    x = np.concatenate([edge, sr.rng(75).uniform(-0.5, 1.5, CAP + 1000).astype(np.float32)])
    got = ops.complement_clip(T(x).to(dev), 0.1)
    ref = sr.complement_clip(x, 0.1)
    same(got, ref, "complement_clip")
    assert ref[2] == 1 and ref[3] == 0 and ref[:11].min() == 0 and ref[:11].max() == 1          # values exactly at the clip points


def test_placement_grid_stride(dev):
    from onet_amd import ops
    h, w, Ho, Wo, pt, pl = 64, 64, 129, 131, 1, 2
    B, C = 5, 64                                               # 5.4 M outputs, 5.2 M gathered elements: both kernels run past the cap
    assert B * C * Ho * Wo > CAP and B * 4 * C * h * w > CAP
    r = sr.rng(76)
    sub, bias = r.standard_normal((B, 4 * C, h, w), dtype=np.float32), r.standard_normal(C, dtype=np.float32)
    out = torch.full((B, C, Ho, Wo), float("nan"), device=dev)
    ops.pixel_shuffle2_bias(T(sub).to(dev), T(bias).to(dev), out, pt, pl)
    ref = sr.pixel_shuffle2_bias(sub, bias, Ho, Wo, pt, pl)
    same(out, ref, "pixel_shuffle2_bias grid stride")
    got, _ = ops.space_to_depth2(out, h, w, pt, pl, False)
    same(got, sr.space_to_depth2(ref, h, w, pt, pl), "space_to_depth2 grid stride")


# ================================================================================================================ bilinear x2
@pytest.mark.parametrize("hw", sr.BIL_HW)
def test_bilinear(dev, hw):
    """(a source index contracted into fma(scale, o, -i0) misses the forward bound from 12 x 12 on, 56 times over at 128 x 128)"""
    from onet_amd import ops
    h, w = hw
    for Ho, Wo, pt, pl in sr.bil_geoms(h, w):
        x, g = sr.bil_case(h, w, Ho, Wo)
        B, C = x.shape[:2]
        out, obuf = sliced(dev, np.full((B, C, Ho, Wo), np.nan, np.float32))
        ops.bilinear2x_fwd(T(x).to(dev), out, pt, pl)
        ref, mag = sr.bilinear2x_fwd(x, Ho, Wo, pt, pl)
        bf = sr.bound(8, mag)
        within(out, ref, bf, f"bilinear fwd {hw} {(Ho, Wo, pt, pl)}")
        y = host(out).astype(np.float64)
        assert not y[mag == 0].any() and bool(torch.isnan(obuf[:, :2]).all())          # the padded border is exactly 0
        border = np.ones((Ho, Wo), bool)
        border[pt:pt + 2 * h, pl:pl + 2 * w] = False
        assert not y[:, :, border].any()
        gv, _ = sliced(dev, g, C2=3)
        dx = ops.bilinear2x_bwd(gv, h, w, pt, pl)
        dref, dmag = sr.bilinear2x_bwd(g, h, w, pt, pl)
        bb = sr.bound(16, dmag)
        within(dx, dref, bb, f"bilinear bwd {hw} {(Ho, Wo, pt, pl)}")
        # <bwd(g), x> = <g, fwd(x)> on the device results, fp64, within the two bounds combined
        lhs, rhs = float((host(dx).astype(np.float64) * x).sum()), float((g.astype(np.float64) * y).sum())
        assert abs(lhs - rhs) <= float((bb * np.abs(x)).sum() + (np.abs(g) * bf).sum()), (lhs, rhs)


def test_bilinear_grid_stride(dev):
    from onet_amd import ops
    h = w = 128
    r = sr.rng(77)
    x = r.standard_normal((1, 65, h, w), dtype=np.float32)              # 65 * 256 * 256 outputs > CAP
    assert x.shape[1] * 4 * h * w > CAP
    out = torch.empty((1, 65, 2 * h, 2 * w), device=dev)
    ops.bilinear2x_fwd(T(x).to(dev), out, 0, 0)
    ref, mag = sr.bilinear2x_fwd(x, 2 * h, 2 * w, 0, 0)
    within(out, ref, sr.bound(8, mag), "bilinear fwd grid stride")
    g = r.standard_normal((1, 257, 2 * h, 2 * w), dtype=np.float32)     # 257 * 128 * 128 inputs > CAP
    assert g.shape[1] * h * w > CAP
    dx = ops.bilinear2x_bwd(T(g).to(dev), h, w, 0, 0)
    dref, dmag = sr.bilinear2x_bwd(g, h, w, 0, 0)
    within(dx, dref, sr.bound(16, dmag), "bilinear bwd grid stride")


# ================================================================================================================ head
HEAD_CASES = sr.HEAD_CASES
head_fwd_bounds, head_bwd_bound = sr.head_fwd_bounds, sr.head_bwd_bound


@functools.lru_cache(maxsize=None)
def head_ref(C, HW, norm):
    c = sr.head_case(C, HW, norm=norm)
    fwd = sr.head_fwd(c["Lt"], c["Ht"], c["Ld"], c["Hd"], c.get("nt"), c.get("nd"))
    return c, fwd


def as_map(dev, a, wide=False):
    """[B, C, HW] -> device [B, C, 1, HW]; wide: the second half of a 2B-image tensor with one channel more (batch stride (C + 1) HW)"""
    a = np.ascontiguousarray(a, np.float32)
    B, C, HW = a.shape
    if not wide:
        return T(a).to(dev).view(B, C, 1, HW)
    buf = torch.full((2 * B, C + 1, 1, HW), float("nan"), device=dev)
    buf[B:, 1:].copy_(T(a).view(B, C, 1, HW))
    return buf[B:, 1:]


@pytest.mark.parametrize("wide", (False, True), ids=("contiguous", "second-halves"))
@pytest.mark.parametrize("C,HW,norm", HEAD_CASES)
def test_head_forward(dev, C, HW, norm, wide):
    from onet_amd import ops
    c, ref = head_ref(C, HW, norm)
    B = c["Lt"].shape[0]
    Lt, Ht, Ld, Hd = (as_map(dev, c[k], wide) for k in ("Lt", "Ht", "Ld", "Hd"))
    h_norm = (T(c["nt"]).to(dev), T(c["nd"]).to(dev)) if norm else None
    Vt, Vd, S, sLt, sLd = ops.head_softmax_fwd(Lt, Ht, Ld, Hd, want_sums=True, h_norm=h_norm)
    bVt, bVd, bS = head_fwd_bounds(ref, C)
    within(Vt.view(B, HW), ref["Vt"], bVt, "Vt")
    within(Vd.view(B, HW), ref["Vd"], bVd, "Vd")
    within(S.view(B, 2, HW), ref["S"], bS, "S")
    within(sLt.view(B, HW), ref["sLt"], sr.bound(C, ref["msLt"]), "sLt")
    within(sLd.view(B, HW), ref["sLd"], sr.bound(C, ref["msLd"]), "sLd")
    same(sLt.view(B, HW), sr.channel_sums32(c["Lt"]), "sLt: channel after channel in float32")
    # bit identity with the sums the loss kernel forms of the same L
    for L, s in ((Lt, sLt), (Ld, sLd)):
        _, sums = ops.jsd_fwd(L, S[:, 0:1], S[:, 1:2])
        assert torch.equal(sums.view(-1), s.view(-1))
    # without the sums: the same V and S
    Vt2, Vd2, S2 = ops.head_softmax_fwd(Lt, Ht, Ld, Hd, h_norm=h_norm)
    assert torch.equal(Vt2, Vt) and torch.equal(Vd2, Vd) and torch.equal(S2, S)


@pytest.mark.parametrize("C,HW,norm", HEAD_CASES)
def test_head_backward(dev, C, HW, norm):
    from onet_amd import ops
    c, fwd = head_ref(C, HW, norm)
    B = c["Lt"].shape[0]
    S32 = fwd["S"].astype(np.float32)
    assert (S32 == 1).any() and (S32 == 0).any()
    Sd = T(S32).to(dev).view(B, 2, 1, HW)
    up = {k: T(c[k]).to(dev).view(B, -1, 1, HW) for k in ("dVt", "dVd", "dS", "gst", "gsd")}
    h_norm = (T(c["nt"]).to(dev), T(c["nd"]).to(dev)) if norm else None
    k = 0
    for use_t in (True, False):
        for use_d in (True, False):
            for use_s in (True, False):
                k += 1
                wide = bool(k & 1)                           # L and H as second halves of wider 2B-image tensors, every other combination
                Lt, Ht, Ld, Hd = (as_map(dev, c[n], wide) for n in ("Lt", "Ht", "Ld", "Hd"))
                a = dict(dVt=c["dVt"] if use_t else None, dVd=c["dVd"] if use_d else None, dS=c["dS"] if use_s else None)
                d = [up[n] if a[n] is not None else None for n in ("dVt", "dVd", "dS")]
                g = ops.head_grad_map(d[0], d[1], d[2], Sd).view(2, B, HW)
                for use_g in (True, False):
                    ref = sr.head_bwd(a["dVt"], a["dVd"], a["dS"], S32, c["Lt"], c["Ht"], c["Ld"], c["Hd"], c["gst"] if use_g else None,
                                      c["gsd"] if use_g else None, c.get("nt"), c.get("nd"))
                    within(g[0], ref["gt"], head_bwd_bound(ref, "gt"), f"gt [dVt={use_t} dVd={use_d} dS={use_s}]")
                    within(g[1], ref["gd"], head_bwd_bound(ref, "gd"), f"gd [dVt={use_t} dVd={use_d} dS={use_s}]")
                    for twin in (False, True):
                        tag = f"[dVt={use_t} dVd={use_d} dS={use_s} gsums={use_g} twin={twin} wide={wide}]"
                        out = ops.head_softmax_bwd(d[0], d[1], d[2], Sd, Lt, Ht, Ld, Hd, twin=twin,
                                                   gsums=(up["gst"], up["gsd"]) if use_g else (None, None), h_norm=h_norm)
                        if twin:
                            dL, dH = out
                            out = [dL[:B], dH[:B], dL[B:], dH[B:]]
                        for name, t in zip(("dLt", "dHt", "dLd", "dHd"), out):
                            within(t.reshape(B, C, HW), ref[name], head_bwd_bound(ref, name), f"{name} " + tag)


def test_head_grad_map_is_the_gradient_the_backward_applies(dev):
    """C = 1, H = 1: dL = fma(g, 1, 0) = g, bit for bit"""
    from onet_amd import ops
    c, fwd = head_ref(1, 1237, False)
    B, HW = 2, 1237
    Sd = T(fwd["S"].astype(np.float32)).to(dev).view(B, 2, 1, HW)
    dVt, dVd, dS = (T(c[k]).to(dev).view(B, -1, 1, HW) for k in ("dVt", "dVd", "dS"))
    one = torch.ones((B, 1, 1, HW), device=dev)
    Lt, Ld = as_map(dev, c["Lt"]), as_map(dev, c["Ld"])
    for d in ((dVt, dVd, dS), (None, None, dS), (dVt, None, None)):
        g = ops.head_grad_map(*d, Sd)
        dLt, _, dLd, _ = ops.head_softmax_bwd(*d, Sd, Lt, one, Ld, one)
        assert torch.equal(g[:B], dLt) and torch.equal(g[B:], dLd)


def test_head_grid_stride(dev):
    """C = 2, B HW = 8192 * 256 + 1000 pixels: forward, gradient map and backward beyond the capped grid"""
    from onet_amd import ops
    C, B, HW = 2, 2, (CAP_PX + 1000) // 2
    c = sr.head_case(C, HW, B=B)
    ref = sr.head_fwd(c["Lt"], c["Ht"], c["Ld"], c["Hd"])
    Lt, Ht, Ld, Hd = (as_map(dev, c[k]) for k in ("Lt", "Ht", "Ld", "Hd"))
    Vt, Vd, S, sLt, sLd = ops.head_softmax_fwd(Lt, Ht, Ld, Hd, want_sums=True)
    bVt, bVd, bS = head_fwd_bounds(ref, C)
    within(Vt.view(B, HW), ref["Vt"], bVt, "Vt")
    within(Vd.view(B, HW), ref["Vd"], bVd, "Vd")
    within(S.view(B, 2, HW), ref["S"], bS, "S")
    same(sLd.view(B, HW), sr.channel_sums32(c["Ld"]), "sLd")
    S32 = ref["S"].astype(np.float32)
    Sd = T(S32).to(dev).view(B, 2, 1, HW)
    up = {k: T(c[k]).to(dev).view(B, -1, 1, HW) for k in ("dVt", "dVd", "dS", "gst", "gsd")}
    rb = sr.head_bwd(c["dVt"], c["dVd"], c["dS"], S32, c["Lt"], c["Ht"], c["Ld"], c["Hd"], c["gst"], c["gsd"])
    g = ops.head_grad_map(up["dVt"], up["dVd"], up["dS"], Sd).view(2, B, HW)
    within(g[0], rb["gt"], head_bwd_bound(rb, "gt"), "gt")
    within(g[1], rb["gd"], head_bwd_bound(rb, "gd"), "gd")
    out = ops.head_softmax_bwd(up["dVt"], up["dVd"], up["dS"], Sd, Lt, Ht, Ld, Hd, gsums=(up["gst"], up["gsd"]))
    for name, t in zip(("dLt", "dHt", "dLd", "dHd"), out):
        within(t.reshape(B, C, HW), rb[name], head_bwd_bound(rb, name), name)


# ================================================================================================================ loss
def test_log1pexp_at_its_branch_points(dev):
    from onet_amd import ops
    pts = sr.quirk_points()
    f, df = sr.f_quirk32(pts), sr.df_quirk32(pts)
    x = T(pts.copy()).to(dev)
    y = ops.log1pexp_(x.clone())
    within(y, f, sr.bound(4, np.maximum(1.0, np.abs(f))), "log1pexp_")
    g = ops.log1pexp_bwd(x, torch.ones_like(x))
    within(g, df, sr.bound(4, np.abs(df), FLOOR), "log1pexp_bwd")
    g2 = ops.log1pexp_bwd(x, torch.full_like(x, -2.0))
    assert torch.equal(g2, -2.0 * g)
    # the loss kernel on the same values: sums = +-x with Si = Sp = 1 makes the two arguments exactly -x and x
    one = torch.ones((1, 1, 1, 1), device=dev)
    for v in pts:
        jsd, _ = ops.jsd_fwd(None, one, one, sums=torch.full((1, 1, 1, 1), float(v), device=dev))
        ref, mean_abs = sr.jsd_fwd(np.array([v]), np.ones(1), np.ones(1))
        assert abs(float(jsd) - ref) <= 8 * U * mean_abs, (float(v), float(jsd), ref)
    n = len(pts)
    ones = torch.ones((1, 1, 1, n), device=dev)
    runs = [ops.jsd_fwd(None, ones, ones, sums=x.view(1, 1, 1, n))[0] for _ in range(2)]
    ref, mean_abs = sr.jsd_fwd(pts, np.ones(n), np.ones(n))
    print(f"RATIO jsd on the branch points: {abs(float(runs[0]) - ref) / (8 * U * mean_abs):.3f}")
    assert abs(float(runs[0]) - ref) <= 8 * U * mean_abs and torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("C,B,HW", sr.JSD_CASES)
def test_jsd(dev, C, B, HW):
    """the scalar, the channel sums and the three gradients; with B = 2 the two channel slices of S are read at batch stride 2 HW, L
    (a slice of a tensor of C + 1 channels) at (C + 1) HW, every image with its own values"""
    from onet_amd import ops
    L, S = sr.jsd_case(C, B, HW)
    n = B * HW
    Ld, Sd = as_map(dev, L, wide=B > 1), T(S).to(dev).view(B, 2, 1, HW)
    Si, Sp = Sd[:, 0:1], Sd[:, 1:2]                        # the production layout: two channel slices
    assert B == 1 or (Si.stride(0) == 2 * HW and Sp.data_ptr() - Si.data_ptr() == 4 * HW and Ld.stride(0) == (C + 1) * HW)
    sums_ref = sr.channel_sums32(L)
    ref, mean_abs = sr.jsd_fwd(sums_ref, S[:, 0], S[:, 1])
    (jsd, sums), (jsd2, _) = ops.jsd_fwd(Ld, Si, Sp), ops.jsd_fwd(Ld, Si, Sp)
    same(sums.view(B, HW), sums_ref, "jsd channel sums")
    print(f"RATIO jsd C={C} B={B} HW={HW}: {abs(float(jsd) - ref) / (8 * U * mean_abs):.3f}")
    assert abs(float(jsd) - ref) <= 8 * U * mean_abs, (float(jsd), ref)
    assert torch.equal(jsd, jsd2)
    jsd3, _ = ops.jsd_fwd(None, Si, Sp, sums=sums.view(B, 1, 1, HW))
    assert torch.equal(jsd3, jsd)
    if B > 1:                                              # the roles of the slices swapped: the second term of the loss
        ref_s, mean_s = sr.jsd_fwd(sums_ref, S[:, 1], S[:, 0])
        jsd_s, _ = ops.jsd_fwd(Ld, Sp, Si)
        assert abs(float(jsd_s) - ref_s) <= 8 * U * mean_s, (float(jsd_s), ref_s)
    for gscale in (1.0, -0.37):
        b = sr.jsd_bwd(gscale, sums_ref, S[:, 0], S[:, 1])
        gL, dSi, dSp = ops.jsd_bwd(torch.tensor([gscale], device=dev), sums, Si, Sp, (B, C, 1, HW))
        for name, t in (("gL", gL), ("dSi", dSi), ("dSp", dSp)):
            within(t.view(n), b[name], sr.bound(8, b["m" + name], FLOOR), f"jsd_bwd {name} gscale={gscale}")


def test_loss_elementwise_grid_stride(dev):
    """8192 * 256 + 1000 elements in two images: log1pexp_, log1pexp_bwd, jsd_bwd, argmax2 and softmax2_labels beyond the capped grid.
    On the two million arguments uniform over -60 .. 60 f is held to K_QUIRK = 8 u (stream_refs.K_QUIRK), its derivative to 4 u"""
    from onet_amd import ops
    n = CAP_PX + 1000
    B, HW = 2, n // 2
    r = sr.rng(81)
    x = r.uniform(-60, 60, n).astype(np.float32)
    xd = T(x).to(dev)
    f, df = sr.f_quirk32(x), sr.df_quirk32(x)
    within(ops.log1pexp_(xd.clone()), f, sr.bound(sr.K_QUIRK, np.maximum(1.0, np.abs(f))), "log1pexp_")
    within(ops.log1pexp_bwd(xd, torch.ones_like(xd)), df, sr.bound(4, np.abs(df), FLOOR), "log1pexp_bwd")
    d = r.uniform(-30, 30, (B, HW))
    S = np.stack([1 / (1 + np.exp(-d)), 1 / (1 + np.exp(d))], 1).astype(np.float32)          # [B, 2, HW]
    S[:, 1, ::7] = S[:, 0, ::7]                                           # ties
    Sd = T(S).to(dev).view(B, 2, 1, HW)
    b = sr.jsd_bwd(1.0, x, S[:, 0], S[:, 1])
    gL, dSi, dSp = ops.jsd_bwd(torch.ones(1, device=dev), xd, Sd[:, 0:1], Sd[:, 1:2], (B, 1, 1, HW))
    for name, t in (("gL", gL), ("dSi", dSi), ("dSp", dSp)):
        within(t.view(n), b[name], sr.bound(8, b["m" + name], FLOOR), f"jsd_bwd {name}")
    same(ops.argmax2(Sd).view(B, HW), sr.argmax2(S), "argmax2")
    Vt, Vd = T(d.astype(np.float32)).to(dev).view(B, 1, 1, HW), torch.zeros((B, 1, 1, HW), device=dev)
    S2, Y2 = ops.softmax2_labels(Vt, Vd)
    assert torch.equal(Y2, ops.argmax2(S2))
    clear = np.abs(d) > 1e-3
    assert np.array_equal(host(Y2).reshape(B, HW)[clear], (d < 0).astype(np.int64)[clear])


def test_argmax_ties_and_neighbours(dev):
    """two images, the second with the roles of the classes swapped"""
    from onet_amd import ops
    base = np.array([0.5, 0.25, 1.0, 0.125, 1e-30, 0.75, 0.5, 0.5], np.float32)          # (no subnormal neighbours)
    up, dn = np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(-1))
    s0 = np.concatenate([base, base, base, up, dn])
    s1 = np.concatenate([base, up, dn, base, base])                      # ties, one ulp above, one below
    S = np.stack([np.stack([s0, s1]), np.stack([s1, s0])]).reshape(2, 2, 5, 8)
    want = sr.argmax2(S)
    assert want[0, 0].sum() == 0 and want[0, 1].all() and not want[0, 2].any() and want[1, 2].all() and not want[1, 1].any()
    same(ops.argmax2(T(S).to(dev)), want, "argmax2")
    # softmax2_labels: ties -> 0; values an ulp apart label as argmax2 labels the S the same launch writes; either output alone
    v = np.array([0.5, 1.0, -3.5, 47.0, -120.0, 88.0, 1e-3, 16.0], np.float32)
    a = np.concatenate([v, v, np.nextafter(v, np.float32(1e9)), v + 1, v - 1])
    b = np.concatenate([v, np.nextafter(v, np.float32(1e9)), v, v - 1, v + 1])
    vt, vd = np.stack([a, b]).reshape(2, 1, 5, 8), np.stack([b, a]).reshape(2, 1, 5, 8)
    Vt, Vd = T(vt).to(dev), T(vd).to(dev)
    S_, Y_ = ops.softmax2_labels(Vt, Vd)
    ref = sr.head_fwd(vt.reshape(2, 1, 40), np.ones((2, 1, 40)), vd.reshape(2, 1, 40), np.ones((2, 1, 40)))["S"]
    within(S_.view(2, 2, 40), ref, ref * 8 * U + FLOOR, "softmax2_labels S")
    y = host(Y_).reshape(2, 5, 8)
    assert not y[:, 0].any() and not y[0, 3].any() and y[0, 4].all() and y[1, 3].all() and not y[1, 4].any()
    assert torch.equal(Y_, ops.argmax2(S_))
    S_only, none = ops.softmax2_labels(Vt, Vd, want_labels=False)
    assert none is None and torch.equal(S_only, S_)
    none, Y_only = ops.softmax2_labels(Vt, Vd, want_S=False)
    assert none is None and torch.equal(Y_only, Y_)


# ================================================================================================================ Adam
@pytest.mark.parametrize("n,hyper", sr.ADAM_CASES)
def test_adam_single_step(dev, n, hyper):
    """one step from a given state, the buffers 8 elements longer than n: what lies past n stays untouched.  (The last eighth of the
    state, v a thousandth of g^2 as in the first steps, is where a complement 1.f - 0.999f formed from the rounded beta shows: 1.3e-5 of
    (1 - beta2) g^2, a hundred times the bound on v.  ops.adam_step hands the betas down as doubles: onet_adam_step_f64.)"""
    from onet_amd import ops
    step, wd, gs = hyper
    p, g, m, v = sr.adam_case(n)
    ref = sr.adam_step(p, g, m, v, sr.ADAM_LR, *sr.ADAM_BETAS, sr.ADAM_EPS, wd, step, gs)
    pad = np.array([3.0, -1.0, 0.5, 2.0, -4.0, 1.5, 0.25, -0.125], np.float32)
    P, Gr, M, V = (T(np.concatenate([t, pad])).to(dev) for t in (p, g, m, v))
    ops.adam_step(P[:n], Gr[:n], M[:n], V[:n], sr.ADAM_LR, *sr.ADAM_BETAS, sr.ADAM_EPS, wd, step, grad_scale=gs)
    tag = f"n={n} step={step} wd={wd} grad_scale={gs}"
    within(M[:n], ref["m"], sr.bound(8, ref["mm"]), "adam m " + tag)
    within(V[:n], ref["v"], sr.bound(8, ref["mv"]), "adam v " + tag)
    within(P[:n], ref["p"], sr.bound(8, ref["mp"]), "adam p " + tag)
    for t in (P, Gr, M, V):
        assert np.array_equal(host(t[n:]), pad)
    assert np.array_equal(host(Gr[:n]), g)


def test_adam_refuses_a_misaligned_buffer(dev):
    from onet_amd import _lib, ops
    n = 1023
    p, g, m, v = sr.adam_case(n)
    for moved in range(4):
        bufs = [T(np.concatenate([np.zeros(1, np.float32), t])).to(dev) for t in (p, g, m, v)]
        views = [b[1:] if k == moved else b[:n] for k, b in enumerate(bufs)]
        before = [b.clone() for b in bufs]
        with pytest.raises(_lib.OnetHipError, match="16-byte aligned"):
            ops.adam_step(*views, sr.ADAM_LR, *sr.ADAM_BETAS, sr.ADAM_EPS, 0.0, 1)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, bufs))
