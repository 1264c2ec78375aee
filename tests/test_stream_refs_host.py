"""The references and bounds of tests/stream_refs.py are neither wrong nor tuned to the kernels (no GPU needed).

Each reference is held against PyTorch's own CPU operator: F.max_pool2d with autograd, F.interpolate(align_corners=True) forward and
backward in float32, torch.softmax / sigmoid with autograd in float64 for the head, torch.optim.Adam in float64, F.pixel_shuffle /
F.pixel_unshuffle for the placement, and the tables tests/golden/log1pexp.npz and loss_extreme.npz (written by the real reference
model) for the quirk function and the loss.

And each bound of tests/test_gpu_stream_kernels.py is shown to be one that CORRECT fp32 arithmetic meets, on that file's own inputs:
the float32 CPU operator (where there is none, a float32 NumPy evaluation of the formula) lies within the bound of the fp64
reference.  The head's bound is also shown to have teeth: the textbook softmax backward in float32 breaks it on the sweep inputs."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_refs as sr

U, FLOOR = sr.U, sr.FLOOR
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = torch.from_numpy


within = sr.within


# ---------------------------------------------------------------------------------------------------------------- pooling
POOL_SHAPES = ((2, 3, 9, 11), (1, 4, 7, 10), (2, 5, 2, 2), (1, 64, 130, 34), (2, 4, 8, 16), (2, 4, 8, 18), (2, 4, 9, 16))


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_refs_match_aten(shape):
    x = sr.pool_input(*shape)
    xt = T(x).double().requires_grad_(True)
    y = F.max_pool2d(xt, 2)
    assert np.array_equal(sr.maxpool2_fwd(x), y.detach().numpy())
    dy, add, add2, old = (sr.normal(*s, seed=k) for k, s in ((2, y.shape), (3, shape), (4, shape), (5, shape)))
    y.backward(T(dy).double())
    g = xt.grad.numpy()
    Ho, Wo = shape[2] // 2, shape[3] // 2
    for a, a2, o in ((None, None, None), (add, None, None), (add, add2, None), (None, None, old)):
        dx, mag = sr.maxpool2_bwd(x, dy, a, a2, o)
        want, got32 = g.copy(), g.astype(np.float32)
        for t in (a, a2, o):
            if t is not None:
                want = want + t.astype(np.float64)
                got32 = got32 + t                                   # float32, the kernel's order
        assert np.array_equal(dx, want)
        within(got32, dx, sr.bound(4, mag), "pool bwd fp32")
        if a is None and o is None:
            assert not dx[:, :, 2 * Ho:, :].any() and not dx[:, :, :, 2 * Wo:].any() and not mag[:, :, 2 * Ho:, :].any()
    # ties: the all-equal window routes to its first element
    assert (g[..., 2 * Ho - 2, 2 * Wo - 2] == dy[..., Ho - 1, Wo - 1]).all() and not g[..., 2 * Ho - 1, 2 * Wo - 1].any()


# ---------------------------------------------------------------------------------------------------------------- placement
@pytest.mark.parametrize("geom", sr.PLACE)
def test_placement_refs_match_aten(geom):
    h, w, Ho, Wo, pt, pl = geom
    sub, bias, dy = sr.place_case(h, w, Ho, Wo)
    B, C4 = sub.shape[:2]
    C = C4 // 4
    ours = T(sub).reshape(B, 4, C, h, w).transpose(1, 2).reshape(B, 4 * C, h, w)          # F.pixel_shuffle: channel co * 4 + q
    for b in (None, bias):
        up = F.pixel_shuffle(ours, 2)
        if b is not None:
            up = up + T(b)[None, :, None, None]
        want = F.pad(up, (pl, Wo - 2 * w - pl, pt, Ho - 2 * h - pt))
        assert np.array_equal(sr.pixel_shuffle2_bias(sub, b, Ho, Wo, pt, pl), want.numpy())
    win = T(dy)[:, :, pt:pt + 2 * h, pl:pl + 2 * w]
    want = F.pixel_unshuffle(win, 2).reshape(B, C, 4, h, w).transpose(1, 2).reshape(B, 4 * C, h, w)
    assert np.array_equal(sr.space_to_depth2(dy, h, w, pt, pl), want.numpy())
    # the gather undoes the shuffle
    assert np.array_equal(sr.space_to_depth2(sr.pixel_shuffle2_bias(sub, None, Ho, Wo, pt, pl), h, w, pt, pl), sub)
    db, mag = sr.convT_dbias(dy, h, w, pt, pl)
    np.testing.assert_allclose(db, win.double().sum((0, 2, 3)).numpy(), rtol=0, atol=1e-13)
    within(win.double().sum((0, 2, 3)).float().numpy(), db, sr.bound(4, mag), "dbias summed in fp64, rounded once")


def test_elementwise_refs():
    x = sr.normal(1000, seed=41)
    y = sr.normal(1000, seed=42)
    for a in (1.0, -0.37):
        ref, mag = sr.axpy(a, x)
        within((np.float32(a) * x), ref, sr.bound(2, mag), "axpy")
        ref, mag = sr.axpy(a, x, y)
        within(y + np.float32(a) * x, ref, sr.bound(2, mag), "axpy accumulate")
        within(np.float32(np.float64(np.float32(a)) * x + y), ref, sr.bound(2, mag), "axpy accumulate, contracted to an fma")
    xc = np.array([0.0, 1.0, 0.1, 1.1, -0.0, 0.5, 2.0, -1.0, 1.1 + 2.0 ** -20, 0.1 - 2.0 ** -24], np.float32)
    got = sr.complement_clip(xc, 0.1)
    want = torch.clip(1 - T(xc) + 0.1, 0, 1).numpy()
    assert np.array_equal(got, want) and got[3] == 0 and got[2] == 1


# ---------------------------------------------------------------------------------------------------------------- bilinear
@pytest.mark.parametrize("hw", sr.BIL_HW)
def test_bilinear_refs_match_aten_fp32(hw):
    """float32 F.interpolate lies within 3.2 u (forward) and 4.8 u (backward; 4.5 u on these inputs) of the fp64 reference with the
    float32 source index: the bounds 8 u and 16 u leave a different summation order a factor 2 - 4, no more"""
    h, w = hw
    for A, n in ((sr.bil_matrix(h, 2 * h), h), (sr.bil_matrix(w, 2 * w), w)):
        assert A.shape == (2 * n, n) and (A >= 0).all() and np.abs(A.sum(1) - 1).max() < 1e-15 and ((A > 0).sum(1) <= 2).all()
    for Ho, Wo, pt, pl in sr.bil_geoms(h, w):
        x, g = sr.bil_case(h, w, Ho, Wo)
        xt = T(x).requires_grad_(True)
        y = F.pad(F.interpolate(xt, size=(2 * h, 2 * w), mode="bilinear", align_corners=True), (pl, Wo - 2 * w - pl, pt, Ho - 2 * h - pt))
        y.backward(T(g))
        ref, mag = sr.bilinear2x_fwd(x, Ho, Wo, pt, pl)
        rf = within(y.detach().numpy(), ref, sr.bound(3.2, mag), f"bilinear fwd {hw}")
        border = np.ones((Ho, Wo), bool)
        border[pt:pt + 2 * h, pl:pl + 2 * w] = False
        assert not ref[:, :, border].any() and not mag[:, :, border].any()
        dref, dmag = sr.bilinear2x_bwd(g, h, w, pt, pl)
        rb = within(xt.grad.numpy(), dref, sr.bound(4.8, dmag), f"bilinear bwd {hw}")
        print(f"bilinear {hw} {(Ho, Wo, pt, pl)}: fp32 ATen at {3.2 * rf:.2f} u fwd, {4.8 * rb:.2f} u bwd")
        # the reference's adjoint identity, fp64
        lhs, rhs = float((dref * x.astype(np.float64)).sum()), float((g.astype(np.float64) * ref).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((np.abs(g) * mag).sum())


# ---------------------------------------------------------------------------------------------------------------- head
HEAD_CASES = sr.HEAD_CASES
head_fwd_bounds, head_bwd_bound = sr.head_fwd_bounds, sr.head_bwd_bound


def head_fwd32(c):
    """the head forward in float32 NumPy, channel after channel (no fma)"""
    Ht, Hd = (sr.norm_relu32(c["Ht"], c["nt"]), sr.norm_relu32(c["Hd"], c["nd"])) if "nt" in c else (c["Ht"], c["Hd"])
    Vt, Vd = np.zeros_like(c["Lt"][:, 0]), np.zeros_like(c["Lt"][:, 0])
    sLt, sLd = np.zeros_like(Vt), np.zeros_like(Vt)
    for ch in range(c["Lt"].shape[1]):
        Vt, Vd = Vt + c["Lt"][:, ch] * Ht[:, ch], Vd + c["Ld"][:, ch] * Hd[:, ch]
        sLt, sLd = sLt + c["Lt"][:, ch], sLd + c["Ld"][:, ch]
    S = torch.softmax(torch.stack([T(Vt), T(Vd)], 1), 1).numpy()
    return Vt, Vd, S, sLt, sLd


@pytest.mark.parametrize("C,HW,norm", HEAD_CASES)
def test_head_forward_ref_and_bounds(C, HW, norm):
    c = sr.head_case(C, HW, norm=norm)
    ref = sr.head_fwd(c["Lt"], c["Ht"], c["Ld"], c["Hd"], c.get("nt"), c.get("nd"))
    d = ref["Vt"] - ref["Vd"]
    # the sweep does its job: both ends of S, and several hundred pixels where S is neither rounded to 1 nor underflowed
    s32 = ref["S"].astype(np.float32)
    assert d.min() < -110 and d.max() > 110 and (s32[:, 0] == 1).any() and (s32[:, 1] == 1).any() and (s32 == 0).any()
    assert ((np.abs(d) >= 17) & (np.abs(d) <= 80)).sum() >= 300
    # torch in float64
    Ht, Hd = ref["Ht"], ref["Hd"]
    if norm:                                                         # the rectified activation against torch's float32 operators
        for H, z, k in ((Ht, c["Ht"], "nt"), (Hd, c["Hd"], "nd")):
            mean, sc, sh = (T(c[k][i])[None, :, None] for i in (0, 2, 3))
            np.testing.assert_allclose(H, torch.relu((T(z) - mean) * sc + sh).numpy(), rtol=0, atol=4 * U * (1 + float(np.abs(H).max())))
    Vt = (T(c["Lt"]).double() * T(Ht)).sum(1)
    Vd = (T(c["Ld"]).double() * T(Hd)).sum(1)
    S = torch.softmax(torch.stack([Vt, Vd], 1), 1)
    np.testing.assert_allclose(ref["Vt"], Vt.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["S"], S.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref["sLt"], T(c["Lt"]).double().sum(1).numpy(), rtol=0, atol=1e-12)
    # float32 arithmetic meets the bounds
    bVt, bVd, bS = head_fwd_bounds(ref, C)
    v32t, v32d, S32, sLt, sLd = head_fwd32(c)
    within(v32t, ref["Vt"], bVt, "Vt fp32")
    within(v32d, ref["Vd"], bVd, "Vd fp32")
    within(S32, ref["S"], bS, "S fp32")
    within(sLt, ref["sLt"], sr.bound(C, ref["msLt"]), "sLt fp32")
    within(sLd, ref["sLd"], sr.bound(C, ref["msLd"]), "sLd fp32")
    assert np.array_equal(sLt, sr.channel_sums32(c["Lt"]))


def head_bwd32(c, S32, dVt, dVd, dS, gst, gsd, Ht, Hd):
    """the backward in float32 NumPy, the cancellation-free expression"""
    z = np.zeros_like(S32[:, 0])
    gt, gd = (z if dVt is None else dVt), (z if dVd is None else dVd)
    if dS is not None:
        t = S32[:, 0] * S32[:, 1] * (dS[:, 0] - dS[:, 1])
        gt, gd = gt + t, gd - t
    at, ad = (0 if gst is None else gst[:, None]), (0 if gsd is None else gsd[:, None])
    return dict(gt=gt, gd=gd, dLt=gt[:, None] * Ht + at, dHt=gt[:, None] * c["Lt"], dLd=gd[:, None] * Hd + ad, dHd=gd[:, None] * c["Ld"])


@pytest.mark.parametrize("C,HW,norm", HEAD_CASES)
def test_head_backward_ref_and_bounds(C, HW, norm):
    c = sr.head_case(C, HW, norm=norm)
    fwd = sr.head_fwd(c["Lt"], c["Ht"], c["Ld"], c["Hd"], c.get("nt"), c.get("nd"))
    S32 = fwd["S"].astype(np.float32)
    Ht32, Hd32 = fwd["Ht"].astype(np.float32), fwd["Hd"].astype(np.float32)
    # (1) the reference against float64 autograd of torch.softmax on the exact S (full chain; the textbook form torch evaluates
    # cancels in fp64 too, hence the absolute slack) ...
    L = [T(c[k]).double().requires_grad_(True) for k in ("Lt", "Ld")]
    H = [T(fwd[k]).clone().requires_grad_(True) for k in ("Ht", "Hd")]
    Vt, Vd = (L[0] * H[0]).sum(1), (L[1] * H[1]).sum(1)
    S = torch.softmax(torch.stack([Vt, Vd], 1), 1)
    loss = (Vt * T(c["dVt"])).sum() + (Vd * T(c["dVd"])).sum() + (S * T(c["dS"])).sum() + (L[0].sum(1) * T(c["gst"])).sum() + \
        (L[1].sum(1) * T(c["gsd"])).sum()
    loss.backward()
    ref = sr.head_bwd(c["dVt"], c["dVd"], c["dS"], fwd["S"], c["Lt"], c["Ht"], c["Ld"], c["Hd"], c["gst"], c["gsd"], c.get("nt"), c.get("nd"))
    for name, t in (("dLt", L[0]), ("dHt", H[0]), ("dLd", L[1]), ("dHd", H[1])):
        slack = 1e-14 * (ref["m" + name] + ref["f" + name] * (np.abs(c["dS"]).sum(1)[:, None, :] + 1))
        assert (np.abs(ref[name] - t.grad.numpy()) <= slack).all(), name
    # ... and (2) its small elements against autograd of torch.sigmoid on the side where that is free of cancellation:
    # St = sigmoid(x), x = Vt - Vd, d St / dx = y (1 - y) with y = sigmoid(-|x|) tiny and 1 - y exact enough
    x = T(fwd["Vt"] - fwd["Vd"]).requires_grad_(True)
    y = torch.sigmoid(-x.abs())
    (y * T(c["dS"][:, 0].astype(np.float64) - c["dS"][:, 1])).sum().backward()          # d/dx = -sign(x) (a - d) y (1 - y)
    only_s = sr.head_px_grad(None, None, c["dS"], fwd["S"])
    nz = x.detach().numpy() != 0                                      # (|x| has no derivative at the sweep's exact middle)
    np.testing.assert_allclose(only_s[0][nz], (-np.sign(x.detach().numpy()) * x.grad.numpy())[nz], rtol=1e-12, atol=0)
    assert np.array_equal(only_s[0], -only_s[1])
    # (3) float32 arithmetic on the float32 S meets the per-element bound, for every combination of upstream gradients
    for dVt, dVd, dS in ((c["dVt"], c["dVd"], c["dS"]), (None, None, c["dS"]), (c["dVt"], None, None), (None, c["dVd"], c["dS"])):
        for gst, gsd in ((c["gst"], c["gsd"]), (None, None)):
            ref = sr.head_bwd(dVt, dVd, dS, S32, c["Lt"], c["Ht"], c["Ld"], c["Hd"], gst, gsd, c.get("nt"), c.get("nd"))
            got = head_bwd32(c, S32, dVt, dVd, dS, gst, gsd, Ht32, Hd32)
            for name in got:
                within(got[name], ref[name], head_bwd_bound(ref, name), f"{name} fp32")


@pytest.mark.parametrize("C,HW,norm", HEAD_CASES[:3])
def test_textbook_softmax_backward_breaks_the_bound(C, HW, norm):
    """the guard: were head_px_grad the textbook St (a - (a St + d Sd)), the per-element bound would catch it on these inputs"""
    c = sr.head_case(C, HW, norm=norm)
    S32 = sr.head_fwd(c["Lt"], c["Ht"], c["Ld"], c["Hd"])["S"].astype(np.float32)
    gt, _, mgt, _, amd = sr.head_px_grad(None, None, c["dS"], S32)
    err = np.abs(sr.textbook_softmax_bwd32(c["dS"], S32).astype(np.float64) - gt)
    bad = err > sr.bound(8, mgt, FLOOR * amd)
    assert bad.sum() >= 300, int(bad.sum())
    # ... while a max-scaled check (the largest element sets the scale) would let it pass at 1e-6
    assert err.max() <= 1e-6 * np.abs(gt).max()


# ---------------------------------------------------------------------------------------------------------------- loss
def test_quirk_function_against_the_reference_models_table():
    g = np.load(os.path.join(G, "log1pexp.npz"))
    x = g["x"]
    f, df = sr.f_quirk32(x), sr.df_quirk32(x)
    within(g["y"], f, sr.bound(4, np.maximum(1, np.abs(f))), "f: the reference model (torch fp32)")
    within(g["dy"], df, sr.bound(4, np.abs(df), FLOOR), "df: the reference model (torch fp32)")
    # the four branches, and the quirks themselves
    assert abs(float(sr.f_quirk32(-50.0)) - np.log(2)) < 1e-7 and float(sr.f_quirk32(-17.0)) == 0 and float(sr.f_quirk32(-16.0)) > 0
    assert float(sr.f_quirk32(40.0)) == 40 and float(sr.df_quirk32(40.0)) == 1 and float(sr.f_quirk32(np.float32(33.3))) == np.float32(33.3)
    pts = sr.quirk_points()
    assert len(pts) >= 25 and len(set(pts.tolist())) >= len(pts) - 2 and np.isfinite(sr.f_quirk32(pts)).all() and np.isfinite(sr.df_quirk32(pts)).all()
    xt = T(pts.copy())
    for lo, hi, fn, dfn in ((-np.inf, -37, lambda v: torch.log(1 + torch.exp(torch.exp(v))), lambda v: torch.exp(torch.exp(v)) / (1 + torch.exp(torch.exp(v))) * torch.exp(v)),
                            (-37, 18, lambda v: torch.log(1 + torch.exp(v)), lambda v: torch.exp(v) / (1 + torch.exp(v))),
                            (18, 33.3, lambda v: v + torch.exp(-v), lambda v: 1 - torch.exp(-v))):
        sel = (pts > np.float32(lo)) & (pts <= np.float32(hi)) if hi != 33.3 else (pts > np.float32(18)) & (pts < np.float32(33.3))
        fr, dfr = sr.f_quirk32(pts[sel]), sr.df_quirk32(pts[sel])
        within(fn(xt[sel]).numpy(), fr, sr.bound(4, np.maximum(1, np.abs(fr))), "f: torch fp32 on the edge points")
        within(dfn(xt[sel]).numpy(), dfr, sr.bound(4, np.abs(dfr), FLOOR), "df: torch fp32 on the edge points")


def quirk32(v):
    """f and df in torch float32, every branch evaluated and selected"""
    e = torch.exp(v)
    ee = torch.exp(e)
    f = torch.where(v <= -37, torch.log(1 + ee), torch.where(v <= 18, torch.log(1 + e), torch.where(v < 33.3, v + torch.exp(-v), v)))
    df = torch.where(v <= -37, ee / (1 + ee) * e, torch.where(v <= 18, e / (1 + e), torch.where(v < 33.3, 1 - torch.exp(-v), torch.ones_like(v))))
    return f, df


def test_quirk_bounds_on_the_random_arguments():
    """The emulation rounds exp and log correctly; a float32 library need not.  On the GPU test's two million random arguments PyTorch's
    own float32 functions stay within 4 u, f and df both (the derivative is held to 4 u everywhere).  With exp one and log two floats
    off, every evaluation of f stays within K_QUIRK = 8 u max(1, |f|) of the emulation -- and the pair (-1, -2) leaves 4 u: for such a
    library 4 u is too tight, 8 u is not."""
    x = np.concatenate([sr.quirk_points(), sr.rng(81).uniform(-60, 60, 8192 * 256 + 1000).astype(np.float32)])
    f, df = sr.f_quirk32(x), sr.df_quirk32(x)
    assert sr.K_QUIRK == 8
    for dexp in (-1, 1):
        for dlog in (-2, 2):
            within(sr.f_quirk32(x, dexp, dlog), f, sr.bound(sr.K_QUIRK, np.maximum(1, np.abs(f))), "f with exp one and log two floats off")
    over4 = np.abs(sr.f_quirk32(x, -1, -2).astype(np.float64) - f) > sr.bound(4, np.maximum(1, np.abs(f)))
    assert over4.any() and ((x[over4] > -2) & (x[over4] < 18)).all()
    t, d = quirk32(T(x.copy()))
    within(t.numpy(), f, sr.bound(4, np.maximum(1, np.abs(f))), "f: torch fp32")
    within(d.numpy(), df, sr.bound(4, np.abs(df), FLOOR), "df: torch fp32")


def test_loss_against_the_reference_models_extreme_case():
    g = np.load(os.path.join(G, "loss_extreme.npz"))
    B, C, H, W = g["Lt"].shape
    S = torch.softmax(torch.cat([T(g["Vt"]), T(g["Vd"])], 1), 1).numpy().reshape(B, 2, H * W)
    sums = [sr.channel_sums32(g[k].reshape(B, C, H * W)) for k in ("Lt", "Ld")]
    j1, m1 = sr.jsd_fwd(sums[0], S[:, 0], S[:, 1])
    j2, m2 = sr.jsd_fwd(sums[1], S[:, 1], S[:, 0])
    loss = -(j1 + j2) / 2
    assert abs(loss - float(g["loss"])) <= 8 * U * (m1 + m2) / 2 + 2 * U * abs(loss), (loss, float(g["loss"]))
    b1, b2 = sr.jsd_bwd(-0.5, sums[0], S[:, 0], S[:, 1]), sr.jsd_bwd(-0.5, sums[1], S[:, 1], S[:, 0])
    n = B * H * W
    for k, b in (("dLt", b1), ("dLd", b2)):
        got = g[k].reshape(B, C, H * W)
        assert np.array_equal(got, np.broadcast_to(got[:, :1], got.shape))
        within(got[:, 0].reshape(n), b["gL"], sr.bound(8, b["mgL"], FLOOR), k)
    dS = np.stack([(b1["dSi"] + b2["dSp"]).reshape(B, H * W), (b1["dSp"] + b2["dSi"]).reshape(B, H * W)], 1)
    gt, gd, mgt, mgd, amd = sr.head_px_grad(None, None, dS, S)
    # (torch's float32 autograd evaluates the textbook softmax backward: its error is relative to that form's terms)
    a, d = np.abs(dS[:, 0]), np.abs(dS[:, 1])
    within(g["dVt"].reshape(B, H * W), gt, 16 * U * S[:, 0] * (a + a * S[:, 0] + d * S[:, 1]) + FLOOR, "dVt")
    within(g["dVd"].reshape(B, H * W), gd, 16 * U * S[:, 1] * (d + a * S[:, 0] + d * S[:, 1]) + FLOOR, "dVd")


@pytest.mark.parametrize("C,B,HW", sr.JSD_CASES)
def test_jsd_bounds_hold_for_fp32(C, B, HW):
    """the scalar and the three gradients in torch float32 (exp, log and the division of PyTorch's CPU library) on the GPU test's inputs"""
    L, S = sr.jsd_case(C, B, HW)
    n = B * HW
    sums = sr.channel_sums32(L)
    ref, mean_abs = sr.jsd_fwd(sums, S[:, 0], S[:, 1])
    t, a1, a2 = sr.jsd_terms(sums, S[:, 0], S[:, 1])
    assert n < 100 or all(((a1 <= lo) | (a2 <= lo)).any() and ((a1 > hi) | (a2 > hi)).any() for lo, hi in ((-37, -37), (18, 18), (-37, 33.3)))
    assert B == 1 or not np.array_equal(S[0], S[1])
    sl, si, sp = (T(np.ascontiguousarray(v).reshape(-1)) for v in (sums, S[:, 0], S[:, 1]))
    x1, x2 = -(sl * si), sl * sp
    assert np.array_equal(x1.numpy(), a1) and np.array_equal(x2.numpy(), a2)
    (f1, d1), (f2, d2) = quirk32(x1), quirk32(x2)
    got = -float((f1 + f2).double().mean())
    assert abs(got - ref) <= 8 * U * mean_abs, (got, ref)
    for gscale in (1.0, -0.37):
        b = sr.jsd_bwd(gscale, sums, S[:, 0], S[:, 1])
        g = -torch.tensor(gscale, dtype=torch.float32) * torch.tensor(1.0 / n, dtype=torch.float32)
        for name, v in (("gL", g * (-si * d1 + sp * d2)), ("dSi", g * (-sl * d1)), ("dSp", g * (sl * d2))):
            within(v.numpy(), b[name], sr.bound(8, b["m" + name], FLOOR), f"jsd_bwd {name} in float32, gscale={gscale}")


# ---------------------------------------------------------------------------------------------------------------- Adam
def torch_adam(p, g, m, v, step, wd, gs, dtype):
    pt = T(p).to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=sr.ADAM_LR, betas=sr.ADAM_BETAS, eps=sr.ADAM_EPS, weight_decay=wd)
    opt.state[pt] = dict(step=torch.tensor(float(step - 1)), exp_avg=T(m).to(dtype).clone(), exp_avg_sq=T(v).to(dtype).clone())
    pt.grad = (T(g).double() * gs).to(dtype)                          # gs is a power of two: exact
    opt.step()
    st = opt.state[pt]
    return dict(p=pt.detach().numpy(), m=st["exp_avg"].numpy(), v=st["exp_avg_sq"].numpy())


@pytest.mark.parametrize("n,hyper", sr.ADAM_CASES)
def test_adam_ref_and_bounds(n, hyper):
    step, wd, gs = hyper
    p, g, m, v = sr.adam_case(n)
    assert n < 8 or ((g == 0) & (v == 0)).any()
    ref = sr.adam_step(p, g, m, v, sr.ADAM_LR, *sr.ADAM_BETAS, sr.ADAM_EPS, wd, step, gs)
    if n <= 10007:
        t64 = torch_adam(p, g, m, v, step, wd, gs, torch.float64)
        for k in "pmv":
            np.testing.assert_allclose(ref[k], t64[k], rtol=1e-12, atol=1e-300)
    bnd = dict(p=sr.bound(8, ref["mp"]), m=sr.bound(8, ref["mm"]), v=sr.bound(8, ref["mv"]))
    emu = sr.adam_step32(p, g, m, v, sr.ADAM_LR, *sr.ADAM_BETAS, sr.ADAM_EPS, wd, step, gs)
    worst = {k: 8 * within(emu[k], ref[k], bnd[k], f"{k}: float32 emulation") for k in "pmv"}
    # the margin the 8 u bounds leave a kernel's own order of operations: the emulation sits at <= 3.2 / 6.3 / 6.0 u (m / v / p) here
    assert worst["m"] <= 4 and worst["v"] <= 7 and worst["p"] <= 6.5, worst
    print(f"adam n={n} {hyper}: float32 emulation at {worst['m']:.2f} / {worst['v']:.2f} / {worst['p']:.2f} u (m / v / p)")
    if n <= 10007:
        t32 = torch_adam(p, g, m, v, step, wd, gs, torch.float32)
        for k in "pmv":
            within(t32[k], ref[k], bnd[k], f"{k}: torch float32 Adam")


def test_adam_bound_sees_a_complement_formed_in_float32():
    """1.f - 0.999f is 1.3e-5 (relative) away from 0.001: two hundred ulps of the second moment where g^2 dominates it, as in the first steps.  The bound on v
    must not let that through (the kernel once formed 1 - beta from the rounded beta)."""
    p, g, m, v = sr.adam_case(10007)
    ref = sr.adam_step(p, g, m, v, sr.ADAM_LR, *sr.ADAM_BETAS, sr.ADAM_EPS, 0.0, 1, 1.0)
    b2 = np.float32(sr.ADAM_BETAS[1])
    wrong = b2 * v + (np.float32(1) - b2) * g * g
    early = slice(10007 - 10007 // 8, 10007)
    assert (np.abs(wrong - ref["v"]) > sr.bound(8, ref["mv"]))[early].mean() > 0.9


def test_adam_f64_entry_is_declared_exported_and_beside_the_float_one():
    """onet_adam_step_f64 lives in a header of its own (doubles for lr, the betas, eps and the decay); onet_hip.h keeps the float
    prototype, its 108 entry points and the ABI its version"""
    import ctypes
    from onet_amd import _lib
    lib = _lib.load()
    protos = _lib.parse_header(_lib.OPTIM_HEADER)
    assert list(protos) == ["onet_adam_step_f64"] and hasattr(lib, "onet_adam_step_f64")
    _, types, names = protos["onet_adam_step_f64"]
    assert names == ["p", "g", "m", "v", "n", "lr", "beta1", "beta2", "eps", "weight_decay", "step", "grad_scale", "stream"]
    assert [t for t, n in zip(types, names) if n in ("lr", "beta1", "beta2", "eps", "weight_decay")] == [ctypes.c_double] * 5
    main = _lib.parse_header()
    assert len(main) == 108 and lib.onet_abi_version() == 4
    _, types, names = main["onet_adam_step"]
    assert names == protos["onet_adam_step_f64"][2] and [t for t, n in zip(types, names) if n in ("lr", "beta1", "beta2")] == [ctypes.c_float] * 3
    # bad arguments are an error code before any launch, from both
    assert lib.onet_adam_step_f64(None, None, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None) != 0
    assert lib.onet_adam_step(None, None, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None) != 0
