"""Plain fp64 references of the streaming kernels (onet_amd/csrc/spatial.hip, head_loss.hip, optim.hip) and the inputs their tests
share.  NumPy only, no project imports: tests/test_stream_refs_host.py holds every function here against PyTorch's own CPU operator
(and shows that correct fp32 arithmetic meets each bound), tests/test_gpu_stream_kernels.py holds the kernels against them.

A reference returns its value in float64 and, where a bound needs it, a MAGNITUDE array: the same formula on absolute values.  Every
per-element bound has the form |got - ref| <= k * U * mag + FLOOR (bound() below); FLOOR only where a result can be subnormal.

Two references are not fp64 formulas, because the operation is DEFINED in fp32:
  * the bilinear source index is ATen's, in float32: scale = float(in - 1) / float(out - 1), s = scale * o.  Its fractional part carries
    about 2 h 2^-23 of rounding, so the exact-rational index is a different function at large h.  The interpolation itself is fp64.
  * f_quirk / df_quirk (the reference model's order-dependent log1pexp): log(1 + exp(x)) is 0 below about -16.6 only
    because 1 + e rounds, so each operation is rounded to float32 (computed in fp64, rounded once) and the branch is chosen on the
    float32 argument.  Sums over pixels are fp64."""
import numpy as np

U = 2.0 ** -24            # unit roundoff of float32
FLOOR = 2.0 ** -126       # smallest normal float32: the slack of a result that may be flushed

F32, F64 = np.float32, np.float64


def bound(k, mag, floor=0.0):
    return k * U * np.asarray(mag, F64) + floor


def r32(x):
    """round an fp64 result to float32 (one operation of an fp32 emulation)"""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(x, F64).astype(F32)


def rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def normal(*shape, seed=0, scale=1.0):
    return (rng(seed, *shape).standard_normal(shape) * scale).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- max-pooling
def pool_input(B, C, H, W, seed=1):
    """ReLU'd data (exact zeros: ties), a zeroed 4 x 4 corner, and the last full window of every plane with the maximum in all four
    positions (the second-last one with it in the two positions of its lower row): the first in scan order must win"""
    x = np.maximum(normal(B, C, H, W, seed=seed), 0)
    x[..., :4, :4] = 0
    Ho, Wo = H // 2, W // 2
    x[..., 2 * Ho - 2:2 * Ho, 2 * Wo - 2:2 * Wo] = 7.5
    if Wo > 1:
        x[..., 2 * Ho - 1, 2 * Wo - 4:2 * Wo - 2] = 6.25
    return x


def _windows(x):
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    return x[..., :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)   # scan order


def maxpool2_fwd(x):
    """MaxPool2d(2), floor semantics: the odd last row and column are dropped.  A selection: exact."""
    return _windows(np.asarray(x)).max(-1)


def maxpool2_bwd(x, dy, add=None, add2=None, old=None):
    """-> (dx, mag): dy routed to the FIRST maximum of each window in scan order, + add + add2 (+ old dx); zero where no window is"""
    x = np.asarray(x)
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    am = _windows(x).argmax(-1)                                  # first occurrence
    onehot = (am[..., None] == np.arange(4)).astype(F64) * np.asarray(dy, F64)[..., None]
    dx = np.zeros((B, C, H, W), F64)
    dx[..., :2 * Ho, :2 * Wo] = onehot.reshape(B, C, Ho, Wo, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * Ho, 2 * Wo)
    mag = np.abs(dx)
    for t in (add, add2, old):
        if t is not None:
            dx = dx + np.asarray(t, F64)
            mag = mag + np.abs(np.asarray(t, F64))
    return dx, mag


# ---------------------------------------------------------------------------------------------------------------- placement
def pixel_shuffle2_bias(sub, bias, Ho, Wo, pt, pl):
    """sub [B, 4C, h, w] (sub-pixel plane q = 2 dy + dx holds channels q C .. q C + C) -> float32 [B, C, Ho, Wo]: the 2h x 2w shuffle
    (+ bias: one float32 addition) at (pt, pl), zero border.  Exact."""
    sub = np.asarray(sub, F32)
    B, C4, h, w = sub.shape
    C = C4 // 4
    y = np.zeros((B, C, Ho, Wo), F32)
    for q in range(4):
        v = sub[:, q * C:(q + 1) * C]
        if bias is not None:
            v = v + np.asarray(bias, F32)[None, :, None, None]
        y[:, :, pt + (q >> 1):pt + 2 * h:2, pl + (q & 1):pl + 2 * w:2] = v
    return y


def space_to_depth2(dy, h, w, pt, pl):
    """the gather that undoes pixel_shuffle2_bias: [B, C, Ho, Wo] -> [B, 4C, h, w].  Exact."""
    dy = np.asarray(dy)
    return np.concatenate([dy[:, :, pt + (q >> 1):pt + 2 * h:2, pl + (q & 1):pl + 2 * w:2] for q in range(4)], 1)


def convT_dbias(dy, h, w, pt, pl):
    """-> (dbias [C], mag): the sum of dy over the batch and the un-padded 2h x 2w window"""
    win = np.asarray(dy, F64)[:, :, pt:pt + 2 * h, pl:pl + 2 * w]
    return win.sum((0, 2, 3)), np.abs(win).sum((0, 2, 3))


def axpy(a, x, y=None):
    """-> (a x (+ y), mag)"""
    ax = float(np.float32(a)) * np.asarray(x, F64)
    if y is None:
        return ax, np.abs(ax)
    return ax + np.asarray(y, F64), np.abs(ax) + np.abs(np.asarray(y, F64))


def complement_clip(x, bias):
    """clip(1 - x + bias, 0, 1): two float32 additions in this order and a selection.  Exact (float32)."""
    x = np.asarray(x, F32)
    return np.minimum(np.maximum((np.float32(1) - x) + np.float32(bias), np.float32(0)), np.float32(1))


# ---------------------------------------------------------------------------------------------------------------- bilinear x2
def bil_matrix(n_in, n_out):
    """[n_out, n_in] interpolation weights of one axis, align_corners=True, the source index as ATen defines it in float32"""
    scale = F32(0) if n_out <= 1 else F32(n_in - 1) / F32(n_out - 1)
    o = np.arange(n_out)
    s = (scale * o.astype(F32)).astype(F32)
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(F32)).astype(F64)            # exact
    A = np.zeros((n_out, n_in), F64)
    np.add.at(A, (o, i0), 1.0 - l1)
    np.add.at(A, (o, i1), l1)
    return A


def bilinear2x_fwd(x, Ho, Wo, pt, pl):
    """-> (y [B, C, Ho, Wo], mag): x up-sampled to 2h x 2w at (pt, pl), zero border; mag = sum |w| |x|"""
    x = np.asarray(x, F64)
    B, C, h, w = x.shape
    Ay, Ax = bil_matrix(h, 2 * h), bil_matrix(w, 2 * w)
    y, mag = np.zeros((B, C, Ho, Wo), F64), np.zeros((B, C, Ho, Wo), F64)
    y[:, :, pt:pt + 2 * h, pl:pl + 2 * w] = np.einsum("oi,bcij,pj->bcop", Ay, x, Ax, optimize=True)
    mag[:, :, pt:pt + 2 * h, pl:pl + 2 * w] = np.einsum("oi,bcij,pj->bcop", Ay, np.abs(x), Ax, optimize=True)
    return y, mag


def bilinear2x_bwd(g, h, w, pt, pl):
    """-> (dx [B, C, h, w], mag): the exact transpose of bilinear2x_fwd, the same weights; mag = sum |w| |g|"""
    gw = np.asarray(g, F64)[:, :, pt:pt + 2 * h, pl:pl + 2 * w]
    Ay, Ax = bil_matrix(h, 2 * h), bil_matrix(w, 2 * w)
    return (np.einsum("oi,bcop,pj->bcij", Ay, gw, Ax, optimize=True), np.einsum("oi,bcop,pj->bcij", Ay, np.abs(gw), Ax, optimize=True))


# ---------------------------------------------------------------------------------------------------------------- head
def norm_relu32(z, coef):
    """H = max(fma(z - mean, scale, shift), 0) in float32, as the producing unit's apply pass writes it; coef [4][C] = mean, invstd,
    scale, shift; z [B, C, HW]"""
    z = np.asarray(z, F32)
    mean, sc, sh = (np.asarray(coef[k], F32)[None, :, None] for k in (0, 2, 3))
    d = z - mean                                                     # one float32 rounding
    return np.maximum(r32(d.astype(F64) * sc.astype(F64) + sh.astype(F64)), F32(0))      # fma: the product of two floats is exact in fp64


def head_fwd(Lt, Ht, Ld, Hd, nt=None, nd=None):
    """L, H [B, C, HW] -> dict of V (Vt, Vd [B, HW]), S [B, 2, HW], channel sums sLt, sLd [B, HW] and the magnitudes mVt, mVd (sum
    |L H|), msLt, msLd (sum |L|).  nt / nd: Ht / Hd are pre-activations, normalised and rectified first (norm_relu32)."""
    if nt is not None:
        Ht, Hd = norm_relu32(Ht, nt), norm_relu32(Hd, nd)
    Lt, Ht, Ld, Hd = (np.asarray(t, F64) for t in (Lt, Ht, Ld, Hd))
    Vt, Vd = (Lt * Ht).sum(1), (Ld * Hd).sum(1)
    m = np.maximum(Vt, Vd)
    et, ed = np.exp(Vt - m), np.exp(Vd - m)
    S = np.stack([et / (et + ed), ed / (et + ed)], 1)
    return dict(Vt=Vt, Vd=Vd, S=S, mVt=np.abs(Lt * Ht).sum(1), mVd=np.abs(Ld * Hd).sum(1), sLt=Lt.sum(1), sLd=Ld.sum(1),
                msLt=np.abs(Lt).sum(1), msLd=np.abs(Ld).sum(1), Ht=Ht, Hd=Hd)


def head_px_grad(dVt, dVd, dS, S):
    """-> (gt, gd, mag, |a - d|) [B, HW]: the head's per-pixel gradients from the upstream gradients of Vt, Vd [B, HW] and S [B, 2, HW]
    (each may be None).  The 2-class softmax backward is St Sd (a - d) for Vt and its negative for Vd -- the Jacobian itself, which no
    rounding of St to 1 touches (the textbook St (a - (a St + d Sd)) is the same only while St + Sd = 1 holds to the last bit)."""
    B, _, HW = np.asarray(S).shape
    z = np.zeros((B, HW), F64)
    gt = z if dVt is None else np.asarray(dVt, F64)
    gd = z if dVd is None else np.asarray(dVd, F64)
    mt, md, amd = np.abs(gt), np.abs(gd), z
    if dS is not None:
        S, dS = np.asarray(S, F64), np.asarray(dS, F64)
        a, d = dS[:, 0], dS[:, 1]
        t = S[:, 0] * S[:, 1] * (a - d)
        mag_t = S[:, 0] * S[:, 1] * (np.abs(a) + np.abs(d))
        gt, gd, mt, md, amd = gt + t, gd - t, mt + mag_t, md + mag_t, np.abs(a - d)
    return gt, gd, mt, md, amd


def head_bwd(dVt, dVd, dS, S, Lt, Ht, Ld, Hd, gst=None, gsd=None, nt=None, nd=None):
    """-> dict: gt, gd (+ their magnitudes mgt, mgd, and amd = |a - d|), dLt = gt Ht + gst, dHt = gt Lt, dLd = gd Hd + gsd, dHd = gd Ld
    [B, C, HW], each with its magnitude m<name> and the factor f<name> that multiplies the pixel gradient (for the subnormal floor)"""
    if nt is not None:
        Ht, Hd = norm_relu32(Ht, nt), norm_relu32(Hd, nd)
    Lt, Ht, Ld, Hd = (np.asarray(t, F64) for t in (Lt, Ht, Ld, Hd))
    gt, gd, mgt, mgd, amd = head_px_grad(dVt, dVd, dS, S)
    out = dict(gt=gt, gd=gd, mgt=mgt, mgd=mgd, amd=amd)
    for name, g, mg, f, gs in (("dLt", gt, mgt, Ht, gst), ("dHt", gt, mgt, Lt, None), ("dLd", gd, mgd, Hd, gsd), ("dHd", gd, mgd, Ld, None)):
        add = 0.0 if gs is None else np.asarray(gs, F64)[:, None, :]
        out[name] = g[:, None, :] * f + add
        out["m" + name] = mg[:, None, :] * np.abs(f) + np.abs(add)
        out["f" + name] = np.abs(f)
    return out


def head_case(C, HW, B=2, seed=7, norm=False):
    """Inputs whose Vt - Vd sweeps -120 .. +120 across the pixels of each image (the second image backwards): channel 0 carries the
    sweep (H is a ReLU output: the losing side's H is 0), the rest are noise.  S rounds to 1 on one side and underflows on the other
    at both ends; more than half of the pixels lie in 17 <= |Vt - Vd| <= 80 where it does neither.  norm: Ht / Hd are pre-activations z
    and 'nt' / 'nd' the [4][C] coefficients that make (about) the same H of them."""
    g = rng(seed, C, HW, B)
    d = np.linspace(-120.0, 120.0, HW)
    d = np.stack([d if b % 2 == 0 else d[::-1] for b in range(B)])                     # [B, HW]
    f = lambda *s: g.standard_normal(s)
    Lt, Ld = 0.3 * f(B, C, HW), 0.3 * f(B, C, HW)
    Ht, Hd = 0.3 * np.maximum(f(B, C, HW), 0), 0.3 * np.maximum(f(B, C, HW), 0)
    l0t, l0d = np.sqrt(np.abs(d)) * g.uniform(0.5, 2.0, (B, HW)) + 0.25, np.sqrt(np.abs(d)) * g.uniform(0.5, 2.0, (B, HW)) + 0.25
    Lt[:, 0], Ld[:, 0] = l0t, l0d
    Ht[:, 0], Hd[:, 0] = np.maximum(d, 0) / l0t, np.maximum(-d, 0) / l0d
    case = dict(Lt=Lt, Ld=Ld, Ht=Ht, Hd=Hd)
    if norm:
        for k, n in (("Ht", "nt"), ("Hd", "nd")):
            coef = np.stack([0.1 * f(C), 1.0 + 0.05 * f(C), 1.0 + 0.1 * f(C), 0.1 * f(C)]).astype(F32)      # mean, invstd, scale, shift
            H = case[k]
            z = np.where(H > 0, (H - coef[3][None, :, None]) / coef[2][None, :, None], -(1.0 + np.abs(f(B, C, HW)))) + coef[0][None, :, None]
            case[k], case[n] = z, coef
    case = {k: np.ascontiguousarray(v, F32) for k, v in case.items()}
    case.update(dVt=normal(B, HW, seed=seed + 1, scale=1e-3), dVd=normal(B, HW, seed=seed + 2, scale=1e-3), dS=normal(B, 2, HW, seed=seed + 3),
                gst=normal(B, HW, seed=seed + 4, scale=1e-3), gsd=normal(B, HW, seed=seed + 5, scale=1e-3))
    return case


def textbook_softmax_bwd32(dS, S):
    """the textbook 2-class softmax backward St (a - (a St + d Sd)) in float32: what head_px_grad must NOT be (it loses everything once
    St rounds to 1)"""
    S, dS = np.asarray(S, F32), np.asarray(dS, F32)
    st, sd, a, d = S[:, 0], S[:, 1], dS[:, 0], dS[:, 1]
    return st * (a - (a * st + d * sd))


# ---------------------------------------------------------------------------------------------------------------- loss
def _ulps(r, d):
    """r moved d float32 values up (d > 0) or down: a library function that is accurate to |d| ulp instead of correctly rounded"""
    for _ in range(abs(d)):
        r = np.nextafter(r, F32(np.inf if d > 0 else -np.inf))
    return r


def _exp32(x, d=0):
    with np.errstate(over="ignore", under="ignore"):
        return _ulps(r32(np.exp(np.asarray(x, F32).astype(F64))), d)


def _log32(x, d=0):
    with np.errstate(divide="ignore"):
        return _ulps(r32(np.log(np.asarray(x, F32).astype(F64))), d)


def _add32(a, b):
    return r32(np.asarray(a, F32).astype(F64) + np.asarray(b, F32).astype(F64))


def _mul32(a, b):
    return r32(np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64))


def f_quirk32(x, dexp=0, dlog=0):
    """float32 emulation, operation by operation, of the effective function of the reference's log1pexp on the original x:
    x <= -37: log(1 + exp(exp(x)));  x <= 18: log(1 + exp(x));  x < 33.3f: x + exp(-x);  else x.
    Every operation correctly rounded; dexp / dlog = +-1: exp / log one ulp off instead, which a float32 library function may be
    (the bounds must hold for those too: test_stream_refs_host.py)"""
    x = np.asarray(x, F32)
    one = F32(1)
    e = _exp32(x, dexp)
    b1 = _log32(_add32(one, _exp32(e, dexp)), dlog)
    b2 = _log32(_add32(one, e), dlog)
    b3 = _add32(x, _exp32(-x, dexp))
    return np.where(x <= F32(-37), b1, np.where(x <= F32(18), b2, np.where(x < F32(33.3), b3, x))).astype(F32)


def df_quirk32(x, dexp=0):
    """the autograd derivative of the composed operations, likewise: ee / (1 + ee) * e;  e / (1 + e);  1 - exp(-x);  1"""
    x = np.asarray(x, F32)
    one = F32(1)
    e = _exp32(x, dexp)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        ee = _exp32(e, dexp)
        b1 = _mul32(r32(ee.astype(F64) / _add32(one, ee).astype(F64)), e)
        b2 = r32(e.astype(F64) / _add32(one, e).astype(F64))
        b3 = _add32(one, -_exp32(-x, dexp))
    return np.where(x <= F32(-37), b1, np.where(x <= F32(18), b2, np.where(x < F32(33.3), b3, one))).astype(F32)


# The quirk function on arbitrary arguments against its float32 emulation.  A float32 library's exp and log are not correctly rounded:
# take them accurate to 2 ulp (4 u relative at most), the emulation's to u.  Two such evaluations of log(1 + exp(x)) differ by up to
# 5 u e / (1 + e) (the two exp, through the sum and the logarithm) + 2 u (the two roundings of 1 + e) + 5 u |f| (the two logarithms); the
# three worst cases exclude one another (e / (1 + e) -> 1 needs |f| large, where the first two terms vanish against the third), and on
# the tests' arguments every evaluation with exp one and log two floats off stays within 8 u max(1, |f|), while the pair (-1, -2) leaves
# 4 u: test_stream_refs_host.py asserts both.  At the branch points, and for correctly rounded functions, 4 u holds.
K_QUIRK = 8


def neighbours(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


def quirk_points():
    """the three branch points with their two float32 neighbours each, +-0, the stretch -16.5 .. -17 where 1 + e stops rounding up (in
    decades of ulps: 1, 10, 100, ... ulps below -16.5), and the far ends"""
    pts = neighbours(-37.0) + neighbours(18.0) + neighbours(F32(33.3)) + [F32(0.0), F32(-0.0)]
    ulp = np.spacing(F32(16.5))
    k = 0
    while 16.5 + (10 ** k) * ulp < 17.0:
        pts.append(F32(-(16.5 + (10 ** k) * float(ulp))))
        k += 1
    pts += [F32(-16.5), F32(-16.6), F32(-16.7), F32(-17.0), F32(-87.0), F32(-104.0), F32(88.0), F32(1e4)]
    return np.array(pts, F32)


def channel_sums32(L):
    """sum_c L[b, c, p] in float32, channel after channel: the argument of the quirk function is this float32 value"""
    L = np.asarray(L, F32)
    s = np.zeros((L.shape[0], L.shape[2]), F32)
    for c in range(L.shape[1]):
        s = s + L[:, c]
    return s


def jsd_terms(sums, Si, Sp):
    """-> (terms [n] fp64, a1, a2): f(-(sl Si)) + f(sl Sp) per pixel; the two arguments are float32 products"""
    sl, si, sp = (np.asarray(t, F32).reshape(-1) for t in (sums, Si, Sp))
    a1, a2 = -(sl * si), sl * sp
    return f_quirk32(a1).astype(F64) + f_quirk32(a2).astype(F64), a1, a2


def jsd_fwd(sums, Si, Sp):
    """one jsd term -> (jsd, mean |terms|): jsd = -mean f(-Si sL) - mean f(Sp sL), the sum over pixels in fp64"""
    t, _, _ = jsd_terms(sums, Si, Sp)
    return -t.mean(), np.abs(t).mean()


def jsd_bwd(gscale, sums, Si, Sp):
    """-> dict gL, dSi, dSp [n] with magnitudes mgL, mdSi, mdSp; g = -gscale / n"""
    sl, si, sp = (np.asarray(t, F32).reshape(-1).astype(F64) for t in (sums, Si, Sp))
    _, a1, a2 = jsd_terms(sums, Si, Sp)
    d1, d2 = df_quirk32(a1).astype(F64), df_quirk32(a2).astype(F64)
    g = -float(F32(gscale)) / sl.size
    return dict(gL=g * (-si * d1 + sp * d2), mgL=abs(g) * (np.abs(si * d1) + np.abs(sp * d2)), dSi=g * (-sl * d1), mdSi=np.abs(g * sl * d1),
                dSp=g * (sl * d2), mdSp=np.abs(g * sl * d2))


def argmax2(S):
    """class 1 where S[:, 1] > S[:, 0], ties -> 0"""
    S = np.asarray(S)
    return (S[:, 1] > S[:, 0]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- Adam
ADAM_N = (1, 2, 3, 4, 5, 1023, 10007, 4 * 8192 * 256 + 4 * 1000 + 3)
ADAM_HYPER = ((1, 0.0, 1.0), (2, 1e-2, 1.0), (1000, 1e-2, 0.125), (100000, 0.0, 1.0))          # step, weight decay, gradient scale
ADAM_LR, ADAM_BETAS, ADAM_EPS = 1e-3, (0.9, 0.999), 1e-8
# every length (the longest lies beyond the 8192-block grid) with every set of hyper-parameters
ADAM_CASES = [(n, hy) for n in ADAM_N for hy in ADAM_HYPER]


def adam_case(n, seed=11):
    """p, g, m, v float32: g log-uniform in magnitude over 1e-6 .. 1e2 with random signs, m and v non-zero -- v of the order of g^2 (a
    settled state) but for the last eighth, where it is a thousandth of that (the state of the first steps: (1 - beta2) g^2 makes half
    of v') -- and a block (the second eighth, and element 0 from n = 3) of g = 0 with v = 0: the eps-only denominator"""
    r = rng(seed, n)
    g = (10.0 ** r.uniform(-6, 2, n)) * np.where(r.random(n) < 0.5, -1.0, 1.0)
    p = r.standard_normal(n)
    m = 0.1 * g * r.uniform(0.5, 1.5, n) + 1e-4 * r.standard_normal(n)
    v = g * g * r.uniform(0.5, 1.5, n) + 1e-12
    v[n - n // 8:] *= 1e-3
    z = slice(n // 8, n // 4)
    g[z], v[z] = 0.0, 0.0
    if n >= 3:
        g[0], v[0] = 0.0, 0.0
    return tuple(np.ascontiguousarray(t, F32) for t in (p, g, m, v))


def adam_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    """one torch.optim.Adam step (no amsgrad, L2 weight decay) from the given state -> dict p, m, v and the magnitudes mp = |p| + |dp|,
    mm = b1 |m| + (1 - b1) |g'|, mv = v', each the same formula on absolute values: |g'| = |gs g| + wd |p| (the two terms of the
    decayed gradient may cancel, and no fp32 evaluation is accurate to the cancelled sum)"""
    p, g, m, v = (np.asarray(t, F64) for t in (p, g, m, v))
    g, mg = g * grad_scale + wd * p, np.abs(g * grad_scale) + np.abs(wd * p)
    m2, mm = beta1 * m + (1.0 - beta1) * g, beta1 * np.abs(m) + (1.0 - beta1) * mg
    v2, mv = beta2 * v + (1.0 - beta2) * g * g, beta2 * v + (1.0 - beta2) * mg * mg
    c1, c2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = np.sqrt(v2) / np.sqrt(c2) + eps
    return dict(p=p - (lr / c1) * (m2 / denom), m=m2, v=v2, mp=np.abs(p) + (lr / c1) * (mm / denom), mm=mm, mv=mv)


def adam_step32(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    """the same step in float32 arithmetic, scalar coefficients rounded once from their fp64 values (as torch's fp32 Adam holds them):
    what correct fp32 arithmetic gives, for the bounds' sake"""
    p, g, m, v = (np.asarray(t, F32) for t in (p, g, m, v))
    f = F32
    g = g * f(grad_scale)
    if wd != 0:
        g = g + f(wd) * p
    m2 = f(beta1) * m + f(1.0 - beta1) * g
    v2 = f(beta2) * v + f(1.0 - beta2) * g * g
    c1, c2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = np.sqrt(v2) * f(1.0 / np.sqrt(c2)) + f(eps)
    return dict(p=p - f(lr / c1) * (m2 / denom), m=m2, v=v2)


# ---------------------------------------------------------------------------------------------------------------- shared case lists
BIL_HW = ((1, 1), (1, 37), (37, 1), (2, 3), (3, 5), (12, 12), (63, 65), (128, 128))
PLACE = ((8, 8, 16, 16, 0, 0), (12, 12, 25, 25, 0, 0), (5, 7, 11, 16, 0, 1), (1, 1, 3, 3, 1, 0))       # h, w, Ho, Wo, pt, pl


def bil_geoms(h, w):
    """(Ho, Wo, pt, pl): the exact 2h x 2w plane, and the padded (2h + 1) x (2w + 3) one with the window at every pt, pl in {0, 1}"""
    return [(2 * h, 2 * w, 0, 0)] + [(2 * h + 1, 2 * w + 3, pt, pl) for pt in (0, 1) for pl in (0, 1)]


def bil_case(h, w, Ho, Wo, B=2, C=3):
    """x [B, C, h, w] and an upstream gradient g [B, C, Ho, Wo]"""
    return normal(B, C, h, w, seed=21), normal(B, C, Ho, Wo, seed=22)


def place_case(h, w, Ho, Wo, B=3, C=5):
    """sub [B, 4C, h, w], bias [C], dy [B, C, Ho, Wo]"""
    return normal(B, 4 * C, h, w, seed=31), normal(C, seed=32), normal(B, C, Ho, Wo, seed=33)


HEAD_CASES = ((1, 1237, False), (3, 1237, False), (64, 1237, False), (3, 1237, True))          # C, HW, normalise-on-load
CAP_JSD = 2048 * 256                                                                          # pixels of one sweep of jsd_fwd_kernel's grid
# C, B, HW: the pixel counts 1, 255, 257 in one image and per image of two, and B HW = 2048 * 256 and 2048 * 256 + 1000 in two images
JSD_CASES = [(C, 1, hw) for C in (1, 64) for hw in (1, 255, 257)] + \
    [(C, 2, hw) for C in (1, 64) for hw in (1, 255, 257, CAP_JSD // 2, CAP_JSD // 2 + 500)]


def jsd_case(C, B, HW, seed=61):
    """L [B, C, HW] whose channel sums spread over all four branches of the quirk function, and S [B, 2, HW] of a sweep, every image
    its own"""
    r = rng(seed, C, B, HW)
    target = r.uniform(-60, 60, (B, HW))
    L = (r.standard_normal((B, C, HW)) * 0.5).astype(F32)
    L[:, 0] += (target - L.sum(1)).astype(F32)
    d = r.uniform(-30, 30, (B, HW))
    S = np.stack([1 / (1 + np.exp(-d)), 1 / (1 + np.exp(d))], 1).astype(F32)
    return L, S


def head_fwd_bounds(ref, C):
    """-> bounds of Vt, Vd ((C + 1) u sum |L H|) and S (S (8 u + the two V bounds) + floor)"""
    bVt, bVd = bound(C + 1, ref["mVt"]), bound(C + 1, ref["mVd"])
    return bVt, bVd, ref["S"] * (8 * U + (bVt + bVd)[:, None, :]) + FLOOR


def head_bwd_bound(ref, name):
    """8 u mag + floor |a - d| for the pixel gradients; through dL = g H + gs and dH = g L the floor carries the factor (>= 1) that
    multiplies the pixel gradient, and one more floor for the product's own result"""
    if name in ("gt", "gd"):
        return bound(8, ref["m" + name], FLOOR * ref["amd"])
    return bound(8, ref["m" + name], FLOOR * (1 + ref["amd"][:, None, :] * np.maximum(1.0, ref["f" + name])))


def within(got, ref, bnd, what, report=None):
    """assert |got - ref| <= bnd per element, every element finite; -> the worst error / bound (report: a function that is told it)"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what + ": not finite"
    err = np.abs(got - ref)
    bnd = np.broadcast_to(np.asarray(bnd, F64), err.shape)
    ratio = float((err / np.maximum(bnd, 1e-300)).max()) if err.size else 0.0
    if report is not None:
        report(f"RATIO {what}: err / bound {ratio:.3f}")
    bad = err > bnd
    assert not bad.any(), f"{what}: {int(bad.sum())} of {err.size} elements outside the bound, worst err / bound {ratio:.3f}"
    return ratio
