"""Plain fp64 references, per-element magnitudes, float32 emulations and shape tables of the fp32 matrix-core convolution kernels
(onet_amd/csrc/conv_mfma.hip, conv_wino4.hip, conv_wino4w.hip).  NumPy only, no project imports: tests/test_conv_refs_host.py holds every function here
against PyTorch's own CPU operators in float64 (and sizes the bounds), tests/test_gpu_fp32_conv_kernels.py holds the kernels against them.

Every comparison has the form |got - ref64| <= K * U * mag per element (stream_refs.bound / within).  `mag` is the same formula on absolute
values: the quantity a first-order rounding analysis of the ALGORITHM scales with --
  direct kernels            conv(|x|, |w|);  sum |dz| |x| for dW (+ |prior| when accumulating)
  F(4x4,3x3) (Lavin & Gray) |A^T| [ sum_ci (|G| |g| |G^T|) (.) (|B^T| |d| |B|) ] |A| per 4 x 4 output tile: an output element's error
                            depends on the whole 6 x 6 patch, so with one outlier in a tile conv(|x|, |w|) is the wrong scale.
  F(3x3,4x4) weight gradient |A'^T| [ sum_tiles (|G'| |dY| |G'^T|) (.) (|B^T| |d| |B|) ] |A'|
One K per algorithm and pass, NOT taken from the GPU: the smallest power of two at or above twice the worst err / (U mag) of the float32
emulation below over the GPU test's own shape list AND operands (same makers, same seeds -- the graded operands with their 2^8 outlier
set the worst case: every addition after the outlier rounds at its level; Gaussian data alone sits 10 to 30 times lower).  The factor
two: any summation order the kernels may use has the same first-order bound.  test_conv_refs_host.py recomputes the ratios and asserts
K / 4 < worst <= K / 2."""
import numpy as np

from stream_refs import U, bound, within, r32, rng, normal, F32, F64   # noqa: F401  (re-exported for the two test modules)

# K of |err| <= K U mag (derivation: module docstring; figures: profiles/r20_fp32_conv_fp64.md)
K_DIRECT = 64.0       # direct forward / input gradient (3x3 and 1x1)
K_DIRECT_DW = 16.0    # direct weight gradient, split-K + reduce (+ accumulate)
K_WINO4 = 8.0         # F(4x4,3x3) forward / input gradient, of the per-tile Winograd magnitude
K_WINO4_PACK = 8.0    # G g G^T of pack3x3_wino4_kernel, of |G| |g| |G^T|
K_WINO4W = 4.0        # F(3x3,4x4) weight gradient (+ accumulate), of its Winograd magnitude
K_STEM_DW = 4.0       # stem weight gradient (plain and BatchNorm-backward on load; + accumulate)

CI_T = 8              # conv_fwd_kernel: input channels per K chunk
FLUSH = 4             # ... chunks per fold of the two-level accumulation


# ---------------------------------------------------------------------------------------------------------------- inputs
def gaussian(B, C, H, W, seed):
    return normal(B, C, H, W, seed=seed)


def graded(B, C, H, W, seed):
    """Gaussian data times a magnitude ramp 2^-12 (column 0, channel 0) ... 2^0 (last column) over columns and channels, a checkerboard
    (2 x 2 squares) of exact zeros, and one 2^8 outlier per image: small and large outputs side by side."""
    x = normal(B, C, H, W, seed=seed).astype(F64)
    fw = np.arange(W) / (W - 1) if W > 1 else np.ones(1)
    fc = np.arange(C) / (C - 1) if C > 1 else np.zeros(1)
    e = -(12.0 - 2.0 * fc[:, None]) * (1.0 - fw[None, :])                       # [C, W]
    x = x * np.exp2(np.round(e))[None, :, None, :]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x[:, :, ((yy // 2 + xx // 2) % 2) == 1] = 0.0
    g = rng(seed, 77, B, C, H, W)
    for b in range(B):
        x[b, g.integers(C), g.integers(H), g.integers(W)] = 256.0
    return x.astype(F32)


def weights(Cout, Cin, ks, seed):
    return normal(Cout, Cin, ks, ks, seed=seed, scale=(2.0 / (Cin * ks * ks)) ** 0.5)


def twin_batch(x, bias):
    """[X ; clip(1 - X + bias, 0, 1)]: float32 operations in this order (stem.hip on load)"""
    x = np.asarray(x, F32)
    c = np.minimum(np.maximum((np.float32(1) - x) + np.float32(bias), np.float32(0)), np.float32(1))
    return np.concatenate([x, c], 0)


# ---------------------------------------------------------------------------------------------------------------- fp64 references
def _pad(x, p):
    return np.pad(np.asarray(x, F64), ((0, 0), (0, 0), (p, p), (p, p)))


def conv_fwd(x, w):
    """-> (z, mag) of the ks x ks convolution with padding ks // 2, x [B, Cin, H, W], w [Cout, Cin, ks, ks]"""
    w = np.asarray(w, F64)
    ks = w.shape[2]
    B, _, H, W = x.shape
    xp = _pad(x, ks // 2)
    z = np.zeros((B, w.shape[0], H, W), F64)
    mag = np.zeros_like(z)
    for ky in range(ks):
        for kx in range(ks):
            v = xp[:, :, ky:ky + H, kx:kx + W]
            z += np.tensordot(w[:, :, ky, kx], v, ([1], [1])).transpose(1, 0, 2, 3)
            mag += np.tensordot(np.abs(w[:, :, ky, kx]), np.abs(v), ([1], [1])).transpose(1, 0, 2, 3)
    return z, mag


def dgrad_weights(w):
    """the weights with which the input gradient is a forward convolution of dz: transposed and flipped"""
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def conv_dgrad(dz, w):
    return conv_fwd(dz, dgrad_weights(w))


def conv_wgrad(x, dz, ks, prior=None):
    """-> (dW [Cout, Cin, ks, ks] (+ prior), mag)"""
    B, _, H, W = x.shape
    xp = _pad(x, ks // 2)
    dz = np.asarray(dz, F64)
    dw = np.zeros((dz.shape[1], x.shape[1], ks, ks), F64)
    mag = np.zeros_like(dw)
    for ky in range(ks):
        for kx in range(ks):
            v = xp[:, :, ky:ky + H, kx:kx + W]
            dw[:, :, ky, kx] = np.tensordot(dz, v, ([0, 2, 3], [0, 2, 3]))
            mag[:, :, ky, kx] = np.tensordot(np.abs(dz), np.abs(v), ([0, 2, 3], [0, 2, 3]))
    if prior is not None:
        dw += np.asarray(prior, F64)
        mag += np.abs(np.asarray(prior, F64))
    return dw, mag


# ---------------------------------------------------------------------------------------------------------------- F(4x4, 3x3)
# Lavin & Gray 2016, interpolation points {0, +-1, +-2, inf}; as written out in the comments of conv_wino4.hip
WG = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], F64)
WBT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], F64)
WAT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], F64)


def _patches(x):
    """-> [B, C, ty, tx, 6, 6]: the 6 x 6 input patches (origin 4 t - 1) of the 4 x 4 output tiles, zero beyond the image"""
    B, C, H, W = x.shape
    ty, tx = -(-H // 4), -(-W // 4)
    xp = np.zeros((B, C, 4 * ty + 2, 4 * tx + 2), F64)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    p = np.empty((B, C, ty, tx, 6, 6), F64)
    for i in range(6):
        for j in range(6):
            p[..., i, j] = xp[:, :, i:i + 4 * ty:4, j:j + 4 * tx:4]
    return p


def _mm(a, x, bt, rnd):
    """a x bt^T over the last two axes; rnd: every product and every addition rounded to float32, summed left to right"""
    if rnd is None:
        return np.einsum("ik,...kl,jl->...ij", a, x, bt)

    def left(m, v):          # m [i, k] applied to axis -2 of v
        out = np.zeros(v.shape[:-2] + (m.shape[0], v.shape[-1]), F64)
        for k in range(m.shape[1]):
            out = rnd(out + rnd(m[:, k][:, None] * v[..., k:k + 1, :]))
        return out
    t = left(a, x)
    return np.swapaxes(left(bt, np.swapaxes(t, -1, -2)), -1, -2)


def wino4_pack(w, rnd=None, absval=False):
    """U = G g G^T -> [Cout, Cin, 6, 6]"""
    G = np.abs(WG) if absval else (WG if rnd is None else rnd(WG))
    g = np.abs(np.asarray(w, F64)) if absval else np.asarray(w, F64)
    return _mm(G, g, G, rnd)


def _wino4(x, w, rnd, absval, defect=None):
    B, Cin, H, W = x.shape
    f = np.abs if absval else (lambda m: m)
    Uw = wino4_pack(w, rnd, absval)                                            # [o, c, 6, 6]
    if defect is not None:
        Uw = defect(Uw)
    V = _mm(f(WBT), f(_patches(np.asarray(x, F64))), f(WBT), rnd)               # [b, c, ty, tx, 6, 6]
    if rnd is None:
        M = np.einsum("ijoc,ijcn->ijon", Uw.transpose(2, 3, 0, 1), V.transpose(4, 5, 1, 0, 2, 3).reshape(6, 6, Cin, -1), optimize=True)
        M = M.reshape((6, 6, Uw.shape[0], B) + V.shape[2:4]).transpose(3, 2, 4, 5, 0, 1)
    else:                                                                      # an MFMA accumulator: one fused multiply-add per channel
        M = np.zeros((B, Uw.shape[0]) + V.shape[2:], F64)
        for c in range(Cin):
            M = rnd(M + Uw[None, :, c, None, None] * V[:, None, c])
    Y = _mm(f(WAT), M, f(WAT), rnd)                                            # [b, o, ty, tx, 4, 4]
    ty, tx = Y.shape[2:4]
    return Y.transpose(0, 1, 2, 4, 3, 5).reshape(B, Uw.shape[0], 4 * ty, 4 * tx)[:, :, :H, :W]


def wino4_fwd(x, w):
    """-> (z, mag): the fp64 Winograd restatement (equal to conv_fwd up to fp64 rounding) and the per-tile Winograd magnitude"""
    return _wino4(x, w, None, False), _wino4(x, w, None, True)


def wino4_emul(x, w, defect=None):
    """float32 emulation: transforms in float32 (coefficients rounded, every operation rounded), sequential accumulation over ci"""
    return _wino4(r32(x).astype(F64), r32(w).astype(F64), lambda v: r32(v).astype(F64), False, defect)


# ---------------------------------------------------------------------------------------------------------------- emulations, direct
def _f(v):
    return r32(v).astype(F64)


def direct_emul(x, w, fold=True, trunc=None, halo=None):
    """conv_fwd_kernel in float32: a sequential fused-multiply-add chain over (chunk of 8 channels; tap; channel), folded into a second
    accumulator every FLUSH chunks (fold=False: the plain sequential chain, the envelope -- and planted defect (a)).
    trunc: operands cut to that many mantissa bits (defect (c));  halo = (b, y, x, ky, kx): at output pixel (y, x) of image b the tap
    (ky, kx), which lies outside the image, reads the nearest row inside instead of zero (defect (d))."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    if trunc is not None:
        def cut(v):
            m, e = np.frexp(v)
            return np.ldexp(np.trunc(m * 2.0 ** (trunc + 1)) / 2.0 ** (trunc + 1), e)
        x, w = cut(x), cut(w)
    ks = w.shape[2]
    B, Cin, H, W = x.shape
    xp = _pad(x, ks // 2)
    acc = np.zeros((B, w.shape[0], H, W), F64)
    tot = np.zeros_like(acc)
    nch = -(-Cin // CI_T)
    for ch in range(nch):
        for ky in range(ks):
            for kx in range(ks):
                for c in range(ch * CI_T, min(Cin, (ch + 1) * CI_T)):
                    v = xp[:, c, None, ky:ky + H, kx:kx + W]
                    if halo is not None and (ky, kx) == tuple(halo[3:]):
                        v = v.copy()
                        b, y, xx = halo[:3]
                        yy = min(max(y + ky - ks // 2, 0), H - 1)
                        v[b, 0, y, xx] = x[b, c, yy, xx + kx - ks // 2]
                    acc = _f(acc + w[None, :, c, ky, kx, None, None] * v)
        if fold and ch % FLUSH == FLUSH - 1:
            tot = _f(tot + acc)
            acc = np.zeros_like(acc)
    return _f(acc + tot) if fold else acc


def wgrad_plan(B, Cin, Cout, H, W, ks):
    """wgrad_plan of conv_mfma.hip -> (pw, splitK, stripsX, stripsY)"""
    pw = 32 if W > 16 else 16
    pr = 64 // pw
    sx, sy = -(-W // pw), -(-H // pr)
    nunits = B * sx * sy
    tiles = -(-Cout // 64) * -(-Cin // 64)
    s = -(-1024 // tiles)
    s = min(s, (192 << 20) // (ks * ks * Cout * Cin * 4), nunits)
    return pw, max(s, 1), sx, sy


def wgrad_ws_bytes(B, Cin, Cout, H, W, ks):
    if ks == 3 and Cin <= 4:
        return stem_blocks(B, H) * 9 * Cout * Cin * 4
    return wgrad_plan(B, Cin, Cout, H, W, ks)[1] * ks * ks * Cout * Cin * 4


def stem_blocks(B, H):
    return B * -(-H // 32)


def wino4_nparts(B, H, W):
    """onet_conv3x3_winograd4_nparts: one record per 16 x 16-pixel tile half of a full 16 x 32-pixel block; 0: no statistics there"""
    return 2 * B * (W // 32) * (H // 16) if B > 0 and W % 32 == 0 and H % 16 == 0 else 0


def stem_nparts(B, Cin, Cout, H, W):
    """onet_conv3x3_stem_nparts: one record per full 16 x 64-pixel tile; 0: not the fused stem's shape"""
    return B * (H // 16) * (W // 64) if 1 <= Cin <= 4 and Cout <= 128 and H % 16 == 0 and W % 64 == 0 else 0


def fwd_in_range(Cin, Cout, planes, plane, ks):
    """launch_fwd of conv_mfma.hip: `planes` input planes of `plane` floats (Cin of H W; MODE 2 gathers from Cin / 4 planes of Ho Wo) with
    two K chunks of look-ahead, and the packed weights, inside the 2 GiB buffer-resource range"""
    return (planes + 2 * CI_T) * plane * 4 < 2 ** 31 and (Cin + 2 * CI_T) * ks * ks * Cout * 4 < 2 ** 31


def dw_in_range(Cin, HW, dz_planes, dz_plane):
    """wgrad_in_range of conv_mfma.hip: x and dz with a 64-channel tile of look-ahead"""
    return (Cin + 64) * HW * 4 < 2 ** 31 and (dz_planes + 64) * dz_plane * 4 < 2 ** 31


def fwd_blocks(B, Cout, H, W):
    """ConvCfg<KS,2,2,1,4,TW>: 64 channels x (8 rows x 32 px | 16 rows x 16 px) -> (blocks, tilesX, tilesY, coTiles)"""
    tw = 32 if W > 16 else 16
    rows = 4 * (32 // tw) * 2
    tx, ty, co = -(-W // tw), -(-H // rows), -(-Cout // 64)
    return B * tx * ty * co, tx, ty, co


def direct_dw_emul(x, dz, ks, prior=None):
    """conv_wgrad_kernel + wgrad_reduce_kernel in float32: split s takes the 64-pixel strips s, s + splitK, ... (image-major, then strip
    rows, then strip columns), one sequential fused-multiply-add chain over their pixels; the reduce sums the splits in four
    interleaved groups, (g0 + g1) + (g2 + g3), then adds the prior dW.  Pass a few channels: every (co, ci) is independent."""
    x, dz = np.asarray(x, F64), np.asarray(dz, F64)
    B, Cin, H, W = x.shape
    Cout = dz.shape[1]
    pw, splitK, sx, sy = wgrad_plan(B, Cin, Cout, H, W, ks)
    return _dw_emul(x, dz, ks, pw, sx, sy, prior, splitK)


def _dw_emul(x, dz, ks, pw, sx, sy, prior, splitK):
    B, Cin, H, W = x.shape
    Cout = dz.shape[1]
    pr = 64 // pw
    xp = _pad(x, ks // 2)
    nunits = B * sx * sy
    slabs = np.zeros((splitK, Cout, Cin, ks, ks), F64)
    for s in range(splitK):
        acc = slabs[s]
        for u in range(s, nunits, splitK):
            b, y0, x0 = u // (sx * sy), ((u // sx) % sy) * pr, (u % sx) * pw
            for r in range(pr):
                for c in range(pw):
                    y, xx = y0 + r, x0 + c
                    if y < H and xx < W:
                        acc = _f(acc + dz[b, :, y, xx][:, None, None, None] * xp[b, :, y:y + ks, xx:xx + ks][None])
        slabs[s] = acc
    g = []
    for k0 in range(4):
        t = np.zeros_like(slabs[0])
        for k in range(k0, splitK, 4):
            t = _f(t + slabs[k])
        g.append(t)
    s = _f(_f(g[0] + g[1]) + _f(g[2] + g[3]))
    return s if prior is None else _f(np.asarray(prior, F64) + s)


def direct_dw_emul_full(x, dz, ks, full_shape, prior=None):
    """direct_dw_emul of a channel subset of a layer whose plan (splitK) is that of the FULL shape (B, Cin, Cout, H, W)"""
    pw, splitK, sx, sy = wgrad_plan(*full_shape, ks)
    return _dw_emul(np.asarray(x, F64), np.asarray(dz, F64), ks, pw, sx, sy, prior, splitK)


# ---------------------------------------------------------------------------------------------------------------- packs (index maps)
def pack3x3_fwd(w):
    """[ci][tap][co]"""
    Cout, Cin = w.shape[:2]
    return np.ascontiguousarray(np.asarray(w).reshape(Cout, Cin, 9).transpose(1, 2, 0)).reshape(-1)


def pack3x3_dgrad(w):
    """[co][8 - tap][ci]"""
    Cout, Cin = w.shape[:2]
    return np.ascontiguousarray(np.asarray(w).reshape(Cout, Cin, 9)[:, :, ::-1].transpose(0, 2, 1)).reshape(-1)


def packT2x2(w):
    """w [Cin, Cout, 2, 2] -> (wf [ci][q][co], wd [q][co][ci], wq [ci][co][q]), q = 2 dy + dx"""
    Cin, Cout = w.shape[:2]
    v = np.asarray(w).reshape(Cin, Cout, 4)
    return (np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(-1), np.ascontiguousarray(v.transpose(2, 1, 0)).reshape(-1),
            np.ascontiguousarray(v).reshape(-1))


def wino4_pack_layout(Uw, fwd):
    """U [Cout, Cin, 6, 6] -> the packed [row][36][CnP] of pack3x3_wino4_kernel: rows ci (fwd) / co (dgrad: the taps flipped before the
    transform, i.e. U of the flipped kernel), the other channel padded to 64s with zeros and permuted inside each block of 64 --
    channel 16 g + i of a block sits at float 4 i + g."""
    Uw = np.asarray(Uw)
    t = Uw.transpose(1, 0, 2, 3) if fwd else Uw                # [row, cn, 6, 6]
    R, Cn = t.shape[:2]
    CnP = (Cn + 63) & ~63
    out = np.zeros((R, 36, CnP), Uw.dtype)
    q = np.arange(CnP)
    cn = (q & ~63) + ((q & 63) >> 2) + 16 * (q & 3)
    ok = cn < Cn
    out[:, :, q[ok]] = t.reshape(R, Cn, 36).transpose(0, 2, 1)[:, :, cn[ok]]
    return out


# ---------------------------------------------------------------------------------------------------------------- shape tables
# (property, (B, Cin, Cout, H, W)): the reason the row is there, asserted by check_fwd_property from the restated tile arithmetic
FWD_SHAPES = [("tile32", (1, 8, 64, 8, 32)), ("tile16", (2, 8, 64, 16, 16))] + \
    [("cin", (1, c, 8, 5, 17)) for c in (1, 3, 7, 9, 32, 33, 40)] + \
    [("cout", (1, 9, c, 5, 17)) for c in (1, 3, 4, 36, 68)] + \
    [("map", (1, 9, 8, h, w)) for h, w in ((1, 1), (2, 2), (4, 4), (7, 15), (9, 16), (17, 17), (2, 33))] + \
    [("deep", (2, 1024, 64, 4, 4)), ("xcd", (3, 8, 8, 17, 33)), ("fold", (2, 1024, 64, 4, 4)), ("fold", (2, 4096, 64, 4, 4))]


def fwd_inputs(prop):
    """the operand sets a row of FWD_SHAPES runs with.  "fold": operands of ONE SIGN (post-ReLU data times a mean filter) -- the
    accumulator then grows to the magnitude itself and every addition rounds at its level, so a single sequential chain of 9 Cin
    terms leaves the bound that the two-level accumulation keeps (test_bound_sees_the_lost_two_level_fold); on signed Gaussian data
    the partial sums stay a small fraction of the magnitude and either form sits far inside."""
    return ("onesign",) if prop == "fold" else ("gauss", "graded")


def fwd_operands(shape, ks, name):
    """-> (x, dz, w) of a direct forward / input gradient case: what the GPU test runs and what the emulation sizes K on"""
    B, Cin, Cout, H, W = shape
    if name == "onesign":
        return np.abs(gaussian(B, Cin, H, W, 101)), np.abs(gaussian(B, Cout, H, W, 102)), np.abs(weights(Cout, Cin, ks, 103))
    maker = dict(gauss=gaussian, graded=graded)[name]
    return maker(B, Cin, H, W, 101), maker(B, Cout, H, W, 102), weights(Cout, Cin, ks, 103)


def check_fwd_property(prop, shape):
    B, Cin, Cout, H, W = shape
    blocks, tx, ty, co = fwd_blocks(B, Cout, H, W)
    chunks = -(-Cin // CI_T)
    if prop == "tile32":
        assert blocks == 1 and W == 32 and H == 8 and Cout == 64 and Cin == CI_T
    elif prop == "tile16":
        assert blocks == B and W == 16 and H == 16 and Cout == 64
    elif prop == "cin":       # chunk tails; 32 ends on the fold, 33 and 40 start a fifth chunk after it
        assert Cin % CI_T != 0 or Cin in (FLUSH * CI_T, (FLUSH + 1) * CI_T)
        assert (chunks > FLUSH) == (Cin > FLUSH * CI_T)
    elif prop == "cout":      # scalar weight staging (Cout % 4 != 0); a channel-tile tail
        assert Cout % 4 != 0 or Cout < 64 or (co == 2 and Cout % 64 != 0)
    elif prop == "map":
        assert (H, W) in ((1, 1), (2, 2), (4, 4)) or W in (15, 16, 17) or (W == 33 and tx == 2)
    elif prop in ("deep", "fold"):      # at least 32 folds: 9 Cin >= 9216 terms against chains of 288
        assert chunks >= 32 * FLUSH and H == W == 4
    elif prop == "xcd":       # the remainder branch of xcd_block_id; odd batch; a second column tile of one pixel; a row-tile tail
        assert blocks >= 9 and blocks % 8 != 0 and B == 3 and W == 33 and H % 8 != 0
    else:
        raise AssertionError(prop)


# (property, (B, Cin, Cout, H, W), ks, out_layout)
DW_SHAPES = [("unit1", (1, 5, 3, 2, 20), 3, 0), ("unit1", (1, 5, 3, 4, 9), 1, 0),
             ("all", (2, 64, 64, 7, 17), 3, 0), ("all", (3, 72, 100, 9, 16), 3, 0), ("all", (3, 72, 100, 9, 16), 1, 1),
             ("all", (2, 64, 64, 7, 17), 1, 0),
             ("ragged", (5, 256, 256, 20, 48), 3, 0), ("ragged", (5, 256, 256, 20, 48), 1, 1)]


def check_dw_property(prop, shape, ks, out_layout):
    B, Cin, Cout, H, W = shape
    pw, splitK, sx, sy = wgrad_plan(B, Cin, Cout, H, W, ks)
    units = B * sx * sy
    assert not (ks == 3 and Cin <= 4), "the stem kernel's shapes have their own table"
    assert out_layout == 0 or (ks == 1 and Cout % 4 == 0)
    if prop == "unit1":
        assert units == 1 and splitK == 1 and (H % (64 // pw) or W % pw)
    elif prop == "all":       # every strip its own split; channel tiles with tails or exactly full
        assert splitK == units > 1
    elif prop == "ragged":    # units not divisible by splitK, a split's strips lie in different images, odd batch
        assert 1 < splitK < units and units % splitK != 0 and B % 2 == 1 and splitK % (sx * sy) != 0
    else:
        raise AssertionError(prop)


# (property, (B, Cin, Cout, H, W)) of conv_wino4_kernel<8,0> (W > 16) and <4,0> (W <= 16: two images per block)
WINO_SHAPES = [("k", (1, c, 8, 16, 32)) for c in (4, 8, 12, 16, 20)] + [("kpair", (2, c, 8, 16, 16)) for c in (4, 8, 12, 16, 20)] + \
    [("cout", (1, 8, c, 16, 32)) for c in (4, 60, 64, 68, 132)] + \
    [("wide", (1, 8, 8, h, w)) for h, w in ((3, 17), (4, 20), (15, 30), (16, 32), (18, 36))] + \
    [("pair", (b, 8, 8, 6, w)) for b, w in ((1, 5), (2, 8), (3, 13), (2, 16))] + [("deep", (1, 512, 64, 16, 32))]


WINO_PACK_SHAPES = [(4, 4), (68, 20), (132, 8), (64, 64)]      # (Cout, Cin) of the pack test: padded channels, several 64-blocks


def wino_blocks(B, Cout, H, W):
    """W4Cfg<TXB>: 4 tile rows x TXB tile columns x IMG images, 64 channels -> (blocks, images per block)"""
    txb = 8 if W > 16 else 4
    img = 32 // (txb * 4)
    return -(-B // img) * -(-W // (4 * txb)) * -(-H // 16) * -(-Cout // 64), img


def check_wino_property(prop, shape):
    B, Cin, Cout, H, W = shape
    blocks, img = wino_blocks(B, Cout, H, W)
    assert Cin % 4 == 0 and Cout % 4 == 0
    if prop in ("k", "kpair"):     # one to five K steps of 4 channels: around the weight ring (2 ahead) and the halo prefetch (3 ahead)
        assert 1 <= Cin // 4 <= 5 and blocks == 1 and img == (2 if prop == "kpair" else 1)
    elif prop == "cout":
        assert Cout < 64 or Cout % 64 == 0 or -(-Cout // 64) >= 2
    elif prop == "wide":
        assert img == 1 and (W % 4 != 0 or W % 32 != 0 or H % 16 != 0 or (H, W) == (16, 32))
    elif prop == "pair":           # odd B: a half-empty pair
        assert img == 2 and W in (5, 8, 13, 16)
    elif prop == "deep":
        assert Cin == 512
    else:
        raise AssertionError(prop)


# ---------------------------------------------------------------------------------------------------------------- F(3x3, 4x4) weight gradient
# dW = A'^T [ sum_tiles (G' dY G'^T) (.) (B^T d B) ] A'  (conv_wino4w.hip): 4 x 4 tiles of dY in the role of the filter, the same
# points.  G' rows p^j / N_p for p = 0, 1, -1, 2, -2 with N = 4, -6, -6, 24, 24, row inf = (0, 0, 0, 1); the kernel applies the
# integer rows per tile and the 1 / N_p scales once per position in the fold kernel.
WGP_INT = np.array([[1, 0, 0, 0], [1, 1, 1, 1], [1, -1, 1, -1], [1, 2, 4, 8], [1, -2, 4, -8], [0, 0, 0, 1]], F64)
WGP_SCALE = np.array([1 / 4, -1 / 6, -1 / 6, 1 / 24, 1 / 24, 1], F64)
WAPT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 1]], F64)


def wino4w_ok(B, Cin, Cout, H, W):
    return B > 0 and Cin >= 32 and Cin % 32 == 0 and Cout > 0 and Cout % 4 == 0 and (W % 32 == 0 or (W == 16 and B % 2 == 0)) and H % 4 == 0


def wino4w_plan(B, Cin, Cout, H, W, target=256):
    """wino4w_plan of conv_wino4w.hip -> (splitK, units, units per split); a unit is a row of 8 tiles (W == 16: of an image pair)"""
    ty, tx = -(-H // 4), -(-W // 32)
    units = (B // 2) * ty if W == 16 else B * ty * tx
    tiles = -(-Cin // 32) * -(-Cout // 64)
    k = max(1, -(-target // tiles))
    k = min(k, max(1, (320 << 20) // (36 * Cout * Cin * 4)), max(1, units // 8))
    return k, units, -(-units // k)


def wino4w_ws_bytes(B, Cin, Cout, H, W):
    return wino4w_plan(B, Cin, Cout, H, W)[0] * 36 * Cout * Cin * 4


def _tile_seq(t, W):
    """[B, C, ty, tx, i, j] -> [tiles in the kernel's order, C, i, j]: image, tile row, tile column; 16-pixel maps: image PAIR, tile row,
    image of the pair, tile column"""
    B, C, ty, tx = t.shape[:4]
    if W == 16:
        t = t.reshape(B // 2, 2, C, ty, tx, *t.shape[4:]).transpose(0, 3, 1, 4, 2, 5, 6)
    else:
        t = t.transpose(0, 2, 3, 1, 4, 5)
    return t.reshape(-1, C, *t.shape[-2:])


def _wino4w(x, dz, rnd, absval, full_shape=None, prior=None):
    B, Cin, H, W = x.shape
    f = np.abs if absval else (lambda m: m)
    dzt = np.asarray(dz, F64).reshape(B, dz.shape[1], H // 4, 4, W // 4, 4).transpose(0, 1, 2, 4, 3, 5)
    V = _tile_seq(_mm(f(WBT), f(_patches(np.asarray(x, F64))), f(WBT), rnd), W)       # [n, ci, 6, 6]
    if rnd is None:
        G = f(WGP_INT * WGP_SCALE[:, None])
        P = _tile_seq(_mm(G, f(dzt), G, None), W)                                     # [n, co, 6, 6]
        M = np.einsum("noij,ncij->ocij", P, V)
        dw = _mm(f(WAPT), M, f(WAPT), None)
        if prior is not None:
            dw = dw + f(np.asarray(prior, F64))
        return dw
    P = _tile_seq(_mm(WGP_INT, dzt, WGP_INT, rnd), W)
    k, units, per = wino4w_plan(*(full_shape or (B, Cin, dz.shape[1], H, W)))
    assert units * 8 == P.shape[0]
    tot = np.zeros((P.shape[1], Cin, 6, 6), F64)
    for s in range(k):                                  # a split: consecutive units, one fused-multiply-add chain; then the splits in order
        acc = np.zeros_like(tot)
        for n in range(8 * s * per, min(8 * (s + 1) * per, P.shape[0])):
            acc = rnd(acc + P[n][:, None] * V[n][None])
        tot = rnd(tot + acc)
    sc = rnd(rnd(WGP_SCALE)[:, None] * rnd(WGP_SCALE)[None, :])
    dw = _mm(WAPT, rnd(tot * sc), WAPT, rnd)
    return dw if prior is None else rnd(np.asarray(prior, F64) + dw)


def wino4w_wgrad(x, dz, prior=None):
    """-> (dW, mag): the fp64 restatement (equal to conv_wgrad up to fp64 rounding) and its Winograd magnitude (+ prior)"""
    return _wino4w(x, dz, None, False, prior=prior), _wino4w(x, dz, None, True, prior=prior)


def wino4w_emul(x, dz, full_shape, prior=None):
    """float32 emulation on a channel subset of a layer of `full_shape` (its split-K plan)"""
    return _wino4w(_f(x), _f(dz), _f, False, full_shape, prior)


# (property, (B, Cin, Cout, H, W))
W4W_SHAPES = [("unit1", (1, 32, 4, 4, 32)), ("split", (2, 32, 4, 32, 32)), ("ragged", (17, 32, 68, 8, 32)), ("split", (2, 96, 68, 16, 64)),
              ("pair1", (2, 32, 64, 4, 16)), ("pair", (6, 64, 96, 16, 16)), ("pairsplit", (8, 32, 4, 16, 16))]


def check_w4w_property(prop, shape):
    B, Cin, Cout, H, W = shape
    assert wino4w_ok(*shape)
    k, units, per = wino4w_plan(*shape)
    if prop == "unit1":
        assert units == 1 and k == 1
    elif prop == "split":
        assert k > 1 and units % k == 0
    elif prop == "ragged":    # the last split is shorter; B odd, a split ends inside an image; a Cout tile tail
        assert k > 1 and units % k != 0 and (k - 1) * per < units and B % 2 == 1 and per % (units // B) != 0 and Cout % 64 != 0
    elif prop in ("pair1", "pair", "pairsplit"):
        assert W == 16 and B % 2 == 0 and (units == 1) == (prop == "pair1") and (k > 1) == (prop == "pairsplit")
    else:
        raise AssertionError(prop)


# ---------------------------------------------------------------------------------------------------------------- stem weight gradient
def bn_case(z, da, groups, seed, train=True):
    """What the stem kernel reads beside x when it forms dz on load: save [G][4][C] = (mean, invstd, scale, shift) of each statistics
    group's z (float32), coef [G][4][C] = the (hi, lo) float pairs of c1 = mean(dy), c2 = mean(dy xhat) of the BatchNorm backward
    (train; eval: no coef, c1 = c2 = 0), dy = da where fma(z - mean, scale, shift) > 0 in float32 -- and dz in fp64 from exactly those
    float32 values:  dz = scale (dy - c1 - xhat c2), xhat = (z - mean) invstd."""
    z, da = np.asarray(z, F32), np.asarray(da, F32)
    B, C = z.shape[:2]
    Bg = B // groups
    gamma, beta = (1 + 0.1 * normal(C, seed=seed)).astype(F64), 0.1 * normal(C, seed=seed + 1).astype(F64)
    save, coef, dz = np.zeros((groups, 4, C), F32), np.zeros((groups, 4, C), F32), np.zeros(z.shape, F64)
    for g in range(groups):
        s = slice(g * Bg, (g + 1) * Bg)
        z64 = z[s].astype(F64)
        mean = z64.mean((0, 2, 3))
        inv = 1 / np.sqrt(z64.var((0, 2, 3)) + 1e-5)
        save[g] = np.stack([mean, inv, gamma * inv, beta]).astype(F32)
        m32, i32, sc32, sh32 = (save[g, i].astype(F64)[None, :, None, None] for i in range(4))
        zc32 = (z[s] - save[g, 0][None, :, None, None]).astype(F64)                  # the float32 subtraction of the mask expression
        dy = np.where(zc32 * sc32 + sh32 > 0, da[s].astype(F64), 0.0)
        xhat = (z64 - m32) * i32
        c1, c2 = (dy.mean((0, 2, 3)), (dy * xhat).mean((0, 2, 3))) if train else (np.zeros(C), np.zeros(C))
        for i, c in ((0, c1), (2, c2)):
            coef[g, i] = c.astype(F32)
            coef[g, i + 1] = (c - coef[g, i].astype(F64)).astype(F32)
        c1 = coef[g, 0].astype(F64) + coef[g, 1].astype(F64)
        c2 = coef[g, 2].astype(F64) + coef[g, 3].astype(F64)
        dz[s] = sc32 * (dy - c1[None, :, None, None] - xhat * c2[None, :, None, None])
    return save, (coef if train else None), dz


def stem_dw_emul(x, dz, prior=None):
    """conv3x3_stem_wgrad_kernel + wgrad_reduce_kernel in float32: a block takes a band of 32 rows of one image, a wave 8 of them, a
    lane four neighbouring columns (and the same four 256 columns further on), walking down its rows with one fused multiply-add
    per term; then the butterfly over the 64 lanes, (w0 + w1) + (w2 + w3), and the reduce over the blocks; dz rounded to float32 first
    (the BatchNorm-on-load form rounds its fp64 dz once)."""
    x, dz = np.asarray(x, F64), _f(dz)
    B, Cin, H, W = x.shape
    Cout = dz.shape[1]
    xp = _pad(x, 1)
    lanes = np.arange(64)
    slabs = []
    for b in range(B):
        for yb in range(0, H, 32):
            waves = []
            for wid in range(4):
                acc = np.zeros((64, Cout, Cin, 3, 3), F64)
                y0 = yb + 8 * wid
                for xb in range(0, W, 256):
                    for y in range(y0, min(y0 + 8, H)):
                        for p in range(4):
                            col = xb + 4 * lanes + p
                            ok = col < W
                            cc = np.where(ok, col, 0)
                            g = np.where(ok[None], dz[b][:, y][:, cc], 0.0)                           # [Cout, 64]
                            win = np.stack([np.stack([xp[b][:, y + i][:, cc + j] for j in range(3)], -1) for i in range(3)], -2)   # [Cin, 64, 3, 3]
                            acc = _f(acc + g.T[:, :, None, None, None] * win.transpose(1, 0, 2, 3)[:, None])
                for o in (32, 16, 8, 4, 2, 1):
                    acc = _f(acc + acc[lanes ^ o])
                waves.append(acc[0])
            slabs.append(_f(_f(waves[0] + waves[1]) + _f(waves[2] + waves[3])))
    g = []
    for k0 in range(4):
        t = np.zeros_like(slabs[0])
        for k in range(k0, len(slabs), 4):
            t = _f(t + slabs[k])
        g.append(t)
    s = _f(_f(g[0] + g[1]) + _f(g[2] + g[3]))
    return s if prior is None else _f(np.asarray(prior, F64) + s)


# (B, Cin, Cout, H, W): the four <CIN, COG> instances <1,4> <2,2> <3,2> <4,1>; Cout tails of COG; W % 4 != 0 (scalar loads); the second
# trip of the 256-column loop; one row, a full band, a band and one row
STEM_SHAPES = [(2, 1, 10, 33, 260), (2, 2, 5, 1, 3), (2, 3, 6, 32, 64), (4, 4, 3, 33, 64)]


def check_stem_shapes():
    assert [s[1] for s in STEM_SHAPES] == [1, 2, 3, 4]
    cog = {1: 4, 2: 2, 3: 2, 4: 1}
    assert any(s[2] % cog[s[1]] for s in STEM_SHAPES if s[1] == 1) and any(s[2] % cog[s[1]] for s in STEM_SHAPES if s[1] == 2)
    assert {s[4] for s in STEM_SHAPES} == {3, 64, 260} and {s[3] for s in STEM_SHAPES} == {1, 32, 33}
    assert any(s[4] > 256 and s[4] % 4 == 0 for s in STEM_SHAPES) and any(s[4] % 4 for s in STEM_SHAPES)
    assert all(s[0] % 2 == 0 for s in STEM_SHAPES) and any(stem_blocks(s[0], s[3]) > 4 for s in STEM_SHAPES)
