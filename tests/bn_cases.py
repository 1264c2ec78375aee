"""Hostile BatchNorm + ReLU inputs, their fp64 reference and per-channel error bounds (shared by tests/test_bn_bounds_host.py and
tests/test_gpu_bn_fp64.py; pure numpy, no GPU).

Inputs (`make`): channel c has kind c % 9 (KINDS): |mean| >> std of either sign, constant channels, a channel whose whole variance
lies BETWEEN the per-image partials, var << eps, a large spread, an outlier where the statistics kernel takes its pivot, a single
non-zero element, and one ordinary channel.  gamma is negative where c % 4 == 1 and exactly 0 in one channel when C > 8.
|mean| / std stops at 1e4 in kind 0: at 1e6 the fp32 rounding of the mean alone moves about a third of the ReLU decisions and a
comparison says nothing any more.

Reference (`train_ref`, `eval_ref`): everything in fp64 from the fp32 inputs.

Bounds, per channel and from reference quantities only (u = 2^-24, one fp32 rounding; every bound + 1e-37 so exact zeros compare):

  E_mean = 2u max|z_c|       a partial mean is stored as fp32 (one rounding), the channel mean is stored as fp32 (another)
  E_inv  = 8u + 2 E_mean D / (var + eps)   on invstd, relative; D = max over the kernel's partials (image x statistics chunk) of
           |partial mean - mean64|.  The second term is real and not slack: a record carries its partial mean r_k ROUNDED to fp32
           (e_k = r_k - mean_k) and M2 about that rounded mean, and Chan's merge of such records computes
               sum_i (z_i - m)^2 + 2 sum_k n_k e_k (r_k - m)
           -- the cross term is dropped.  It is bounded by 2 n max|e_k| max|r_k - m| <= n E_mean D, is a property of the record
           format (three floats per record), and vanishes for realistic n_k, where r_k - m is small.  Not to be "fixed".
  R      = 4u + E_inv        relative error of scale = fl(gamma invstd) with the roundings of t = fl(z - mean) and of the fma
  tol_a      = |s| (E_mean + R |z - mean64|) + 2u |a64|
  tol_dbeta  = 2u |dbeta64| + 2^-40 sum|dy|          the (hi, lo) records keep ~48 bits of each partial sum
  tol_dgamma = (E_mean invstd64 + R max|xhat|) sum|dy| + 2u |dgamma64|
  tol_dz     = |s| [ R (|dy| + |c1| + |xhat c2|) + |c2| (E_mean invstd64 + R |xhat|) + |xhat| tol_dgamma / N ] + u |dz64|
  running_mean: |rm' - ((1 - m) rm + m mean64)| <= 3u (|rm| + |mean64|) + m E_mean
  running_var : the same with the unbiased variance, whose error is E_inv's two terms before the division by var + eps:
                m (4u unb64 + 2 E_mean D n / (n - 1))

ReLU decisions: the kernels take the mask from an fp32 pre-activation, so pixels with |pre64| <= 4 tol_a are undetermined; the
reference returns `da` with zeros there (feed THAT da to the kernels) and neither the sums nor dz depend on the decision.  The share
of such pixels must stay <= 3 % in every channel of every case (asserted by the host test; a condition on the inputs)."""
import math

import numpy as np

U = 2.0 ** -24
TINY = 1e-37
EPS = float(np.float32(1e-5))           # the kernels take eps and momentum as fp32
MOMENTUM = float(np.float32(0.1))
STAT_CHUNK = 16384                      # ops._bn_nparts: one statistics partial per image and 16384-element chunk

KINDS = ["mean=1e4 std=1", "mean=-3e3 std=1", "constant 7.25", "constant per image", "var << eps", "std=1e3", "pivot is an outlier",
         "one non-zero element", "ordinary"]

# (B, C, H, W): the smallest shapes that reach each code path
SHAPES = [
    (2, 9, 1, 1),        # N = 2
    (1, 9, 1, 2),        # N = 2 in one image
    (3, 10, 7, 9),       # scalar loops (HW % 4 != 0)
    (4, 18, 16, 16),     # every kind twice; two statistics groups of 2 images
    (2, 9, 64, 64),      # HW = 4096: the full-chunk apply path
    (2, 9, 50, 82),      # HW = 4100: a full chunk and a 4-element tail
    (2, 9, 132, 128),    # two statistics chunks; the unrolled loop
    (1, 9, 131, 129),    # two chunks on the scalar path; chunk_len rounded up to 8452
]
SLICE_SHAPE = (2, 9, 64, 64)            # also taken as channels SLICE_CH of a SLICE_BUF-channel buffer (z_bs = 16 HW)
SLICE_CH, SLICE_BUF = slice(3, 12), 16


def kind_of(c):
    return KINDS[c % 9]


def make(B, C, H, W, seed=0):
    """-> fp32 z [B,C,H,W], gamma [C], beta [C], da [B,C,H,W]"""
    g = np.random.Generator(np.random.PCG64([seed, B, C, H, W]))
    z = np.empty((B, C, H, W), dtype=np.float64)
    for c in range(C):
        r = g.standard_normal((B, H, W))
        k = c % 9
        if k == 0:
            v = 1e4 + r
        elif k == 1:
            v = -3e3 + r
        elif k == 2:
            v = np.full_like(r, 7.25)
        elif k == 3:
            v = np.broadcast_to((3.5 * np.arange(B) - 2.0)[:, None, None], r.shape).copy()
        elif k == 4:
            v = 1e-4 * r
        elif k == 5:
            v = 1e3 * r
        elif k == 6:
            v = 5.0 + 1e-2 * r
            v[:, 0, 0] += 1e2
        elif k == 7:
            v = np.zeros_like(r)
            v.reshape(-1)[int(g.integers(v.size))] = 3.0
        else:
            v = 0.7 + 2.0 * r
        z[:, c] = v
    gamma = 1.0 + 0.3 * g.standard_normal(C)
    gamma[np.arange(C) % 4 == 1] *= -1.0
    if C > 8:
        gamma[(seed + C - 1) % C] = 0.0
    beta = 0.2 * g.standard_normal(C)
    beta[np.abs(beta) < 0.02] = 0.05
    da = g.standard_normal((B, C, H, W))
    return z.astype(np.float32), gamma.astype(np.float32), beta.astype(np.float32), da.astype(np.float32)


def stat_plan(HW):
    """(chunks, chunk_len) of the statistics / backward-reduce passes for one image plane (split_plan's rule in bn.hip)"""
    chunks = max(1, -(-HW // STAT_CHUNK))
    chunk_len = (-(-HW // chunks) + 3) & ~3
    return chunks, chunk_len


def partials(z):
    """the kernel's partials of z [B,C,H,W]: list of (b, beg, end) -- image x statistics chunk"""
    B, _, H, W = z.shape
    HW = H * W
    chunks, chunk_len = stat_plan(HW)
    return [(b, ch * chunk_len, min((ch + 1) * chunk_len, HW)) for b in range(B) for ch in range(chunks)]


def _per_c(x):
    return x[None, :, None, None]


def _sum_c(x):
    return x.sum(axis=(0, 2, 3))


def _finish(ref, z, s, invstd, mean, beta, da, E_mean, E_inv, training):
    """pre-activation, masked da, backward quantities and their bounds for statistics (mean, invstd) -- fp64"""
    N = z.shape[0] * z.shape[2] * z.shape[3]
    R = 4 * U + E_inv
    zc = z - _per_c(mean)
    xhat = zc * _per_c(invstd)
    pre = zc * _per_c(s) + _per_c(beta)
    a = np.maximum(pre, 0.0)
    tol_a = _per_c(np.abs(s)) * (_per_c(E_mean) + _per_c(R) * np.abs(zc)) + 2 * U * np.abs(a) + TINY
    undet = np.abs(pre) <= 4 * tol_a
    da = np.where(undet, np.float32(0), da).astype(np.float32)
    dy = da.astype(np.float64) * (pre > 0)
    sum_abs_dy = _sum_c(np.abs(dy))
    dbeta, dgamma = _sum_c(dy), _sum_c(dy * xhat)
    max_xhat = np.abs(xhat).max(axis=(0, 2, 3))
    tol_dbeta = 2 * U * np.abs(dbeta) + 2.0 ** -40 * sum_abs_dy + TINY
    tol_dgamma = (E_mean * invstd + R * max_xhat) * sum_abs_dy + 2 * U * np.abs(dgamma) + TINY
    if training:
        c1, c2 = dbeta / N, dgamma / N
        dz = _per_c(s) * (dy - _per_c(c1) - xhat * _per_c(c2))
        tol_dz = _per_c(np.abs(s)) * (_per_c(R) * (np.abs(dy) + _per_c(np.abs(c1)) + np.abs(xhat * _per_c(c2)))
                                      + _per_c(np.abs(c2)) * (_per_c(E_mean * invstd) + _per_c(R) * np.abs(xhat))
                                      + np.abs(xhat) * _per_c(tol_dgamma / N)) + U * np.abs(dz) + TINY
    else:                               # eval: dz = s dy; the affine gradients are still produced
        c1 = c2 = None
        dz = _per_c(s) * dy
        tol_dz = _per_c(np.abs(s) * R) * np.abs(dy) + U * np.abs(dz) + TINY
    ref.update(N=N, mean=mean, invstd=invstd, s=s, E_mean=E_mean, E_inv=E_inv, R=R, xhat=xhat, pre=pre, a=a, tol_a=tol_a, undet=undet,
               da=da, dy=dy, dbeta=dbeta, dgamma=dgamma, tol_dbeta=tol_dbeta, tol_dgamma=tol_dgamma, c1=c1, c2=c2, dz=dz, tol_dz=tol_dz,
               tol_mean=E_mean + TINY, tol_inv=E_inv + TINY)
    return ref


def train_ref(z, gamma, beta, da, z_apply=None, eps=EPS):
    """fp64 reference and bounds of train-mode BatchNorm + ReLU over ONE statistics group z [B,C,H,W] (fp32 arrays).
    z_apply: the values the apply / backward passes read when they differ from the ones the statistics were taken of (z stored as
    bf16): pre, xhat and the sums are evaluated on them, max|z| of E_mean is taken over them.
    -> dict; ref['da'] is da with zeros at the undetermined ReLU decisions."""
    z64, gamma, beta = z.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64)
    B, C, H, W = z.shape
    N = B * H * W
    mean = z64.mean(axis=(0, 2, 3))
    var = ((z64 - _per_c(mean)) ** 2).mean(axis=(0, 2, 3))
    invstd = 1.0 / np.sqrt(var + eps)
    unb = var * N / (N - 1) if N > 1 else var
    za = z64 if z_apply is None else z_apply.astype(np.float64)
    E_mean = 2 * U * np.abs(za).max(axis=(0, 2, 3))
    flat = z64.reshape(B, C, H * W)
    D = np.zeros(C)
    for b, beg, end in partials(z):
        D = np.maximum(D, np.abs(flat[b, :, beg:end].mean(axis=1) - mean))
    E_inv = 8 * U + 2 * E_mean * D / (var + eps)
    ref = dict(var=var, unb=unb, D=D, tol_unb=4 * U * unb + 2 * E_mean * D * (N / (N - 1) if N > 1 else 1.0))
    return _finish(ref, za, gamma * invstd, invstd, mean, beta, da, E_mean, E_inv, True)


def eval_ref(z, gamma, beta, da, running_mean, running_var, training_bwd=False, eps=EPS):
    """the same in eval mode: statistics = the running ones (save[0] is running_mean itself: E_mean = 0; invstd is computed in fp32 --
    one addition, a square root and a division, 3u relative)."""
    z64, gamma, beta = z.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64)
    mean, rv = running_mean.astype(np.float64), running_var.astype(np.float64)
    invstd = 1.0 / np.sqrt(rv + eps)
    C = z.shape[1]
    return _finish({}, z64, gamma * invstd, invstd, mean, beta, da, np.zeros(C), np.full(C, 3 * U), training_bwd)


def running_ref(rm, rv, ref, momentum=MOMENTUM):
    """-> (rm', tol), (rv', tol) after one train-mode update from `ref` (fp32 arrays rm, rv)"""
    rm, rv = rm.astype(np.float64), rv.astype(np.float64)
    m = momentum
    new_rm = (1 - m) * rm + m * ref["mean"]
    tol_rm = 3 * U * (np.abs(rm) + np.abs(ref["mean"])) + m * ref["E_mean"] + TINY
    new_rv = (1 - m) * rv + m * ref["unb"]
    tol_rv = 3 * U * (np.abs(rv) + np.abs(ref["unb"])) + m * ref["tol_unb"] + TINY
    return (new_rm, tol_rm), (new_rv, tol_rv)


def undetermined_share(ref):
    """per channel"""
    return ref["undet"].mean(axis=(0, 2, 3))


def bf16_round(x):
    """fp32 array -> the fp32 values of its bf16 rounding (to nearest even)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(x.shape)


# ------------------------------------------------------------------ comparison: which kernel, which quantity, which channel kind
RATIOS = {}                             # (entry point, quantity) -> worst err / tol seen (the profile table is printed from this)


def worst_ratio(got, want, tol):
    """-> (worst err / tol, channel) for arrays [C] or [B,C,H,W]; a NaN or infinity in `got` counts as infinitely wrong"""
    got = np.asarray(got, dtype=np.float64)
    want, tol = np.broadcast_to(want, got.shape), np.broadcast_to(tol, got.shape)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got - want) / tol
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    per_c = ratio if ratio.ndim == 1 else ratio.max(axis=(0, 2, 3))
    c = int(np.argmax(per_c))
    return float(per_c[c]), c


def check(entry, quantity, got, want, tol, table=RATIOS, kind=kind_of):
    """assert |got - want| <= tol everywhere; a failure names the kernel entry point, the channel kind and the worst err / tol"""
    r, c = worst_ratio(got, want, tol)
    key = (entry, quantity)
    if table is not None:
        table[key] = max(table.get(key, 0.0), r)
    assert r <= 1.0, f"{entry}: {quantity} of channel {c} ({kind(c)}) is off by {r:.3g} x its bound"
    return r


def format_ratios(table=RATIOS):
    return "\n".join(f"{e:34s} {q:14s} {r:.3g}" for (e, q), r in sorted(table.items()))


# ------------------------------------------------------------------ record-level references (the two finalize kernels)
def chan_merge(n, r, m2):
    """exact (fsum) fp64 Chan merge of fp32 records (n_k, r_k, M2_k): -> (n, mean, M2)"""
    n, r, m2 = (np.asarray(v, dtype=np.float64) for v in (n, r, m2))
    nt = math.fsum(n)
    mean = math.fsum(n * r) / nt
    return nt, mean, math.fsum(m2) + math.fsum(n * (r - mean) ** 2)


def block_records(z, block=512):
    """fp32 (n, mean, M2) records of consecutive `block`-element blocks of z [..., K * block] from their fp64 statistics"""
    v = z.astype(np.float64).reshape(z.shape[:-1] + (-1, block))
    mean = v.mean(axis=-1)
    m2 = ((v - mean[..., None]) ** 2).sum(axis=-1)
    return np.stack([np.full_like(mean, block), mean, m2], axis=-1).astype(np.float32)


def hi_lo(v):
    """fp64 -> (hi, lo) fp32 pair, the reduce kernels' record of one sum"""
    hi = v.astype(np.float32)
    return hi, (v - hi.astype(np.float64)).astype(np.float32)
