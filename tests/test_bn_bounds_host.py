"""The bounds of tests/bn_cases.py are neither vacuous nor wrong (no GPU needed): a numpy emulation that follows the algorithm of
onet_amd/csrc/bn.hip step by step -- fp64 pivot-shifted sums per partial, the fp32 record (n, fl(mean_k), fl(M2 about the ROUNDED
mean)), the fp64 merge, fp32 invstd / scale / t = fl(z - mean) / fma, fp64 backward sums through (hi, lo) records and dz evaluated in
fp64 -- satisfies every bound on every case, and each of six plausible mistakes breaks the bound it should.
(`pytest -s` prints the emulation's worst err / tol per quantity.)"""
import numpy as np
import pytest

import bn_cases as bc

F32, F64 = np.float32, np.float64
HOST_RATIOS = {}
CASE_IDS = ["x".join(map(str, s)) for s in bc.SHAPES]


def _case(shape, seed=0):
    return bc.make(*shape, seed=seed)


# ------------------------------------------------------------------ the emulation
def emu_stats(z, variant=None, eps=bc.EPS):
    """statistics pass + finalize: -> dict(mean fp32, invstd fp32, unb fp64 (what the running variance takes))"""
    B, C, H, W = z.shape
    HW, N = H * W, B * H * W
    flat = z.reshape(B, C, HW)
    if variant == "fp32_ez2":                       # E[z^2] - mean^2 with running fp32 sums
        v = flat.transpose(1, 0, 2).reshape(C, N)
        s = np.cumsum(v, axis=1, dtype=F32)[:, -1]
        q = np.cumsum(v * v, axis=1, dtype=F32)[:, -1]
        mean = s / F32(N)
        var = np.maximum(q / F32(N) - mean * mean, F32(0))
        return dict(mean=mean, invstd=(F32(1) / np.sqrt(var + F32(eps))).astype(F32), unb=var.astype(F64))
    recs = []
    for b, beg, end in bc.partials(z):
        if variant == "skip4" and end == HW and end - beg > 4:
            end -= 4
        seg = flat[b, :, beg:end].astype(F64)
        n = float(end - beg)
        pivot = seg[:, :1]
        d = seg - pivot
        s1, s2 = d.sum(axis=1), (d * d).sum(axis=1)
        mean = pivot[:, 0] + s1 / n
        m2 = np.maximum(s2 - s1 * s1 / n, 0.0)
        r = mean.astype(F32)
        recs.append((np.full(C, n, dtype=F32), r, (m2 + n * (mean - r.astype(F64)) ** 2).astype(F32)))
    nk, rk, mk = (np.stack([rec[i] for rec in recs]).astype(F64) for i in range(3))       # [parts, C]
    n = nk.sum(axis=0)
    mean = (nk * rk).sum(axis=0) / n
    m2 = mk.sum(axis=0)
    if variant != "no_between":
        m2 = m2 + (nk * (rk - mean) ** 2).sum(axis=0)
    var = m2 / n
    unb = np.where(n > 1, m2 / np.maximum(n - 1, 1), var)
    if variant == "unbiased":
        var = unb
    return dict(mean=mean.astype(F32), invstd=(1.0 / np.sqrt(var + eps)).astype(F32), unb=unb)


def emu_save(st, gamma, beta):
    """save [4][C] = (mean, invstd, scale = fl(gamma invstd), shift) in fp32"""
    return st["mean"], st["invstd"], (gamma * st["invstd"]).astype(F32), beta.astype(F32)


def _pre32(z, save):
    mean, _, sc, sh = (v[None, :, None, None] for v in save)
    t = (z - mean).astype(F32)                                                    # t = fl(z - mean)
    return (t.astype(F64) * sc.astype(F64) + sh.astype(F64)).astype(F32)          # fma: one rounding (the product is exact in fp64)


def emu_apply(z, save):
    return np.maximum(_pre32(z, save), F32(0))


def emu_bwd(z, da, save, training=True, variant=None, stat_parts=None):
    """reduce (fp64 sums per partial -> (hi, lo) fp32 records), finalize, apply: -> dz fp32, dgamma fp32, dbeta fp32"""
    B, C, H, W = z.shape
    HW, N = H * W, B * H * W
    mean, invstd, sc, _ = (v.astype(F64)[None, :, None, None] for v in save)
    dy = np.where(_pre32(z, save) > 0, da.astype(F64), 0.0)
    xhat = (z.astype(F64) - mean) * invstd
    s = np.zeros(C)
    sx = np.zeros(C)
    f_dy, f_x = dy.reshape(B, C, HW), (dy * xhat).reshape(B, C, HW)
    for b, beg, end in (stat_parts or bc.partials(z)):
        for acc, src in ((s, f_dy), (sx, f_x)):
            hi, lo = bc.hi_lo(src[b, :, beg:end].sum(axis=1))
            acc += hi.astype(F64) + lo.astype(F64)
    if variant == "fp32_dbeta":                     # a running fp32 sum of dy over the channel
        s = np.cumsum(dy.transpose(1, 0, 2, 3).reshape(C, N).astype(F32), axis=1, dtype=F32)[:, -1].astype(F64)
    if training:
        c1, c2 = (sum(v.astype(F64) for v in bc.hi_lo(t / N))[None, :, None, None] for t in (s, sx))
        dz = (sc * (dy - c1 - xhat * c2)).astype(F32)
    else:
        dz = (sc * dy).astype(F32)
    return dz, sx.astype(F32), s.astype(F32)


def emu_running(rm, rv, st, m=bc.MOMENTUM):
    m = F32(m)
    return (F32(1) - m) * rm + m * st["mean"], (F32(1) - m) * rv + m * st["unb"].astype(F32)


def check_all(tag, z, gamma, beta, da, z_apply=None, table=None):
    """the whole train-mode chain of the emulation against every bound"""
    ref = bc.train_ref(z, gamma, beta, da, z_apply=z_apply)
    za = z if z_apply is None else z_apply
    st = emu_stats(z)
    save = emu_save(st, gamma, beta)
    rm0, rv0 = np.linspace(-1, 1, z.shape[1]).astype(F32), np.linspace(0.5, 2, z.shape[1]).astype(F32)
    rm1, rv1 = emu_running(rm0, rv0, st)
    (rm_ref, tol_rm), (rv_ref, tol_rv) = bc.running_ref(rm0, rv0, ref)
    dz, dgamma, dbeta = emu_bwd(za, ref["da"], save, stat_parts=bc.partials(z))
    t = table if table is not None else HOST_RATIOS
    bc.check(tag, "mean", save[0], ref["mean"], ref["tol_mean"], t)
    bc.check(tag, "invstd", save[1] / ref["invstd"], 1.0, ref["tol_inv"], t)
    bc.check(tag, "running_mean", rm1, rm_ref, tol_rm, t)
    bc.check(tag, "running_var", rv1, rv_ref, tol_rv, t)
    bc.check(tag, "a", emu_apply(za, save), ref["a"], ref["tol_a"], t)
    bc.check(tag, "dbeta", dbeta, ref["dbeta"], ref["tol_dbeta"], t)
    bc.check(tag, "dgamma", dgamma, ref["dgamma"], ref["tol_dgamma"], t)
    bc.check(tag, "dz", dz, ref["dz"], ref["tol_dz"], t)
    return ref


# ------------------------------------------------------------------ the faithful emulation meets every bound
@pytest.mark.parametrize("shape", bc.SHAPES, ids=CASE_IDS)
def test_emulation_meets_every_bound(shape):
    check_all("emulation", *_case(shape))
    print("\n" + bc.format_ratios(HOST_RATIOS))


@pytest.mark.parametrize("shape", [(2, 9, 64, 64), (2, 9, 50, 82)], ids=["2x9x64x64", "2x9x50x82"])
def test_emulation_meets_every_bound_bf16_z(shape):
    z, gamma, beta, da = _case(shape)
    check_all("emulation bf16 z", z, gamma, beta, da, z_apply=bc.bf16_round(z))
    print("\n" + bc.format_ratios(HOST_RATIOS))


def test_emulation_meets_every_bound_eval():
    z, gamma, beta, da = _case((3, 10, 7, 9))
    C = z.shape[1]
    rm = z.astype(F64).mean(axis=(0, 2, 3)).astype(F32)
    rv = np.array([0.0, 1e-12, 1.0, 1e8], dtype=F32)[np.arange(C) % 4]
    ref = bc.eval_ref(z, gamma, beta, da, rm, rv)
    invstd = (F32(1) / np.sqrt(rv + F32(bc.EPS))).astype(F32)
    save = (rm, invstd, (gamma * invstd).astype(F32), beta)
    dz, dgamma, dbeta = emu_bwd(z, ref["da"], save, training=False)
    bc.check("emulation eval", "invstd", invstd / ref["invstd"], 1.0, ref["tol_inv"], HOST_RATIOS)
    bc.check("emulation eval", "a", emu_apply(z, save), ref["a"], ref["tol_a"], HOST_RATIOS)
    bc.check("emulation eval", "dbeta", dbeta, ref["dbeta"], ref["tol_dbeta"], HOST_RATIOS)
    bc.check("emulation eval", "dgamma", dgamma, ref["dgamma"], ref["tol_dgamma"], HOST_RATIOS)
    bc.check("emulation eval", "dz", dz, ref["dz"], ref["tol_dz"], HOST_RATIOS)


# ------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", bc.SHAPES, ids=CASE_IDS)
def test_undetermined_relu_decisions_stay_rare(shape, seed):
    z, gamma, beta, da = _case(shape, seed)
    refs = [bc.train_ref(z, gamma, beta, da)]
    if z.shape[2] * z.shape[3] >= 4096 and z.shape[3] % 2 == 0:
        refs.append(bc.train_ref(z, gamma, beta, da, z_apply=bc.bf16_round(z)))
    for ref in refs:
        share = bc.undetermined_share(ref)
        c = int(np.argmax(share))
        assert share[c] <= 0.03, f"{share[c]:.3%} of channel {c} ({bc.kind_of(c)}) is within 4 tol_a of the ReLU kink"
        assert np.array_equal(ref["da"] == 0, ref["undet"] | (da == 0))


@pytest.mark.parametrize("shape", bc.SHAPES + [(1, 1, 3, 3)], ids=CASE_IDS + ["1x1x3x3"])
def test_every_partial_is_non_empty(shape):
    z = np.zeros(shape, dtype=F32)
    parts = bc.partials(z)
    HW = shape[2] * shape[3]
    assert all(0 <= beg < end <= HW for _, beg, end in parts)
    assert sum(end - beg for _, beg, end in parts) == shape[0] * HW
    assert len(parts) == shape[0] * max(1, -(-HW // 16384))
    if shape == (1, 9, 131, 129):
        assert bc.stat_plan(HW) == (2, 8452)


# ------------------------------------------------------------------ wrong variants must break the bound they should
def _ratio(got, want, tol):
    return bc.worst_ratio(got, want, tol)[0]


def _of_kind(k, C):
    return [c for c in range(C) if c % 9 == k]


@pytest.mark.parametrize("shape", bc.SHAPES, ids=CASE_IDS)
def test_wrong_variants_break_their_bound(shape):
    z, gamma, beta, da = _case(shape)
    B, C, H, W = shape
    HW, N = H * W, B * H * W
    ref = bc.train_ref(z, gamma, beta, da)

    def inv_ratio(variant, channels=None):
        st = emu_stats(z, variant)
        sel = slice(None) if channels is None else channels
        return _ratio((st["invstd"] / ref["invstd"])[sel], 1.0, ref["tol_inv"][sel]), _ratio(st["mean"][sel], ref["mean"][sel], ref["tol_mean"][sel])

    if N >= 63:                                     # fp32 E[z^2] - mean^2: the variance of |mean| >> std drowns
        assert inv_ratio("fp32_ez2", _of_kind(0, C))[0] >= 100.0
    if HW >= 63:
        # a running fp32 sum of dy.  Its error is a random walk of half-ulps of the running sum against a bound of 2u |dbeta|: how far
        # it overshoots depends on how small |dbeta| happens to come out in some channel, so with N = 189 (3x10x7x9) a single draw
        # decides little (worst channel of seeds 0..3: 4.2, 5.0, 3.0, 20.7 x the bound; every larger case >= 9.6 x on every seed).
        # The statement is made per case over the four seeds the input conditions are asserted for.
        worst = 0.0
        for seed in range(4):
            zs, gs, bs, das = _case(shape, seed)
            rs = bc.train_ref(zs, gs, bs, das)
            dbeta = emu_bwd(zs, rs["da"], emu_save(emu_stats(zs), gs, bs), variant="fp32_dbeta")[2]
            worst = max(worst, _ratio(dbeta, rs["dbeta"], rs["tol_dbeta"]))
        assert worst >= 8.0
    if HW > 4:                                      # statistics that skip the last 4 elements of a plane
        r_inv, r_mean = inv_ratio("skip4")
        assert r_inv > 1.0 and r_mean > 1.0
    assert inv_ratio("unbiased")[0] > 1.0           # N / (N - 1), N = 2 included
    if B > 1:                                       # all of kind 3's variance lies between the partials
        assert inv_ratio("no_between", _of_kind(3, C))[0] > 1.0


def _two_groups():
    """(4, 18, 16, 16) as two statistics groups of 2 images whose statistics differ by an order of magnitude"""
    z, gamma, beta, da = _case((4, 18, 16, 16))
    z[2:] *= 8.0
    return z, gamma, beta, da


def test_swapped_group_coefficients_break_the_bound():
    z, gamma, beta, da = _two_groups()
    saves = []
    for g in range(2):
        zg, dag = z[2 * g:2 * g + 2], da[2 * g:2 * g + 2]
        ref = check_all("emulation groups", zg, gamma, beta, dag)
        assert bc.undetermined_share(ref).max() <= 0.03
        saves.append(emu_save(emu_stats(zg), gamma, beta))
    assert _ratio(emu_apply(z[2:], saves[0]), ref["a"], ref["tol_a"]) > 1.0       # group 0's coefficients on group 1
    assert _ratio(emu_apply(z[2:], saves[1]), ref["a"], ref["tol_a"]) <= 1.0
