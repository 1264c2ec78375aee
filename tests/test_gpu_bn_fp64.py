"""The BatchNorm kernels of onet_amd/csrc/bn.hip against an fp64 reference on hostile statistics and edge shapes (tests/bn_cases.py:
inputs, reference and the per-channel bounds, each derived from the arithmetic; tests/test_bn_bounds_host.py shows on the CPU that
a faithful emulation meets them and that plausible mistakes do not).  Everything goes through onet_amd.ops; every output buffer is
NaN-filled first, so an element a kernel leaves unwritten fails.  A failure names the entry point, the channel kind and the worst
err / tol; `pytest -s` prints the worst ratio per entry point and quantity at the end of the module."""
import math

import numpy as np
import pytest
import torch

import bn_cases as bc

pytestmark = pytest.mark.gpu

U = bc.U
NAN = float("nan")
F64 = np.float64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from onet_amd import _lib
    _lib.load()
    yield torch.device("cuda:0")
    print("\nworst err / tol per entry point and quantity\n" + bc.format_ratios())


def host(t):
    return t.detach().cpu().numpy()


def nan(shape, dev):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device=dev)


def slot_max(slots):
    return float(host(slots).view(np.float32).max())


def put(x, dev, sliced=False):
    """fp32 array [B,C,H,W] on the device -- plain, or as channels SLICE_CH of a wider buffer whose other channels hold 1e30"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if not sliced:
        return t
    B, C, H, W = x.shape
    buf = torch.full((B, bc.SLICE_BUF, H, W), 1e30, dtype=torch.float32, device=dev)
    buf[:, bc.SLICE_CH] = t
    return buf[:, bc.SLICE_CH]


def out_buf(shape, dev, sliced=False):
    """NaN-filled destination -> (tensor to pass, whole buffer)"""
    B, C, H, W = shape
    if not sliced:
        t = nan(shape, dev)
        return t, t
    buf = nan((B, bc.SLICE_BUF, H, W), dev)
    return buf[:, bc.SLICE_CH], buf


def untouched_outside(buf, sliced):
    if sliced:
        rest = torch.ones(bc.SLICE_BUF, dtype=torch.bool)
        rest[bc.SLICE_CH] = False
        assert bool(torch.isnan(buf[:, rest.to(buf.device)]).all()), "a kernel wrote outside its channel slice"


# layouts: plain | z a channel slice | z, da and the outputs channel slices
CASES = [(s, "plain") for s in bc.SHAPES] + [(bc.SLICE_SHAPE, "z sliced"), (bc.SLICE_SHAPE, "all sliced")]
CASE_IDS = ["x".join(map(str, s)) + ("" if lay == "plain" else "-" + lay.replace(" ", "-")) for s, lay in CASES]
_REF = {}


def case(shape):
    """inputs and fp64 reference of one shape, computed once and shared (never modified)"""
    if shape not in _REF:
        z, gamma, beta, da = bc.make(*shape, seed=0)
        _REF[shape] = (z, gamma, beta, bc.train_ref(z, gamma, beta, da))
    return _REF[shape]


def running0(C):
    return np.linspace(-1, 1, C).astype(np.float32), np.linspace(0.5, 2, C).astype(np.float32)


def train_coeffs(ops, zd, gamma, beta, dev, rm=None, rv=None, save=None):
    C = gamma.shape[0]
    rm0, rv0 = running0(C)
    rm = torch.from_numpy(rm0).to(dev) if rm is None else rm
    rv = torch.from_numpy(rv0).to(dev) if rv is None else rv
    save = nan((4, C), dev) if save is None else save
    ops.bn_train_coeffs(zd, torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev), rm, rv, bc.MOMENTUM, bc.EPS, save=save)
    return save, rm, rv


def check_save(entry, save, ref, gamma, beta):
    sv = host(save)
    bc.check(entry, "mean", sv[0], ref["mean"], ref["tol_mean"])
    bc.check(entry, "invstd", sv[1].astype(F64) / ref["invstd"], 1.0, ref["tol_inv"])
    assert np.array_equal(sv[2], gamma * sv[1]), f"{entry}: scale is not fl32(gamma * invstd)"
    assert np.array_equal(sv[3], beta), f"{entry}: shift is not beta"


# ------------------------------------------------------------------ train mode
@pytest.mark.parametrize("shape,layout", CASES, ids=CASE_IDS)
def test_train_forward(dev, shape, layout):
    """onet_bn_stats_partial + onet_bn_finalize (statistics, coefficients, running statistics), onet_bn_relu_apply and, where the
    shape is taken, onet_bn_relu_apply_pool"""
    from onet_amd import ops
    z, gamma, beta, ref = case(shape)
    B, C, H, W = shape
    zd = put(z, dev, layout != "plain")
    save, rm, rv = train_coeffs(ops, zd, gamma, beta, dev)
    check_save("onet_bn_stats_partial+finalize", save, ref, gamma, beta)
    (rm_ref, tol_rm), (rv_ref, tol_rv) = bc.running_ref(*running0(C), ref)
    bc.check("onet_bn_finalize", "running_mean", host(rm), rm_ref, tol_rm)
    bc.check("onet_bn_finalize", "running_var", host(rv), rv_ref, tol_rv)

    a, buf = out_buf(shape, dev, layout == "all sliced")
    slots = ops.new_amax(dev)
    ops.bn_relu_apply(zd, save, out=a, amax=slots)
    bc.check("onet_bn_relu_apply", "a", host(a), ref["a"], ref["tol_a"])
    untouched_outside(buf, layout == "all sliced")
    assert slot_max(slots) == float(a.max()), "onet_bn_relu_apply: the magnitude slots do not hold max a"

    if H % 2 == 0 and W % 4 == 0:
        a2, buf2 = out_buf(shape, dev, layout == "all sliced")
        y = nan((B, C, H // 2, W // 2), dev)
        slots2 = ops.new_amax(dev)
        assert ops.bn_relu_apply_pool(zd, save, a2, y, amax=slots2), "onet_bn_relu_apply_pool did not take the shape"
        bc.check("onet_bn_relu_apply_pool", "a", host(a2), ref["a"], ref["tol_a"])
        untouched_outside(buf2, layout == "all sliced")
        pooled = host(a2).reshape(B, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))
        assert np.array_equal(host(y), pooled), "onet_bn_relu_apply_pool: y is not the 2x2 maximum of its own a"
        assert slot_max(slots2) == float(a2.max()), "onet_bn_relu_apply_pool: the magnitude slots do not hold max a"


@pytest.mark.parametrize("shape,layout", CASES, ids=CASE_IDS)
def test_train_backward(dev, shape, layout):
    """onet_bn_relu_bwd_reduce + onet_bn_bwd_finalize + onet_bn_relu_bwd_apply: dz, dgamma, dbeta; accumulating a second group;
    caller-provided affine gradient buffers; max |dz| in the magnitude slots"""
    from onet_amd import ops
    z, gamma, beta, ref = case(shape)
    C = shape[1]
    zd = put(z, dev, layout != "plain")
    dad = put(ref["da"], dev, layout == "all sliced")
    save, _, _ = train_coeffs(ops, zd, gamma, beta, dev)

    out, buf = out_buf(shape, dev, layout == "all sliced")
    slots = ops.new_amax(dev)
    dz, dgamma, dbeta = ops.bn_relu_bwd(dad, zd, save, True, out=out, amax=slots)
    assert dz is out
    bc.check("onet_bn_relu_bwd_reduce+finalize", "dbeta", host(dbeta), ref["dbeta"], ref["tol_dbeta"])
    bc.check("onet_bn_relu_bwd_reduce+finalize", "dgamma", host(dgamma), ref["dgamma"], ref["tol_dgamma"])
    bc.check("onet_bn_relu_bwd_apply", "dz", host(dz), ref["dz"], ref["tol_dz"])
    untouched_outside(buf, layout == "all sliced")
    assert slot_max(slots) == float(dz.abs().max()), "onet_bn_relu_bwd_apply: the magnitude slots do not hold max |dz|"

    # a second statistics group accumulates into the first one's sums: fl(prior + fl(sum)), one more rounding
    pg, pb = host(dgamma).astype(F64), host(dbeta).astype(F64)
    acc = (dgamma.clone(), dbeta.clone())
    dz2, g2, b2 = ops.bn_relu_bwd(dad, zd, save, True, acc=acc)
    assert g2 is acc[0] and b2 is acc[1] and torch.equal(dz2, dz)
    bc.check("onet_bn_bwd_finalize(accumulate)", "dbeta", host(b2), pb + ref["dbeta"], ref["tol_dbeta"] + U * np.abs(pb + ref["dbeta"]))
    bc.check("onet_bn_bwd_finalize(accumulate)", "dgamma", host(g2), pg + ref["dgamma"], ref["tol_dgamma"] + U * np.abs(pg + ref["dgamma"]))

    og, ob = nan((C,), dev), nan((C,), dev)
    dz3, g3, b3 = ops.bn_relu_bwd(dad, zd, save, True, affine_out=(og, ob))
    assert g3 is og and b3 is ob and torch.equal(dz3, dz) and torch.equal(og, dgamma) and torch.equal(ob, dbeta)


# ------------------------------------------------------------------ eval mode
@pytest.mark.parametrize("shape", [(3, 10, 7, 9), (2, 9, 50, 82)], ids=["3x10x7x9", "2x9x50x82"])
def test_eval(dev, shape):
    """onet_bn_eval_coeffs with running_var in {0, 1e-12, 1, 1e8} and running_mean up to 1e4 (invstd computed in fp32: 3u), the
    forward, and the backward with training=False: dz = s dy, dgamma and dbeta still produced"""
    from onet_amd import ops
    z, gamma, beta, da = bc.make(*shape, seed=0)
    C = shape[1]
    rm = z.astype(F64).mean(axis=(0, 2, 3)).astype(np.float32)
    rv = np.array([0.0, 1e-12, 1.0, 1e8], dtype=np.float32)[np.arange(C) % 4]
    assert np.abs(rm).max() > 9e3
    ref = bc.eval_ref(z, gamma, beta, da, rm, rv)
    zd, dad = put(z, dev), put(ref["da"], dev)
    save = nan((4, C), dev)
    ops.bn_eval_coeffs(torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev), torch.from_numpy(rm).to(dev),
                       torch.from_numpy(rv).to(dev), bc.EPS, save=save)
    assert np.array_equal(host(save)[0], rm), "onet_bn_eval_coeffs: mean is not running_mean"
    check_save("onet_bn_eval_coeffs", save, ref, gamma, beta)
    a = nan(shape, dev)
    ops.bn_relu_apply(zd, save, out=a)
    bc.check("onet_bn_relu_apply(eval)", "a", host(a), ref["a"], ref["tol_a"])
    out = nan(shape, dev)
    dz, dgamma, dbeta = ops.bn_relu_bwd(dad, zd, save, False, out=out)
    bc.check("onet_bn_relu_bwd_reduce+finalize(eval)", "dbeta", host(dbeta), ref["dbeta"], ref["tol_dbeta"])
    bc.check("onet_bn_relu_bwd_reduce+finalize(eval)", "dgamma", host(dgamma), ref["dgamma"], ref["tol_dgamma"])
    bc.check("onet_bn_relu_bwd_apply(eval)", "dz", host(dz), ref["dz"], ref["tol_dz"])


# ------------------------------------------------------------------ statistics groups
def test_statistics_groups(dev):
    """(4, 18, 16, 16) as two groups of 2 images whose statistics differ by an order of magnitude (swapped coefficients cannot
    pass): onet_bn_relu_apply(group_images = 2), and the reduce / finalize / apply launches over both groups of
    ops.bn_relu_bwd_groups, against the fp64 reference taken per group"""
    from onet_amd import ops
    shape = (4, 18, 16, 16)
    z, gamma, beta, da = bc.make(*shape, seed=0)
    z[2:] *= 8.0
    C = shape[1]
    refs = [bc.train_ref(z[2 * g:2 * g + 2], gamma, beta, da[2 * g:2 * g + 2]) for g in range(2)]
    assert np.all(np.abs(refs[1]["invstd"][[0, 5, 8]] * 8 / refs[0]["invstd"][[0, 5, 8]] - 1) < 0.2)
    zd = put(z, dev)
    save_all = nan((2, 4, C), dev)
    rm, rv = None, None
    for g in range(2):
        _, rm, rv = train_coeffs(ops, zd[2 * g:2 * g + 2], gamma, beta, dev, rm, rv, save=save_all[g])
        check_save("onet_bn_stats_partial+finalize", save_all[g], refs[g], gamma, beta)
    a = nan(shape, dev)
    ops.bn_relu_apply(zd, save_all, out=a, group_images=2)
    dad = put(np.concatenate([r["da"] for r in refs]), dev)
    dz, dgamma, dbeta = ops.bn_relu_bwd_groups(dad, zd, save_all, True, affine_out=(nan((C,), dev), nan((C,), dev)))
    for g in range(2):
        bc.check("onet_bn_relu_apply(groups)", "a", host(a[2 * g:2 * g + 2]), refs[g]["a"], refs[g]["tol_a"])
        bc.check("onet_bn_relu_bwd_apply(groups)", "dz", host(dz[2 * g:2 * g + 2]), refs[g]["dz"], refs[g]["tol_dz"])
    for q, got in (("dbeta", dbeta), ("dgamma", dgamma)):       # fl(fl(sum of group 0) + fl(sum of group 1))
        want = refs[0][q] + refs[1][q]
        bc.check("onet_bn_bwd_finalize(groups)", q, host(got), want, refs[0]["tol_" + q] + refs[1]["tol_" + q] + U * np.abs(want))


# ------------------------------------------------------------------ z stored as bf16
@pytest.mark.parametrize("shape", [(2, 9, 64, 64), (2, 9, 50, 82)], ids=["2x9x64x64", "2x9x50x82"])
def test_bf16_stored_z(dev, shape):
    """statistics from the fp32 z; onet_bn_relu_apply and onet_bn_relu_bwd_reduce then read z rounded to bf16.  Reference: fp64 on
    the rounded values, same bounds with max|z| over the rounded values."""
    from onet_amd import ops
    z, gamma, beta, da = bc.make(*shape, seed=0)
    zb = bc.bf16_round(z)
    ref = bc.train_ref(z, gamma, beta, da, z_apply=zb)
    zd = put(z, dev)
    z16 = zd.to(torch.bfloat16)
    assert np.array_equal(host(z16.float()), zb)
    save, _, _ = train_coeffs(ops, zd, gamma, beta, dev)
    a = nan(shape, dev)
    ops.bn_relu_apply(z16, save, out=a)
    bc.check("onet_bn_relu_apply(bf16 z)", "a", host(a), ref["a"], ref["tol_a"])
    coef, dgamma, dbeta = ops.bn_bwd_coefs(put(ref["da"], dev), z16, save, True)
    bc.check("onet_bn_relu_bwd_reduce(bf16 z)", "dbeta", host(dbeta), ref["dbeta"], ref["tol_dbeta"])
    bc.check("onet_bn_relu_bwd_reduce(bf16 z)", "dgamma", host(dgamma), ref["dgamma"], ref["tol_dgamma"])
    cf = host(coef).astype(F64)
    bc.check("onet_bn_relu_bwd_reduce(bf16 z)", "c1", cf[0] + cf[1], ref["c1"], ref["tol_dbeta"] / ref["N"])
    bc.check("onet_bn_relu_bwd_reduce(bf16 z)", "c2", cf[2] + cf[3], ref["c2"], ref["tol_dgamma"] / ref["N"])


# ------------------------------------------------------------------ onet_bn_finalize_cm on host-built records
CM_KINDS = ["mean=1e4 std=1", "std=1e3", "ordinary"]
_CM = {}


def cm_records(nrec, groups):
    """fp32 (n, mean, M2) records [C][groups * nrec][3] of 512-pixel blocks (group 1's values 8 x group 0's) and the exact fp64
    Chan merge of those records per group and channel"""
    key = (nrec, groups)
    if key not in _CM:
        g = np.random.Generator(np.random.PCG64([77, nrec, groups]))
        v = g.standard_normal((3, groups * nrec, 512), dtype=np.float32)
        v[0] += np.float32(1e4)
        v[1] *= np.float32(1e3)
        v[2] = v[2] * np.float32(2) + np.float32(0.7)
        if groups == 2:
            v[:, nrec:] *= np.float32(8)
        rec = bc.block_records(v.reshape(3, -1))
        merged = [[bc.chan_merge(*rec[c, gi * nrec:(gi + 1) * nrec].T) for c in range(3)] for gi in range(groups)]
        _CM[key] = (rec, merged)
    return _CM[key]


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("nrec", [300, 5000])
def test_finalize_cm(dev, nrec, groups):
    """300 and 5000 records per channel and group (more than the block's 256 threads and no multiple of them), taken from the
    middle of a larger record buffer; reference = the exact fp64 Chan merge of the same fp32 records: mean to u, invstd to 2u;
    running statistics updated group after group; the activation bound |gamma| sqrt(N - 1) 1.000001 + |beta| in the slots"""
    from onet_amd import ops
    rec, merged = cm_records(nrec, groups)
    C, first = 3, 7
    kind = lambda c: CM_KINDS[c]
    gamma, beta = np.array([1.25, -0.75, 0.5], dtype=np.float32), np.array([0.1, -0.3, 0.05], dtype=np.float32)
    buf = nan((C, first + groups * nrec + 5, 3), dev)
    buf[:, first:first + groups * nrec] = torch.from_numpy(rec).to(dev)
    rm0, rv0 = running0(C)
    rm, rv = torch.from_numpy(rm0).to(dev), torch.from_numpy(rv0).to(dev)
    save = nan((groups, 4, C) if groups > 1 else (4, C), dev)
    slots = ops.new_amax(dev)
    ops.bn_train_coeffs(torch.empty((2, C, 1, 1), device=dev), torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev), rm, rv,
                        bc.MOMENTUM, bc.EPS, cm=(buf, first, nrec), save=save, act_slots=slots, groups=groups)
    sv = host(save).reshape(groups, 4, C)
    m = bc.MOMENTUM
    rm_ref, rv_ref, tol_rm, tol_rv = rm0.astype(F64), rv0.astype(F64), np.zeros(C), np.zeros(C)
    for gi in range(groups):
        n, mean, m2 = (np.array([merged[gi][c][i] for c in range(C)]) for i in range(3))
        invstd, unb = 1.0 / np.sqrt(m2 / n + bc.EPS), m2 / (n - 1)
        e = f"onet_bn_finalize_cm(groups={groups})"
        bc.check(e, "mean", sv[gi, 0], mean, U * np.abs(mean) + bc.TINY, kind=kind)
        bc.check(e, "invstd", sv[gi, 1].astype(F64) / invstd, 1.0, 2 * U, kind=kind)
        assert np.array_equal(sv[gi, 2], gamma * sv[gi, 1]) and np.array_equal(sv[gi, 3], beta)
        tol_rm = (1 - m) * tol_rm + 3 * U * (np.abs(rm_ref) + np.abs(mean)) + m * U * np.abs(mean)
        tol_rv = (1 - m) * tol_rv + 3 * U * (np.abs(rv_ref) + unb) + m * U * unb
        rm_ref, rv_ref = (1 - m) * rm_ref + m * mean, (1 - m) * rv_ref + m * unb
    bc.check(e, "running_mean", host(rm), rm_ref, tol_rm, kind=kind)
    bc.check(e, "running_var", host(rv), rv_ref, tol_rv, kind=kind)
    bound = np.abs(gamma.astype(F64)) * np.sqrt(n - 1) * float(np.float32(1.000001)) + np.abs(beta.astype(F64))
    got = host(slots).view(np.float32)[np.arange(C) * 32]
    bc.check(e, "act bound", got, bound, 2 * U * bound, kind=kind)


# ------------------------------------------------------------------ onet_bn_bwd_finalize on synthetic (hi, lo, hi, lo) records
def _fsum(x):
    return math.fsum(np.asarray(x, dtype=F64).ravel())


@pytest.mark.parametrize("accumulate", [0, 1])
def test_bwd_finalize_records(dev, accumulate):
    """groups = 2, accumulate in {0, 1}, 300 records per group: dgamma / dbeta against the fp64 sum of the records -- one u per
    fp32 rounding of the chain acc (+)= fl(sum of group g), which is 2u relative for a single group, plus 2^-40 sum|record| --
    and coef (hi + lo) against sum / count to 2^-45.  Also through ops.bn_bwd_coefs(red4=, acc=) and ops.bn_relu_bwd_groups(rec4=)."""
    from onet_amd import ops
    G, NP, C, count = 2, 300, 5, 2 * 64 * 64
    g = np.random.Generator(np.random.PCG64([91, G, NP, C]))
    v = (0.5 + g.standard_normal((G, NP, C, 2))) * np.array([1.0, 1e3, 1e-3, -7.0, 30.0])[None, None, :, None]
    rec = np.empty((G, NP, C, 4), dtype=np.float32)
    rec[..., 0], rec[..., 1] = bc.hi_lo(v[..., 0])
    rec[..., 2], rec[..., 3] = bc.hi_lo(v[..., 1])
    r64 = rec.astype(F64)
    s = np.array([[[_fsum(r64[gi, :, c, 2 * q:2 * q + 2]) for c in range(C)] for gi in range(G)] for q in range(2)])   # [q][g][c]
    sabs = np.abs(r64).reshape(G, NP, C, 2, 2).sum(axis=(1, 4))                                                          # [g][c][q]
    prior = np.stack([np.linspace(-3, 5, C), np.linspace(40, -2, C)]).astype(np.float32)                                # [q][c]: dbeta, dgamma
    kind = lambda c: f"record scale #{c}"

    def expect(q, groups):
        total = prior[q].astype(F64) if accumulate else np.zeros(C)
        tol = np.zeros(C)
        for gi in groups:
            adds = accumulate or gi != groups[0]
            total = total + s[q, gi]
            tol = tol + U * np.abs(s[q, gi]) + (U * np.abs(total) if adds else 0.0) + 2.0 ** -40 * sabs[gi, :, q]
        return total, tol + bc.TINY

    def check(entry, groups, dbeta, dgamma, coef):
        for q, (name, got) in enumerate((("dbeta", dbeta), ("dgamma", dgamma))):
            want, tol = expect(q, groups)
            bc.check(entry, name, host(got), want, tol, kind=kind)
        cf = host(coef).astype(F64).reshape(len(groups), 4, C)
        for i, gi in enumerate(groups):
            for q, name in enumerate(("c1", "c2")):
                want = s[q, gi] / count
                bc.check(entry, name, cf[i, 2 * q] + cf[i, 2 * q + 1], want, 2.0 ** -45 * np.abs(want), kind=kind)

    recd = torch.from_numpy(rec.reshape(G * NP, C, 4)).to(dev)
    zd = torch.zeros((2, C, 64, 64), device=dev)
    save = torch.ones((4, C), device=dev)
    acc = lambda: (torch.from_numpy(prior[1].copy()).to(dev), torch.from_numpy(prior[0].copy()).to(dev)) if accumulate else None

    # both groups in one launch, straight through the entry point ops uses (ops passes accumulate = 0 with groups > 1)
    dg, db = acc() or (nan((C,), dev), nan((C,), dev))
    coef = nan((G, 4, C), dev)
    ops._lib.call("onet_bn_bwd_finalize", recd.data_ptr(), NP, count, dg.data_ptr(), db.data_ptr(), coef.data_ptr(), accumulate, G, C,
                  None, None, None, torch.cuda.current_stream().cuda_stream)
    check(f"onet_bn_bwd_finalize(groups=2,accumulate={accumulate})", [0, 1], db, dg, coef)

    # one group (the second: records 300 ..) through ops.bn_bwd_coefs(red4=), accumulating or not
    coef1, dg1, db1 = ops.bn_bwd_coefs(zd, zd, save, True, acc=acc(), red4=(recd, NP, NP))
    check(f"onet_bn_bwd_finalize(groups=1,accumulate={accumulate})", [1], db1, dg1, coef1)

    if not accumulate:          # ops.bn_relu_bwd_groups(rec4=): the same launch as the direct one, then the apply pass
        save_all = torch.ones((G, 4, C), device=dev)
        z4 = torch.zeros((4, C, 64, 64), device=dev)
        dz, dg2, db2 = ops.bn_relu_bwd_groups(z4, z4, save_all, True, rec4=recd)
        assert torch.equal(dg2, dg) and torch.equal(db2, db) and bool(torch.isfinite(dz).all())


# ------------------------------------------------------------------ plans with an empty chunk are refused
def test_plan_with_an_empty_chunk_is_refused(dev):
    """HW = 9 cut into 4 chunks: chunk_len rounds up to 4 and the fourth chunk would begin at 12, past the plane.  Both public
    entry points refuse the plan with the bad-argument code and leave the NaN-filled record buffers untouched.  (The inputs
    carry spare channels, so that even a library without the check would have stayed inside the allocations.)"""
    from onet_amd import _lib
    lib = _lib.load()
    B, C, HW, nparts = 1, 2, 9, 4
    z = torch.zeros((B, C + 2, 3, 3), device=dev)
    da = torch.zeros_like(z)
    save = torch.ones((4, C), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    part, part2 = nan((nparts, C, 3), dev), nan((nparts, C, 4), dev)
    assert lib.onet_bn_stats_partial(z.data_ptr(), (C + 2) * HW, part.data_ptr(), nparts, B, C, HW, st) == -1
    assert "bn_stats_partial" in _lib.last_error()
    assert lib.onet_bn_relu_bwd_reduce(da.data_ptr(), (C + 2) * HW, z.data_ptr(), 0, (C + 2) * HW, save.data_ptr(), part2.data_ptr(), nparts,
                                       None, 0, B, C, HW, st) == -1
    assert "bn_relu_bwd_reduce" in _lib.last_error()
    with pytest.raises(_lib.OnetHipError):
        _lib.call("onet_bn_stats_partial", z.data_ptr(), (C + 2) * HW, part.data_ptr(), nparts, B, C, HW, st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(part2).all())
    # the plans ops makes, and the largest legal cut of this plane (3 chunks of 4, 4 and 1), still pass
    assert lib.onet_bn_stats_partial(z.data_ptr(), (C + 2) * HW, part.data_ptr(), 3, B, C, HW, st) == 0
    torch.cuda.synchronize()
    assert host(part)[:3, :, 0].tolist() == [[4.0] * C, [4.0] * C, [1.0] * C] and bool(torch.isnan(part[3]).all())
