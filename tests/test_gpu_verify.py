"""The SNR-gain report and the two-stage cascade on the device (ops.snr_moments / ops.cascade_input, onet_amd.verify_step / EvalSnr /
cascade_input / verify_cascade; include/onet_hip_verify.h).

Kernel level (K): the kernel's own constants pick the shapes -- 1024 pixels per block and step, at most 64 blocks per image -- one pixel,
less than a wave, either side of 256, one pixel (and, for the wide loads, four) past one block's chunk, and past the 64 x 1024 stride
where block 0 takes a second step.  minmax and the maxima are bit patterns: exact.  The sums are fp64 sums of fp64 squares of the fp32
values metrics.tensor_normal_per_frame gives (the same __device__ function): against NumPy's float64 sum of the same squares they differ
by summation order alone, at most 2^21 additions here: 2^21 * 2^-53 = 2.4e-10 relative, bound 1e-9 (all terms are >= 0: no
cancellation).  The cascade's input is the bits of metrics.tensor_normal_per_frame of the selected map.

Model level (M): verify_step against validate on the same model, input and settings (counts, labels, Vt, Vd bit for bit, the same
convolution launches: one forward), its moments against those recomputed from its own Vt, Vd, EvalCounts + EvalSnr through
metrics.snr_report, verify_cascade against the manual composition, and validate's launch records, unchanged.
dB bound of a report recomputed from sums within 1e-9 relative: three such sums enter a ratio, 10 log10(1 + 3e-9) = 1.3e-8 dB; 2e-8."""
import numpy as np
import pytest
import torch

import test_verify_host as vh

pytestmark = pytest.mark.gpu

CHUNK, PARTS = 1024, 64                     # evalside.hip: COUNTS_CHUNK, FRAME_PARTS
SHAPES = [(1, 1, 1), (1, 1, 7), (2, 1, 255), (1, 16, 16), (3, 1, 257), (2, 25, 41), (1, 4, 257), (1, 1, PARTS * CHUNK + 1),
          (2, 4, PARTS * CHUNK // 4 + 1)]
DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float32]
SENTINEL = -7777.0
SUM_RTOL = 1e-9
DB_TOL = 2e-8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from onet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _maps(B, H, W, seed=0):
    """X, Vt, Vd fp32 [B, 1, H, W] and gt uint8 [B, H, W] on the host: V of either sign, X in [-0.2, 1], about a third of the pixels
    positive (a one-pixel image: positive)"""
    g = np.random.Generator(np.random.PCG64([seed, B, H, W]))
    X = (g.random((B, 1, H, W)) * 1.2 - 0.2).astype(np.float32)
    Vt = (g.standard_normal((B, 1, H, W)) * 3 - 1).astype(np.float32)
    Vd = (g.standard_normal((B, 1, H, W)) * 0.01 + 40).astype(np.float32)
    gt = (g.random((B, H, W)) > 0.65).astype(np.uint8)
    if H * W == 1:
        gt[:] = 1
    return tuple(torch.from_numpy(a) for a in (X, Vt, Vd, gt))


def _expected(X, Vt, Vd, gt):
    """(minmax fp32 [B, 4], moment rows float64 [B, 9]) of device maps: amin / amax, and NumPy's float64 sums and fp32 maxima of the
    fp32 maps metrics.tensor_normal_per_frame gives"""
    from onet_amd import metrics
    B = Vt.shape[0]
    vt, vd = Vt.reshape(B, -1), Vd.reshape(B, -1)
    minmax = torch.stack([vt.amin(1), vt.amax(1), vd.amin(1), vd.amax(1)], dim=1)
    nt, nd = metrics.tensor_normal_per_frame(Vt.contiguous()), metrics.tensor_normal_per_frame(Vd.contiguous())
    rows = vh.moment_rows(None if X is None else X.cpu().numpy(), nt.cpu().numpy(), nd.cpu().numpy(), gt.cpu().numpy())
    return minmax, rows


def _assert_rows(got, want, what):
    """maxima bit for bit, sums within SUM_RTOL relative (a sum of nothing: exactly 0)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(got[:, 2::3], want[:, 2::3]), (what, got[:, 2::3], want[:, 2::3])
    for k in (0, 1, 3, 4, 6, 7):
        err = np.abs(got[:, k] - want[:, k])
        assert np.all(err <= SUM_RTOL * want[:, k]), (what, k, got[:, k], want[:, k])
    sums = want[:, [0, 1, 3, 4, 6, 7]]
    return float((np.abs(got[:, [0, 1, 3, 4, 6, 7]] - sums) / np.where(sums > 0, sums, 1)).max())


def _check_moments(dev, X, Vt, Vd, gt, what):
    """ops.snr_moments on device maps (any layout the binding takes) into rows 2.. of a sentinel-filled tensor"""
    from onet_amd import ops
    B = Vt.shape[0]
    want_mm, want = _expected(X, Vt, Vd, gt)
    row = 2
    moments = torch.full((B + 3, 9), SENTINEL, dtype=torch.float64, device=dev)
    minmax = ops.snr_moments(X, Vt, Vd, gt, moments, row=row)
    torch.cuda.synchronize()
    assert minmax.dtype == torch.float32 and tuple(minmax.shape) == (B, 4) and torch.equal(minmax, want_mm), (what, minmax, want_mm)
    got = moments.cpu().numpy()
    worst = _assert_rows(got[row:row + B], want, what)
    assert (got[:row] == SENTINEL).all() and (got[row + B:] == SENTINEL).all(), what          # written, and nothing else touched
    if X is None:
        assert (got[row:row + B, :3] == 0).all(), what
    # a second run into fresh rows, a caller's minmax: the same bits
    again, mm2 = torch.full((B, 9), 3.0, dtype=torch.float64, device=dev), torch.empty((B, 4), dtype=torch.float32, device=dev)
    assert ops.snr_moments(X, Vt, Vd, gt, again, minmax=mm2) is mm2
    assert torch.equal(again, moments[row:row + B]) and torch.equal(mm2, minmax), what
    print(f"{what}: worst relative error of a sum {worst:.2e}")
    return moments[row:row + B], minmax


# ----------------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_k1_moments_at_the_path_edges(dev, shape):
    """every shape: contiguous maps, uint8 ground truth (the wide loads where HW % 4 == 0, scalar loads elsewhere)"""
    X, Vt, Vd, gt = (t.to(dev) for t in _maps(*shape))
    assert int(gt.sum()) > 0
    _check_moments(dev, X, Vt, Vd, gt, f"K1 {shape}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", [(3, 16, 20), (2, 25, 41)], ids=["wide", "scalar"])
def test_k2_batch_strided_ground_truth_and_input(dev, shape, dtype):
    """gt a channel of a wider tensor (batch stride 3 HW) in each dtype, X likewise; an image without a positive pixel"""
    B, H, W = shape
    X, Vt, Vd, gt = _maps(*shape, seed=2)
    gt[1] = 0
    wide_gt = torch.zeros((B, 3, H, W), dtype=dtype, device=dev)
    wide_gt[:, 1] = gt.to(dtype).to(dev)
    wide_gt[:, 0] = 1
    wide_x = torch.full((B, 3, H, W), 9.0, dtype=torch.float32, device=dev)
    wide_x[:, 2:] = X.to(dev)
    g, x = wide_gt[:, 1], wide_x[:, 2:]
    assert g.stride(0) == 3 * H * W and x.stride(0) == 3 * H * W and not x.is_contiguous()
    rows, _ = _check_moments(dev, x, Vt.to(dev), Vd.to(dev), g, f"K2 {shape} {dtype}")
    assert (rows[1, [0, 2, 3, 5, 6, 8]] == 0).all()


def test_k3_unaligned_base_pointers_and_no_input(dev):
    """HW % 4 == 0 but every map starts 4 (gt: 1) bytes past an aligned address: the scalar path; then X = None"""
    B, H, W = 2, 16, 72                                 # 1152 pixels: two blocks per image
    X, Vt, Vd, gt = _maps(B, H, W, seed=3)
    n = B * H * W

    def shifted(t):
        buf = torch.zeros(n + 1, dtype=t.dtype, device=dev)
        buf[1:] = t.reshape(-1).to(dev)
        out = buf[1:].view(t.shape)
        assert out.data_ptr() % 16 != 0 and out.is_contiguous()
        return out
    x, vt, vd, g = shifted(X), shifted(Vt), shifted(Vd), shifted(gt)
    r1, _ = _check_moments(dev, x, vt, vd, g, "K3 unaligned")
    r0, _ = _check_moments(dev, X.to(dev), Vt.to(dev), Vd.to(dev), gt.to(dev), "K3 aligned")
    _assert_rows(r1.cpu().numpy(), r0.cpu().numpy(), "K3 unaligned against aligned")
    r2, _ = _check_moments(dev, None, vt, Vd.to(dev), g, "K3 no X")
    assert torch.equal(r2[:, 3:6], r1[:, 3:6])          # (n(Vt) took the scalar path both times: the same order, the same bits)


def test_k4_bindings_refuse_bad_arguments(dev):
    from onet_amd import ops
    X, Vt, Vd, gt = (t.to(dev) for t in _maps(2, 8, 8))
    mom = torch.zeros((2, 9), dtype=torch.float64, device=dev)
    cnt = torch.zeros((2, 4), dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.snr_moments(X, Vt[:, 0], Vd[:, 0], gt, mom)
    with pytest.raises(ValueError):
        ops.snr_moments(X.expand(2, 3, 8, 8), Vt, Vd, gt, mom)
    with pytest.raises(ValueError):
        ops.snr_moments(X, Vt, Vd, gt, mom, row=1)
    with pytest.raises(ValueError):
        ops.snr_moments(X, Vt, Vd, gt, mom.float())
    with pytest.raises(ValueError):
        ops.snr_moments(X, Vt, Vd, gt[:1], mom)
    with pytest.raises(TypeError):
        ops.snr_moments(X, Vt, Vd, gt.to(torch.int16), mom)
    with pytest.raises(ValueError):
        ops.snr_moments(X, Vt, Vd, gt, mom, minmax=torch.zeros((2, 3), device=dev))
    with pytest.raises(ValueError):
        ops.cascade_input(Vt, Vd, cnt[:1])
    with pytest.raises(ValueError):
        ops.cascade_input(Vt, Vd, cnt.int())
    with pytest.raises(ValueError):
        ops.cascade_input(Vt, Vd, cnt, out=torch.zeros((2, 1, 8, 4), device=dev))
    with pytest.raises(RuntimeError):
        ops.cascade_input(Vt.cpu(), Vd, cnt)


@pytest.fixture(scope="module")
def golden(dev):
    """the fixture's batches on the device with the counts ops.score_counts gives them: computed once, never modified"""
    from onet_amd import ops
    g, sizes, mom, cnt, _ = vh.load_fixture()
    out, r0 = [], 0
    for b, n in enumerate(sizes):
        X, Vt, Vd, gt = (torch.from_numpy(g[f"{k}{b}"]).to(dev) for k in ("X", "Vt", "Vd", "gt"))
        counts = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        ops.score_counts(Vt, Vd, gt, counts)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), cnt[r0:r0 + n]), b
        out.append(dict(X=X, Vt=Vt, Vd=Vd, gt=gt, counts=counts, X2=g[f"X2_{b}"], flipped=bool(g["flipped"][b])))
        r0 += n
    return g, sizes, mom, cnt, out


def test_k5_fixture_batches_through_the_report(dev, golden):
    """snr_moments on every fixture batch: the checks of K1, and metrics.snr_report of the device's rows against the reference"""
    from onet_amd import metrics
    g, sizes, mom, cnt, batches = golden
    rows = []
    for b, d in enumerate(batches):
        r, _ = _check_moments(dev, d["X"], d["Vt"], d["Vd"], d["gt"], f"K5 batch {b}")
        rows.append(r.cpu().numpy())
    rows = np.concatenate(rows)
    _assert_rows(rows, mom, "K5 against the host's NumPy rows")
    rep = metrics.snr_report(rows, cnt, sizes)
    got = np.array([[p[k] for k in vh.KEYS] for p in rep["per_batch"]])
    f64, f32, gap = g["psnr_fp64"], g["psnr_fp32"], float(g["ref_gap_db"])
    fin = np.isfinite(f64)
    print("K5 worst [dB] vs float64", np.abs(got[fin] - f64[fin]).max(), "vs the reference's fp32", np.abs(got[fin] - f32[fin]).max())
    assert [p["flipped"] for p in rep["per_batch"]] == [d["flipped"] for d in batches]
    assert np.array_equal(got[~fin], f64[~fin], equal_nan=True)
    assert np.all(np.abs(got[fin] - f64[fin]) <= DB_TOL) and np.all(np.abs(got[fin] - f32[fin]) <= 2 * gap + 1e-9)


def test_c1_cascade_input_on_the_fixture(dev, golden):
    """flip, keep, tie (and the two odd-sized batches): the bits of tensor_normal_per_frame of the selected map, with snr_moments'
    minmax and without; the reference's X2 at tests/test_gpu_model.py's bound for tensor_normal_per_frame"""
    from onet_amd import metrics, ops
    import onet_amd
    _, _, _, _, batches = golden
    assert [d["flipped"] for d in batches[:3]] == [True, False, False]
    for b, d in enumerate(batches):
        want = metrics.tensor_normal_per_frame(d["Vt"] if d["flipped"] else d["Vd"])
        other = metrics.tensor_normal_per_frame(d["Vd"] if d["flipped"] else d["Vt"])
        assert not torch.equal(want, other)
        minmax = ops.snr_moments(None, d["Vt"], d["Vd"], d["gt"], torch.empty((len(d["Vt"]), 9), dtype=torch.float64, device=dev))
        out = torch.full_like(want, 5.0)
        got = [ops.cascade_input(d["Vt"], d["Vd"], d["counts"], minmax=minmax), ops.cascade_input(d["Vt"], d["Vd"], d["counts"]),
               onet_amd.cascade_input(d["Vt"], d["Vd"], d["counts"]), ops.cascade_input(d["Vt"], d["Vd"], d["counts"], out=out)]
        assert got[3] is out
        for i, x2 in enumerate(got):
            assert x2.dtype == torch.float32 and x2.shape == want.shape and torch.equal(x2, want), (b, i)
            np.testing.assert_allclose(x2.cpu().numpy(), d["X2"], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("shape", [(2, 25, 41), (1, 4, 257), (1, 1, PARTS * CHUNK + 1), (300, 2, 6)], ids=lambda s: "x".join(map(str, s)))
def test_c2_cascade_input_at_the_path_edges(dev, shape):
    """more than one block per image, the grid's stride, more count rows than a block has threads; counts made by hand: one row
    decides, a tie, and sums that only the whole batch decides"""
    from onet_amd import metrics, ops
    B = shape[0]
    _, Vt, Vd, _ = (t.to(dev) for t in _maps(*shape, seed=5))
    nt, nd = metrics.tensor_normal_per_frame(Vt), metrics.tensor_normal_per_frame(Vd)
    minmax = torch.stack([Vt.reshape(B, -1).amin(1), Vt.reshape(B, -1).amax(1), Vd.reshape(B, -1).amin(1), Vd.reshape(B, -1).amax(1)], 1)
    right = torch.tensor([[3, 1, 1, 2]] * B, dtype=torch.int64)                  # TP + TN = 5 > 2
    tie = torch.tensor([[2, 1, 3, 2]] * B, dtype=torch.int64)                    # 4 == 4: kept
    wrong = right.clone()
    wrong[B - 1] = torch.tensor([0, 2 * B + 1, B, 0])                            # the LAST row turns the batch: 5 (B - 1) < 2 (B - 1) + 3 B + 1
    for counts, flip in ((right, False), (tie, False), (wrong, True)):
        tot = counts.sum(0)
        assert bool(tot[0] + tot[3] < tot[1] + tot[2]) == flip
        for mm in (minmax, None):
            got = ops.cascade_input(Vt, Vd, counts.to(dev), minmax=mm)
            assert torch.equal(got, nt if flip else nd), (shape, flip, mm is None)


# ----------------------------------------------------------------------------------------------------------------- model level
_M = {}


def _models(dev):
    """two small shared-weight Onets (1 channel), built once: the first stage's and the second stage's"""
    if not _M:
        import test_gpu_fused_head as fh
        from oracle import onet_oracle as orc
        _M["m1"] = fh._onet(fh._prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
        _M["m2"] = fh._onet(fh._prefixed(orc.det_state_dict(1, 1982)), 1, True, dev)
    return _M["m1"], _M["m2"]


def _batch(dev, B, H, W, seed, dtype=torch.uint8):
    from oracle import onet_oracle as orc
    g = np.random.Generator(np.random.PCG64([seed, B, H, W]))
    gt = torch.from_numpy((g.random((B, H, W)) > 0.7).astype(np.uint8)).to(dtype)
    return orc.det_input(B, 1, H, W, seed=seed).to(dev), gt.to(dev)


FUSED = "bf16+pool+anymap+pairs+up"


def _settings(which):
    from onet_amd import ops
    return ops.Settings() if which == "default" else ops.Settings(conv="bf16", fused_eval=FUSED)


def _check_verify_step(dev, m, X, gt, what):
    import onet_amd
    import test_gpu_fused_head as fh
    B = X.shape[0]
    onet_amd.validate(m, X, gt)                        # (the first call under these settings also packs the weights)
    val, k_val, o_val = fh._mfma_kinds(lambda: onet_amd.validate(m, X, gt, want_labels=True))
    ver, k_ver, o_ver = fh._mfma_kinds(lambda: onet_amd.verify_step(m, X, gt, want_labels=True))
    assert not {"onet_snr_moments", "onet_cascade_input"} & set(o_val), o_val
    assert k_ver == k_val, (what, k_ver, k_val)                                   # the same convolution launches: one forward
    assert o_ver == {**o_val, "onet_snr_moments": 1}, (what, o_ver, o_val)
    assert torch.equal(ver.counts, val.counts) and torch.equal(ver.labels, val.labels), what
    assert torch.equal(ver.Vt, val.Vt) and torch.equal(ver.Vd, val.Vd), what
    assert ver.moments.is_cuda and ver.moments.dtype == torch.float64 and tuple(ver.moments.shape) == (B, 9)
    _, want = _expected(X, ver.Vt, ver.Vd, gt)
    worst = _assert_rows(ver.moments.cpu().numpy(), want, what)
    plain = onet_amd.verify_step(m, X, gt)
    assert plain.labels is None and torch.equal(plain.counts, val.counts) and torch.equal(plain.moments, ver.moments), what
    # validate itself: the records it had before
    val2, k_val2, o_val2 = fh._mfma_kinds(lambda: onet_amd.validate(m, X, gt, want_labels=True))
    assert (k_val2, o_val2) == (k_val, o_val) and torch.equal(val2.counts, val.counts) and torch.equal(val2.labels, val.labels), what
    print(f"{what}: kinds {k_ver}, worst relative error of a sum {worst:.2e}")
    return k_ver


@pytest.mark.parametrize("which", ["default", "fused"])
@pytest.mark.parametrize("shape", [(2, 32, 32), (3, 24, 40)], ids=["2x32x32", "3x24x40"])
def test_m1_verify_step_is_validate_plus_the_moments(dev, shape, which):
    m, _ = _models(dev)
    m.settings = _settings(which)
    X, gt = _batch(dev, *shape, seed=41, dtype=torch.float32 if which == "default" else torch.uint8)
    _check_verify_step(dev, m, X, gt, f"M1 {shape} {which}")


def test_m2_verify_step_on_the_labels_only_plan(dev):
    """tests/test_gpu_fused_head.py's recipe A (2 x 1 x 128^2, shared weights) under Settings(conv="bf16", fused_eval="bf16"): the
    forward is the labels-only plan's (the head in the last convolution's epilogue), as validate's"""
    import test_gpu_fused_head as fh
    from onet_amd import ops
    r = fh._recipe(dev, "A")
    m, Xg = r["m"], r["Xg"]
    m.settings = ops.Settings(conv="bf16", fused_eval="bf16")
    _, gt = _batch(dev, 2, 128, 128, seed=43)
    kinds = _check_verify_step(dev, m, Xg, gt, "M2 recipe A")
    assert "conv3x3_pre16_head_kernel" in kinds, kinds


def test_m3_an_epoch_through_snr_report(dev):
    """EvalCounts + EvalSnr over three batches: the rows are the batches', snr_report on them is the per-batch recomputation from the
    returned Vt, Vd"""
    import onet_amd
    from onet_amd import metrics
    m, _ = _models(dev)
    m.settings = _settings("default")
    ec, es = onet_amd.EvalCounts(8, dev), onet_amd.EvalSnr(8, dev)
    want_rows, want_counts, per_batch = [], [], []
    for i, B in enumerate((2, 3, 2)):
        X, gt = _batch(dev, B, 24, 40, seed=50 + i)
        v = onet_amd.verify_step(m, X, gt, into=ec, snr=es)
        rows = _expected(X, v.Vt, v.Vd, gt)[1]
        counts = onet_amd.validate(m, X, gt).counts.cpu().numpy()
        assert torch.equal(v.counts.cpu(), torch.from_numpy(counts))
        want_rows.append(rows)
        want_counts.append(counts)
        per_batch.append(metrics.snr_report(rows, counts, [B])["per_batch"][0])
    assert ec.batch_sizes == es.batch_sizes == [2, 3, 2] and len(es) == 7
    with pytest.raises(ValueError):
        onet_amd.verify_step(m, *_batch(dev, 2, 24, 40, seed=60), into=ec, snr=es)
    assert ec.batch_sizes == es.batch_sizes == [2, 3, 2]
    rows, counts = es.rows().numpy(), ec.rows().numpy()
    assert np.array_equal(counts, np.concatenate(want_counts)) and not bool(es.moments[7:].any())
    _assert_rows(rows, np.concatenate(want_rows), "M3")
    rep = metrics.snr_report(rows, counts, es.batch_sizes)
    for got, want in zip(rep["per_batch"], per_batch):
        assert got["flipped"] == want["flipped"]
        for k in vh.KEYS:
            assert np.isfinite(want[k]) and abs(got[k] - want[k]) <= DB_TOL, (k, got, want)
    for k in vh.KEYS:
        assert abs(rep[k] - np.array([p[k] for p in per_batch]).mean()) <= DB_TOL
    print("M3 report", {k: rep[k] for k in vh.KEYS}, "flipped", [p["flipped"] for p in rep["per_batch"]])
    with pytest.raises(ValueError):
        onet_amd.verify_step(m, torch.zeros((2, 3, 24, 40), device=dev), _batch(dev, 2, 24, 40, seed=61)[1])


def test_m4_verify_cascade_is_the_manual_composition(dev):
    """validate -> cascade_input -> validate, each model under its own settings, bit for bit; the EvalCounts of both stages through
    metrics.cascade_metrics"""
    import onet_amd
    import test_gpu_fused_head as fh
    from onet_amd import metrics
    m1, m2 = _models(dev)
    m1.settings, m2.settings = _settings("default"), _settings("fused")
    ec1, ec2 = onet_amd.EvalCounts(5, dev), onet_amd.EvalCounts(5, dev)
    manual = []
    for i, B in enumerate((2, 3)):
        X, gt = _batch(dev, B, 24, 40, seed=70 + i)
        a1 = onet_amd.validate(m1, X, gt)
        X2 = onet_amd.cascade_input(a1.Vt, a1.Vd, a1.counts)
        tot = a1.counts.sum(0).tolist()
        flip = tot[0] + tot[3] < tot[1] + tot[2]
        assert torch.equal(X2, metrics.tensor_normal_per_frame(a1.Vt if flip else a1.Vd))
        a2 = onet_amd.validate(m2, X2, gt)
        (v1, v2), kinds, others = fh._mfma_kinds(lambda: onet_amd.verify_cascade(m1, m2, X, gt, into=ec1, into2=ec2))
        assert others.get("onet_cascade_input", 0) == 1 and others.get("onet_score_counts", 0) == 2 and "onet_snr_moments" not in others
        for got, want in ((v1, a1), (v2, a2)):
            assert torch.equal(got.counts, want.counts) and torch.equal(got.Vt, want.Vt) and torch.equal(got.Vd, want.Vd), i
        manual.append((a1.counts.cpu().numpy(), a2.counts.cpu().numpy()))
    rows1, rows2 = np.concatenate([a for a, _ in manual]), np.concatenate([b for _, b in manual])
    assert np.array_equal(ec1.rows().numpy(), rows1) and np.array_equal(ec2.rows().numpy(), rows2) and ec1.batch_sizes == ec2.batch_sizes == [2, 3]
    try:
        rep = metrics.cascade_metrics(ec1.rows(), ec2.rows(), ec1.batch_sizes)
    except AttributeError:              # (UT:149 on a batch whose prediction and ground truth are one class each: the reference's own)
        rep = None
    if rep is not None:
        assert rep["stage1"] == metrics.epoch_metrics(rows1, [2, 3], "simclutter") and rep["reference_return"][4] == rep["stage1"][4]
        print("M4", rep)
