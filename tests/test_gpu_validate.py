"""The on-device validation step (onet_amd.validate, onet_amd.EvalCounts; include/onet_hip_eval.h).

Kernel level (K): ops.score_counts against the existing ops.softmax2_labels -- S and Y bit for bit -- and against integer counts formed
on the host from that Y and the ground truth; ops.label_counts against metrics.confusion_counts.  Everything is integers or a bit
pattern: every comparison is exact.  Shapes: one pixel, an odd map (scalar loads), less than one block's step, several blocks per
image, several images, and one batch large enough for a block to take more than one step.

Model level (M): validate against segment(head="fused") / the forward of the same model and settings, the launch records, the loss,
the fall-back, an EvalCounts through metrics.epoch_metrics, and the calls that existed before, unchanged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 7), (2, 16, 32), (1, 96, 160), (5, 64, 64)]
MAIN = (5, 64, 64)
DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float32]
SENTINEL = -7777
GONE = ("onet_softmax2_labels", "onet_argmax2", "onet_confusion2", "onet_flip_labels", "onet_head_softmax_fwd")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from onet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _scores(B, H, W, seed=0):
    """Vt, Vd [B, 1, H, W] on the host: ordinary values, and in a fixed pattern over the pixels exact ties, pairs one ulp apart (both
    ways), magnitudes of 1e4 with a gap of 1e-3 (both ways), +inf, -inf, both +inf (their difference is NaN) and NaN"""
    g = np.random.Generator(np.random.PCG64([seed, B, H, W]))
    vt = (g.standard_normal(B * H * W) * 3).astype(np.float32)
    vd = (g.standard_normal(B * H * W) * 3).astype(np.float32)
    k = (np.arange(B * H * W) + seed) % 13
    vd = np.where(k == 0, vt, vd)
    vd = np.where(k == 1, np.nextafter(vt, np.float32(np.inf)), vd)
    vd = np.where(k == 2, np.nextafter(vt, np.float32(-np.inf)), vd)
    vt = np.where(k == 3, np.float32(1e4), vt)
    vd = np.where(k == 3, np.float32(1e4) + np.float32(1e-3), vd)
    vt = np.where(k == 4, np.float32(1e4) + np.float32(1e-3), vt)
    vd = np.where(k == 4, np.float32(1e4), vd)
    vt = np.where(k == 5, np.float32(np.inf), vt)
    vd = np.where(k == 6, np.float32(-np.inf), vd)
    vt = np.where(k == 7, np.float32(np.inf), vt)
    vd = np.where(k == 7, np.float32(np.inf), vd)
    vt = np.where(k == 8, np.float32(np.nan), vt)
    vd = np.where(k == 9, np.float32(np.nan), vd)
    vt, vd = vt.astype(np.float32), vd.astype(np.float32)
    if B * H * W >= 13:
        assert (vt == vd).any() and np.isnan(vt).any() and np.isinf(vd).any()
        assert (np.float32(1e4) + np.float32(1e-3)) != np.float32(1e4)
    return torch.from_numpy(vt).view(B, 1, H, W), torch.from_numpy(vd).view(B, 1, H, W)


def _truth(B, H, W, seed=1):
    g = np.random.Generator(np.random.PCG64([seed, B, H, W]))
    return torch.from_numpy((g.random((B, H, W)) > 0.6).astype(np.uint8))


def _host_counts(Y, gt):
    """int64 [B, 4] = (TP, FP, FN, TN) per image from label maps on the host"""
    B = Y.shape[0]
    p, t = Y.reshape(B, -1).cpu() != 0, gt.reshape(B, -1).cpu() != 0
    return torch.stack([(p & t).sum(1), (p & ~t).sum(1), (~p & t).sum(1), (~p & ~t).sum(1)], dim=1).to(torch.int64)


_REF = {}


def _reference(dev, shape):
    """(Vt, Vd on the device, S0, Y0 of ops.softmax2_labels): computed once per shape, never modified"""
    if shape not in _REF:
        from onet_amd import ops
        Vt, Vd = (v.to(dev) for v in _scores(*shape))
        S0, Y0 = ops.softmax2_labels(Vt, Vd)
        torch.cuda.synchronize()
        _REF[shape] = (Vt, Vd, S0, Y0)
    return _REF[shape]


def _check_score_counts(dev, shape, gt, what):
    """score_counts on `gt` (a device label map in any layout) against the reference of `shape`"""
    from onet_amd import ops
    B, H, W = shape
    Vt, Vd, S0, Y0 = _reference(dev, shape)
    want = _host_counts(Y0, gt)
    if B * H * W >= 35:
        print(f"{what}: counts {want.sum(0).tolist()}")
        assert bool((want.sum(0) > 0).all()), (what, want)
    row = 2
    counts = torch.full((B + 3, 4), SENTINEL, dtype=torch.int64, device=dev)
    counts[row:row + B] = 5
    S, Y = ops.score_counts(Vt, Vd, gt, counts, row=row, want_S=True, want_labels=True)
    torch.cuda.synchronize()
    assert S.dtype == torch.float32 and tuple(S.shape) == (B, 2, H, W) and Y.dtype == torch.int64 and tuple(Y.shape) == (B, H, W)
    # bit for bit (NaN included): compare the patterns
    assert torch.equal(S.view(torch.int32), S0.view(torch.int32)), what
    assert torch.equal(Y, Y0), what
    got = counts.cpu()
    assert torch.equal(got[row:row + B], want + 5), (what, got, want)
    assert bool((got[:row] == SENTINEL).all()) and bool((got[row + B:] == SENTINEL).all()), (what, got)
    # counts alone (S and Y null): a second call into the same rows adds
    none = ops.score_counts(Vt, Vd, gt, counts, row=row)
    assert none == (None, None)
    assert torch.equal(counts.cpu()[row:row + B], 2 * want + 5), what
    assert bool((counts.cpu()[:row] == SENTINEL).all()) and bool((counts.cpu()[row + B:] == SENTINEL).all()), what
    # each output alone, into fresh rows: two runs give the same counts
    c1, c2 = (torch.zeros((B, 4), dtype=torch.int64, device=dev) for _ in range(2))
    S1, n1 = ops.score_counts(Vt, Vd, gt, c1, want_S=True)
    n2, Y2 = ops.score_counts(Vt, Vd, gt, c2, want_labels=True)
    assert n1 is None and n2 is None
    assert torch.equal(S1.view(torch.int32), S0.view(torch.int32)) and torch.equal(Y2, Y0), what
    assert torch.equal(c1, c2) and torch.equal(c1.cpu(), want), what
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_k1_score_counts_against_softmax2_labels(dev, shape, dtype):
    """K1: every shape x every ground-truth dtype, the map contiguous."""
    gt = _truth(*shape).to(dtype).to(dev)
    want = _check_score_counts(dev, shape, gt, f"K1 {shape} {dtype}")
    if shape == MAIN:
        assert bool((want > 0).all()), want                    # all four buckets of every image


def test_k1_bool_ground_truth(dev):
    gt = _truth(*MAIN).to(torch.bool).to(dev)
    _check_score_counts(dev, MAIN, gt, "K1 bool")


def test_k2_misaligned_uint8_ground_truth(dev):
    """K2: HW % 4 == 0 and a uint8 map that starts at byte 1 of its buffer: the scalar path on a shape the wide path would take."""
    shape = (2, 16, 32)
    B, H, W = shape
    buf = torch.zeros(B * H * W + 1, dtype=torch.uint8, device=dev)
    gt = buf[1:].view(B, H, W)
    gt.copy_(_truth(*shape))
    assert gt.data_ptr() % 4 == 1 and gt.is_contiguous()
    _check_score_counts(dev, shape, gt, "K2 misaligned")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.int64], ids=["uint8", "float32", "int64"])
def test_k2_batch_sliced_ground_truth(dev, dtype):
    """K2: the ground truth as a batch slice of a wider tensor (stride 2 HW), read where it lies; and one whose stride (HW + 2 elements)
    leaves the later images of a uint8 map unaligned for wide loads."""
    for shape in ((2, 16, 32), (3, 5, 7)):
        B, H, W = shape
        wide = torch.full((B, 2, H, W), 1 if dtype != torch.float32 else 1.0, dtype=dtype, device=dev)
        wide[:, 0] = 0
        gt = wide[:, 1]
        gt.copy_(_truth(*shape))
        assert gt.stride(0) == 2 * H * W and not gt.is_contiguous()
        _check_score_counts(dev, shape, gt, f"K2 sliced {shape} {dtype}")
        assert bool((wide[:, 0] == 0).all())
        odd = torch.zeros((B, H * W + 2), dtype=dtype, device=dev)
        gt = odd[:, :H * W].unflatten(1, (H, W))
        gt.copy_(_truth(*shape))
        assert gt.stride(0) == H * W + 2
        _check_score_counts(dev, shape, gt, f"K2 odd stride {shape} {dtype}")


def test_k3_a_block_takes_more_than_one_step(dev):
    """K3: 8 images of 520 x 512: 260 steps of 1024 pixels per image for at most max(CUs, 8 CUs / 8) blocks (256 on an MI355X), so some
    blocks loop.  Labels and counts only."""
    from onet_amd import ops
    shape = (8, 520, 512)
    B, H, W = shape
    Vt, Vd = (v.to(dev) for v in _scores(*shape))
    gt = _truth(*shape).to(dev)
    _, Y0 = ops.softmax2_labels(Vt, Vd, want_S=False)
    counts = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    _, Y = ops.score_counts(Vt, Vd, gt, counts, want_labels=True)
    torch.cuda.synchronize()
    assert torch.equal(Y, Y0)
    want = _host_counts(Y0, gt)
    assert torch.equal(counts.cpu(), want) and bool((want > 0).all()) and int(want.sum()) == B * H * W


def test_k4_wrapper_refuses(dev):
    from onet_amd import ops
    B, H, W = 2, 4, 8
    Vt, Vd = (v.to(dev) for v in _scores(B, H, W))
    gt = _truth(B, H, W).to(dev)
    counts = torch.zeros((3, 4), dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.score_counts(Vt, Vd, gt, counts, row=2)                        # rows [2, 4) of 3
    with pytest.raises(ValueError):
        ops.score_counts(Vt, Vd, gt[:1], counts)
    with pytest.raises(ValueError):
        ops.score_counts(Vt, Vd, gt, counts.to(torch.int32))
    with pytest.raises(TypeError):
        ops.score_counts(Vt, Vd, gt.to(torch.int16), counts)
    with pytest.raises(ValueError):
        ops.label_counts(gt, gt[:, :2], counts)
    torch.cuda.synchronize()
    assert not bool(counts.any())


@pytest.mark.parametrize("gdtype", DTYPES, ids=lambda d: "gt-" + str(d).split(".")[-1])
@pytest.mark.parametrize("pdtype", DTYPES, ids=lambda d: "pred-" + str(d).split(".")[-1])
def test_k5_label_counts_against_confusion_counts(dev, pdtype, gdtype):
    """K5: label_counts, every prediction dtype x every ground-truth dtype, against the existing metrics.confusion_counts."""
    from onet_amd import metrics, ops
    for shape in ((3, 5, 7), (2, 16, 32)):
        B, H, W = shape
        pred, gt = _truth(*shape, seed=7).to(pdtype).to(dev), _truth(*shape).to(gdtype).to(dev)
        want = metrics.confusion_counts(pred, gt).cpu()
        assert torch.equal(want, _host_counts(pred, gt)) and bool((want.sum(0) > 0).all()), (shape, want)
        row = 1
        counts = torch.full((B + 2, 4), SENTINEL, dtype=torch.int64, device=dev)
        counts[row:row + B] = 0
        assert ops.label_counts(pred, gt, counts, row=row) is counts
        got = counts.cpu()
        assert torch.equal(got[row:row + B], want), (shape, got, want)
        assert bool((got[:row] == SENTINEL).all()) and bool((got[row + B:] == SENTINEL).all()), (shape, got)
        ops.label_counts(pred, gt, counts, row=row)
        assert torch.equal(counts.cpu()[row:row + B], 2 * want), shape
        c1, c2 = (torch.zeros((B, 4), dtype=torch.int64, device=dev) for _ in range(2))
        ops.label_counts(pred, gt, c1)
        ops.label_counts(pred, gt, c2)
        assert torch.equal(c1, c2) and torch.equal(c1.cpu(), want), shape
        # the reference-signature helpers count with it: one image of the whole batch
        tot = [int(v) for v in want.sum(0)]
        assert metrics._acc(pred, gt, 2) == metrics._acc(tot) and metrics._miou(pred, gt, 2) == metrics._miou(tot)
        assert metrics._target_iou(pred, gt) == metrics._target_iou(tot) and metrics._detection_rate(pred, gt) == metrics._detection_rate(tot)
        assert metrics._false_alarm_rate(pred, gt) == metrics._false_alarm_rate(tot)
        assert metrics.evaluate_nau_segmentation_v2(pred, gt) == metrics.evaluate_nau_segmentation_v2(tot)
        assert metrics.evaluate_segmentation(pred, gt, gt_k=2) == metrics.evaluate_segmentation(tot)


def test_k5_label_counts_misaligned_and_sliced(dev):
    from onet_amd import ops
    shape = (2, 16, 32)
    B, H, W = shape
    buf = torch.zeros(B * H * W + 1, dtype=torch.uint8, device=dev)
    pred = buf[1:].view(B, H, W)
    pred.copy_(_truth(*shape, seed=7))
    wide = torch.zeros((B, 3, H, W), dtype=torch.float32, device=dev)
    gt = wide[:, 2]
    gt.copy_(_truth(*shape))
    counts = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    ops.label_counts(pred, gt, counts)
    assert torch.equal(counts.cpu(), _host_counts(pred, gt))


# ----------------------------------------------------------------------------------------------------------------- model level
def _snapshot(fh, m, Xg):
    """The calls that existed before, with their launch records"""
    import onet_amd
    out, k_fwd, o_fwd = fh._mfma_kinds(lambda: m(Xg))
    sc, k_sc, o_sc = fh._mfma_kinds(lambda: onet_amd.scores(m, Xg))
    lab, k_lab, o_lab = fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused"))
    return (tuple(out) + tuple(sc) + (lab,)), (k_fwd, o_fwd, k_sc, o_sc, k_lab, o_lab)


def _assert_same(a, b):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), f"tensor {i} of the earlier calls changed"
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert x == y, (f"launch record {i} of the earlier calls changed", x, y)


def _model_truth(B, H, W, dev, dtype=torch.uint8):
    return _truth(B, H, W, seed=3).to(dtype).to(dev)


def test_m1_validate_on_the_labels_only_plan(dev):
    """M1: tests/test_gpu_fused_head.py's recipe A (2 x 1 x 128^2, shared weights) under Settings(conv="bf16", fused_eval="bf16"):
    labels bit-equal to segment(head="fused"), counts exact, the MFMA launches those of segment(head="fused"), exactly one
    onet_score_counts and none of softmax2_labels / argmax2 / confusion2 / flip_labels / head_softmax_fwd; the loss bit-equal to
    compute_loss on the forward's Lt, Ld and scores' S; the forward, scores and segment before and after, bit for bit, with the launches
    they made before."""
    import onet_amd
    import test_gpu_fused_head as fh
    from onet_amd import ops
    r = fh._recipe(dev, "A")
    m, Xg, B = r["m"], r["Xg"], r["B"]
    m.settings = ops.Settings(conv="bf16", fused_eval="bf16")
    gt = _model_truth(B, 128, 128, dev)
    _snapshot(fh, m, Xg)            # (the first calls under these settings also pack the weights: not part of the record)
    before = _snapshot(fh, m, Xg)
    out, (k_fwd, o_fwd, k_sc, o_sc, k_lab, o_lab) = before
    Lt, Ld, S, lab = out[0], out[2], out[7], out[8]
    assert "conv3x3_pre16_head_kernel" in k_lab and o_lab.get("onet_softmax2_labels", 0) == 1 and "onet_score_counts" not in o_lab

    v, k_val, o_val = fh._mfma_kinds(lambda: onet_amd.validate(m, Xg, gt, want_labels=True))
    assert k_val == k_lab, (k_val, k_lab)
    assert o_val.get("onet_score_counts", 0) == 1 and not set(GONE) & set(o_val), o_val
    assert {k: n for k, n in o_val.items() if k != "onet_score_counts"} == {k: n for k, n in o_lab.items() if k != "onet_softmax2_labels"}
    assert v.labels.dtype == torch.int64 and torch.equal(v.labels, lab)
    want = _host_counts(lab, gt)
    print("M1 counts", want.tolist())
    assert v.counts.is_cuda and v.counts.dtype == torch.int64 and tuple(v.counts.shape) == (B, 4) and torch.equal(v.counts.cpu(), want)
    assert int(want.sum()) == B * 128 * 128
    assert v.S is None and v.loss is None and torch.equal(v.Vt, out[5]) and torch.equal(v.Vd, out[6])
    # counts alone: no labels stored, the same integers
    v0 = onet_amd.validate(m, Xg, gt)
    assert v0.labels is None and v0.S is None and torch.equal(v0.counts.cpu(), want)

    # the loss: compute_loss on the forward's L (bit-equal activations on the one-part plan) and scores' S
    ref = m.compute_loss(Lt, S[:, :1], Ld, S[:, 1:])
    vl, k_l, o_l = fh._mfma_kinds(lambda: onet_amd.validate(m, Xg, gt, want_loss=True, want_S=True, want_labels=True))
    assert vl.loss.is_cuda and tuple(vl.loss.shape) == (1,) and vl.loss.dtype == torch.float32
    print("M1 loss", float(vl.loss), float(ref))
    assert torch.equal(vl.loss, ref.reshape(1)), (float(vl.loss), float(ref))
    assert torch.equal(vl.S, S) and torch.equal(vl.labels, lab) and torch.equal(vl.counts.cpu(), want)
    assert k_l == k_lab and o_l.get("onet_score_counts", 0) == 1 and not set(GONE) & set(o_l) and o_l.get("onet_jsd_fwd", 0) == 2, (k_l, o_l)

    _assert_same(_snapshot(fh, m, Xg), before)


def test_m2_fall_back_is_the_forward(dev):
    """M2: Settings() on 2 x 1 x 40 x 40 (no fused plan): labels equal predict_label of the forward's S, counts exact, one
    onet_score_counts beside the forward's own launches; the loss is compute_loss's on the forward's tensors."""
    import onet_amd
    import test_gpu_fused_head as fh
    from onet_amd import ops
    from oracle import onet_oracle as orc
    m = fh._onet(fh._prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    m.settings = ops.Settings()
    X = orc.det_input(2, 1, 40, 40, seed=113).to(dev)
    gt = _model_truth(2, 40, 40, dev, torch.float32)
    with torch.no_grad():
        m(X)                        # (packs the weights)
    out, k_fwd, o_fwd = fh._mfma_kinds(lambda: m(X))
    lab = m.predict_label(out[4])
    v, k_val, o_val = fh._mfma_kinds(lambda: onet_amd.validate(m, X, gt, want_labels=True, want_S=True, want_loss=True))
    assert torch.equal(v.labels, lab) and torch.equal(v.counts.cpu(), _host_counts(lab, gt))
    assert torch.equal(v.S, out[4]) and torch.equal(v.Vt, out[1]) and torch.equal(v.Vd, out[3])
    assert k_val == k_fwd and o_val.get("onet_score_counts", 0) == 1, (k_val, o_val)
    assert not {"onet_softmax2_labels", "onet_argmax2", "onet_confusion2", "onet_flip_labels"} & set(o_val), o_val
    with torch.no_grad():
        o2 = m(X)
        ref = m.compute_loss(o2[0], o2[4][:, :1], o2[2], o2[4][:, 1:])
    assert torch.equal(v.loss, ref.reshape(1)), (float(v.loss), float(ref))
    out2, k2, o2r = fh._mfma_kinds(lambda: m(X))
    assert all(torch.equal(a, b) for a, b in zip(out, out2)) and (k2, o2r) == (k_fwd, o_fwd)


@pytest.mark.parametrize("protocol", ["simclutter", "zy3"])
def test_m3_eval_counts_through_epoch_metrics(dev, protocol):
    """M3: an EvalCounts fed a batch of 2 then a batch of 1 (float32 ground truth, the reference's dtype): its rows are the integer
    counts of the labels, and epoch_metrics on them is the protocol computed on the host from the labels."""
    import onet_amd
    import test_gpu_fused_head as fh
    from onet_amd import metrics, ops
    r = fh._recipe(dev, "A")
    m, Xg = r["m"], r["Xg"]
    m.settings = ops.Settings(conv="bf16", fused_eval="bf16")
    gt = _model_truth(2, 128, 128, dev, torch.float32)
    ec = onet_amd.EvalCounts(4, dev)
    a = onet_amd.validate(m, Xg, gt, into=ec, want_labels=True)
    b = onet_amd.validate(m, Xg[1:], gt[1:], into=ec, want_labels=True)
    assert ec.batch_sizes == [2, 1] and len(ec) == 3
    assert a.counts.data_ptr() == ec.counts.data_ptr() and b.counts.data_ptr() == ec.counts[2:].data_ptr()
    rows = ec.rows()
    assert not rows.is_cuda and tuple(rows.shape) == (3, 4)
    host = torch.cat([_host_counts(a.labels, gt), _host_counts(b.labels, gt[1:])])
    assert torch.equal(rows, host), (rows, host)
    assert not bool(ec.counts[3:].any())
    assert metrics.epoch_metrics(rows, ec.batch_sizes, protocol) == metrics.epoch_metrics(host.numpy(), [2, 1], protocol)
    # the protocol step by step on the label maps, with the helpers that existed before
    vals = []
    for lab, g in ((a.labels, gt), (b.labels, gt[1:])):
        if protocol == "simclutter":
            c = metrics.confusion_counts(metrics.re_assign_label(lab, g), g)
            vals.append((metrics._acc(c), metrics._miou(c), metrics._detection_rate(c), metrics._false_alarm_rate(c), metrics._target_iou(c)))
        else:
            Y = metrics.reorder_segmentation(lab, g)
            for i in range(lab.shape[0]):
                c = metrics.confusion_counts(Y[i:i + 1], g[i:i + 1])
                vals.append((metrics._acc(c), metrics._miou(c), metrics._detection_rate(c), metrics._false_alarm_rate(c)))
    want = tuple(float(np.array([v[k] for v in vals]).mean()) for k in range(len(vals[0])))
    got = metrics.epoch_metrics(rows, ec.batch_sizes, protocol)
    print(f"M3 {protocol}: {got}")
    assert got == want, (got, want)
    ec.reset()
    assert ec.batch_sizes == [] and not bool(ec.counts.any())
