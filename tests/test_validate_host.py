"""Host side of the on-device validation step (onet_amd.validate, onet_amd.EvalCounts, metrics.epoch_metrics): the two entry points of
include/onet_hip_eval.h -- declared, bound, exported, refusing bad arguments before a launch -- the pins the feature must not move
(the main header's prototypes, the ABI version), and the host arithmetic against the reference's recorded values: the
reference-signature helpers in count form against tests/golden/eval_side.npz, epoch_metrics against tests/golden/eval_batches.npz
(tests/golden/make_eval_batches.py: the bodies of the reference's two validation loops on three batches of label maps).

Tolerance of the metric checks: exact equality of the float64 values.  Both sides do the same float32 operations on the same integers
(counts below 2^24 are exact in float32; the reference's `a / (b + np.spacing(1))` is one float32 add and one float32 division, its
_miou one float32 division and one float32 add per class) and the same float64 means in numpy's order, so nothing is left to round
differently."""
import ctypes
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORE = ["Vt", "Vd", "gt", "gt_dtype", "gt_bs", "S", "Y", "counts", "B", "HW", "stream"]
LABEL = ["pred", "pred_dtype", "pred_bs", "gt", "gt_dtype", "gt_bs", "counts", "B", "HW", "stream"]


def test_eval_header_declares_exactly_the_two_entries():
    from onet_amd import _lib
    protos = _lib.parse_header(_lib.EVAL_HEADER)
    assert sorted(protos) == ["onet_label_counts", "onet_score_counts"]
    assert protos["onet_score_counts"][2] == SCORE and protos["onet_label_counts"][2] == LABEL
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert protos["onet_score_counts"][:2] == (I, [P, P, P, I, L, P, P, P, I, I, P])
    assert protos["onet_label_counts"][:2] == (I, [P, I, L, P, I, L, P, I, I, P])


def test_main_header_and_abi_version_unchanged():
    from onet_amd import _lib
    main = _lib.parse_header()
    assert len(main) == 108 and main == _lib.parse_header(_lib.HEADER)
    assert "onet_score_counts" not in main and "onet_label_counts" not in main
    assert len(main["onet_confusion2"][1]) == 6 and len(main["onet_softmax2_labels"][1]) == 7 and len(main["onet_argmax2"][1]) == 5
    assert _lib.load().onet_abi_version() == 4


def test_entries_exported_and_bound():
    from onet_amd import _lib, build
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIBPATH)
    for name, names in (("onet_score_counts", SCORE), ("onet_label_counts", LABEL)):
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(names), name
    # the new header is a dependency of the build
    lib_t = os.path.getmtime(build.LIB)
    hdr = _lib.EVAL_HEADER
    st = os.stat(hdr)
    try:
        os.utime(hdr, (lib_t + 10, lib_t + 10))
        assert build._stale()
    finally:
        os.utime(hdr, ns=(st.st_atime_ns, st.st_mtime_ns))


def test_load_reports_a_missing_export(monkeypatch, tmp_path):
    """_lib.load() is as loud about an export the new header declares and the library lacks as about the main header's"""
    from onet_amd import _lib
    _lib.load()
    hdr = tmp_path / "onet_hip_eval.h"
    hdr.write_text(open(_lib.EVAL_HEADER).read().replace("onet_label_counts", "onet_label_counts_missing"))
    monkeypatch.setattr(_lib, "EVAL_HEADER", str(hdr))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.OnetHipError, match="onet_label_counts_missing.*onet_hip_eval.h"):
        _lib.load(build_if_missing=False)


def test_score_counts_bad_arguments_are_refused_before_a_launch():
    from onet_amd import _lib
    lib = _lib.load()
    f, err = lib.onet_score_counts, lib.onet_last_error
    # (16: a non-null, 16-byte aligned address nothing may dereference)
    for missing in (0, 1, 2, 7):                               # Vt, Vd, gt, counts; S and Y may be null
        a = [16, 16, 16, 0, 64, None, None, 16, 1, 64, None]
        a[missing] = None
        assert f(*a) == -1 and b"null" in err(), missing
    assert f(16, 16, 16, 0, 64, 16, 16, 16, 0, 64, None) == -1 and b"bad shape" in err()
    assert f(16, 16, 16, 0, 64, 16, 16, 16, -3, 64, None) == -1 and b"bad shape" in err()
    assert f(16, 16, 16, 0, 64, 16, 16, 16, 1, 0, None) == -1 and b"bad shape" in err()
    for code in (4, -1, 99):
        assert f(16, 16, 16, code, 64, 16, 16, 16, 1, 64, None) == -1 and b"dtype" in err(), code
    assert f(16, 16, 16, 3, 63, 16, 16, 16, 2, 64, None) == -1 and b"stride" in err()
    assert f(16, 16, 16, 3, 0, 16, 16, 16, 1, 64, None) == -1 and b"stride" in err()


def test_label_counts_bad_arguments_are_refused_before_a_launch():
    from onet_amd import _lib
    lib = _lib.load()
    f, err = lib.onet_label_counts, lib.onet_last_error
    for missing in (0, 3, 6):                                  # pred, gt, counts
        a = [16, 2, 64, 16, 0, 64, 16, 1, 64, None]
        a[missing] = None
        assert f(*a) == -1 and b"null" in err(), missing
    assert f(16, 2, 64, 16, 0, 64, 16, 0, 64, None) == -1 and b"bad shape" in err()
    assert f(16, 2, 64, 16, 0, 64, 16, 1, -1, None) == -1 and b"bad shape" in err()
    assert f(16, 4, 64, 16, 0, 64, 16, 1, 64, None) == -1 and b"dtype" in err()
    assert f(16, 2, 64, 16, -1, 64, 16, 1, 64, None) == -1 and b"dtype" in err()
    assert f(16, 2, 63, 16, 0, 64, 16, 2, 64, None) == -1 and b"stride" in err()
    assert f(16, 2, 64, 16, 0, 10, 16, 2, 64, None) == -1 and b"stride" in err()


def test_python_surface():
    import inspect
    import torch
    import onet_amd
    from onet_amd import metrics, ops
    assert {"validate", "EvalCounts"} <= set(onet_amd.__all__)
    sig = inspect.signature(onet_amd.validate)
    assert list(sig.parameters) == ["onet", "X", "gt", "into", "want_labels", "want_S", "want_loss"]
    assert [sig.parameters[k].default for k in ("into", "want_labels", "want_S", "want_loss")] == [None, False, False, False]
    assert list(inspect.signature(ops.score_counts).parameters) == ["Vt", "Vd", "gt", "counts", "row", "want_S", "want_labels"]
    assert list(inspect.signature(ops.label_counts).parameters) == ["pred", "gt", "counts", "row"]
    for name, args in (("_acc", ["preds", "targets", "num_k"]), ("_miou", ["preds", "targets", "num_k"]),
                       ("_target_iou", ["preds", "targets"]), ("_detection_rate", ["preds", "targets"]),
                       ("_false_alarm_rate", ["preds", "targets"]), ("evaluate_nau_segmentation_v2", ["predict_label", "gt_label", "gt_k"]),
                       ("evaluate_segmentation", ["predict_label", "gt_label", "gt_k", "verbose"])):
        assert list(inspect.signature(getattr(metrics, name)).parameters) == args, name
    # the existing entry points of the module keep their signatures
    assert list(inspect.signature(metrics.evaluate).parameters) == ["onet", "X", "labels"]
    assert list(inspect.signature(onet_amd.segment).parameters) == ["onet", "X", "head"]
    assert list(inspect.signature(onet_amd.scores).parameters) == ["onet", "X"]
    ec = onet_amd.EvalCounts(5, torch.device("cpu"))
    assert ec.counts.dtype == torch.int64 and tuple(ec.counts.shape) == (5, 4) and not bool(ec.counts.any()) and ec.batch_sizes == []
    assert ec.reserve(2) == 0 and ec.reserve(3) == 2 and ec.batch_sizes == [2, 3] and tuple(ec.rows().shape) == (5, 4)
    with pytest.raises(ValueError):
        ec.reserve(1)
    ec.counts += 1
    ec.reset()
    assert ec.batch_sizes == [] and not bool(ec.counts.any()) and tuple(ec.rows().shape) == (0, 4)


def _counts(pred, gt):
    """(TP, FP, FN, TN) of one pair of label maps, by numpy"""
    p, t = pred.reshape(-1) != 0, gt.reshape(-1) != 0
    return np.array([(p & t).sum(), (p & ~t).sum(), (~p & t).sum(), (~p & ~t).sum()], dtype=np.int64)


def test_count_form_helpers_against_the_reference_fixture():
    """All nine cases of tests/golden/eval_side.npz (the reference's own _acc, _miou, _target_iou, _detection_rate,
    _false_alarm_rate): exact, including the empty-class rules and the case in which UT:149 raises."""
    from onet_amd import metrics as M
    g = np.load(os.path.join(G, "eval_side.npz"))
    names = [str(n) for n in g["names"]]
    assert len(names) == 9 and "disjoint" in names and "tie" in names
    for name in names:
        c = _counts(g[f"{name}_pred"], g[f"{name}_gt"])
        ref = g[f"{name}_metrics"]
        assert int(c.sum()) == g[f"{name}_pred"].size
        assert M._acc(c) == ref[0], name
        if np.isnan(ref[1]):
            assert name == "disjoint"
            with pytest.raises(AttributeError):
                M._miou(c)
            with pytest.raises(AttributeError):
                M.evaluate_nau_segmentation_v2(c)
        else:
            assert M._miou(c) == ref[1], (name, M._miou(c), ref[1])
            assert M.evaluate_nau_segmentation_v2(c) == (ref[0], ref[1], ref[3], ref[4], ref[2]), name
        assert M._target_iou(c) == ref[2] and M._detection_rate(c) == ref[3] and M._false_alarm_rate(c) == ref[4], name
        # [n, 4] rows are summed; a list is as good as an array
        assert M._acc(np.stack([c, c])) == ref[0] and M._acc([int(v) for v in c]) == ref[0], name
        # the hard re-assignment and the Hungarian relabelling, on the counts: against the reference's relabelled maps
        re = _counts(g[f"{name}_reassign"], g[f"{name}_gt"])
        mine = M.flipped(c) if M._acc(c) < M._acc(M.flipped(c)) else c
        assert np.array_equal(mine, re), name
        assert np.array_equal(M._matched(c), _counts(g[f"{name}_reorder"], g[f"{name}_gt"])), name


@pytest.fixture(scope="module")
def batches():
    g = np.load(os.path.join(G, "eval_batches.npz"))
    sizes = [int(n) for n in g["sizes"]]
    assert sizes == [4, 4, 2]
    rows = []
    for b, n in enumerate(sizes):
        p, t = g[f"pred{b}"], g[f"gt{b}"]
        assert p.dtype == np.uint8 and t.dtype == np.uint8 and p.shape == (n, 24, 40) and t.shape == p.shape
        rows += [_counts(p[i], t[i]) for i in range(n)]
    return g, sizes, np.stack(rows)


def test_fixture_has_a_flipped_a_kept_and_a_tied_batch(batches):
    from onet_amd import metrics as M
    g, sizes, rows = batches
    tot = [rows[0:4].sum(0), rows[4:8].sum(0), rows[8:10].sum(0)]
    flips = [M._acc(t) < M._acc(M.flipped(t)) for t in tot]
    assert flips == [True, False, False] and flips == [bool(v) for v in g["sim_flipped"]]
    assert M._acc(tot[2]) == M._acc(M.flipped(tot[2])) == 0.5               # the exact tie
    assert all(int(r.min()) > 0 for r in tot)


def test_epoch_metrics_simclutter_against_the_reference_loop(batches):
    from onet_amd import metrics as M
    g, sizes, rows = batches
    got = M.epoch_metrics(rows, sizes, "simclutter")
    assert isinstance(got, tuple) and len(got) == 5 and all(isinstance(v, float) for v in got)
    assert got == tuple(float(v) for v in g["sim_epoch"]), (got, g["sim_epoch"])
    r0 = 0
    for b, n in enumerate(sizes):                              # each batch alone: the loop body's five values
        assert M.epoch_metrics(rows[r0:r0 + n], [n], "simclutter") == tuple(float(v) for v in g["sim_batch"][b]), b
        r0 += n
    assert M.epoch_metrics([[int(v) for v in r] for r in rows], sizes, "simclutter") == got


def test_epoch_metrics_zy3_against_the_reference_loop(batches):
    from onet_amd import metrics as M
    g, sizes, rows = batches
    got = M.epoch_metrics(rows, sizes, "zy3")
    assert isinstance(got, tuple) and len(got) == 4
    assert got == tuple(float(v) for v in g["zy3_epoch"]), (got, g["zy3_epoch"])
    r0 = 0
    for b, n in enumerate(sizes):
        batch = rows[r0:r0 + n]
        # evaluate_segmentation on the relabelled batch, as UZ:174-181 calls it
        assert M.evaluate_segmentation(M._matched(batch.sum(0))) == tuple(float(v) for v in g["zy3_batch"][b]), b
        flip = not np.array_equal(M._matched(batch.sum(0)), batch.sum(0))
        per_image = [M.evaluate_nau_segmentation_v2(M.flipped(c) if flip else c)[:4] for c in batch]
        assert per_image == [tuple(float(v) for v in r) for r in g["zy3_images"][r0:r0 + n]], b
        r0 += n


def test_epoch_metrics_errors():
    from onet_amd import metrics as M
    with pytest.raises(ValueError):
        M.epoch_metrics(np.ones((3, 4), np.int64), [2, 2], "simclutter")
    with pytest.raises(ValueError):
        M.epoch_metrics(np.ones((3, 4), np.int64), [3], "nau")
    # UT:149: prediction all background, ground truth all foreground -- per batch (simclutter: the flip makes it perfect, so the batch
    # that raises is one the flip keeps: a tie cannot occur there; zy3 relabels first) and per image (zy3)
    disjoint, perfect = [0, 0, 960, 0], [960, 0, 0, 0]
    assert M.epoch_metrics([disjoint], [1], "simclutter")[0] == 1.0
    assert M.epoch_metrics([disjoint], [1], "zy3")[0] == 1.0
    with pytest.raises(AttributeError):
        # the batch total keeps its labels (3 images right, 1 disjoint), the disjoint image then has no mixed class
        M.epoch_metrics([[400, 0, 0, 560]] * 3 + [disjoint], [4], "zy3")
    assert M.epoch_metrics([perfect, [0, 0, 0, 960]], [1, 1], "zy3") == (1.0, 1.0, 0.5, 0.0)
