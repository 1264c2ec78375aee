"""Host side of the SNR-gain report and the two-stage cascade (onet_amd.verify_step / EvalSnr / cascade_input / verify_cascade,
metrics.snr_report / cascade_metrics; include/onet_hip_verify.h): the two entry points -- declared, bound, exported, refusing bad
arguments before a launch -- the pins the feature must not move (every other header's prototypes, the ABI version), and the host
arithmetic against tests/golden/verify_batches.npz (tests/golden/make_verify_batches.py: the bodies of the reference's
measure_snr_on_fg and test_2nd_stage_simclutter on five batches, with the reference's own functions).

Tolerances.  The per-image moments are formed here by NumPy in float64 from the fixture's fp32 tensors (the squares in float64, as the
kernel forms them), so snr_report differs from the reference's get_psnr evaluated in float64 on the same inputs only by the order of
float64 additions and one log10: 1e-12 relative.  The reference itself sums in fp32; the fixture records the gap between its fp32
results and its float64 ones (ref_gap_db), which IS the expected difference: 2 * ref_gap_db + 1e-9 dB, the factor 2 for the reference's
summation order on another torch build.  The cascade's metrics: exact equality, as tests/test_validate_host.py compares
epoch_metrics."""
import ctypes
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MOMENTS = ["X", "x_bs", "Vt", "Vd", "gt", "gt_dtype", "gt_bs", "moments", "minmax", "B", "HW", "ws", "ws_bytes", "stream"]
CASCADE = ["Vt", "Vd", "minmax", "counts", "X2", "B", "HW", "stream"]
OTHERS = {"EVAL_HEADER": 2, "RAGGED_HEADER": 5, "RAGGED_SPLIT_HEADER": 5, "ANYMAP_HEADER": 2, "PAIRS_HEADER": 1, "UPMAP_HEADER": 1,
          "SPLIT_PAIRS_HEADER": 1, "OPTIM_HEADER": 1}
KEYS = ("input_psnr", "input_snr", "fg_psnr", "fg_snr")


def test_verify_header_declares_exactly_the_two_entries():
    from onet_amd import _lib
    protos = _lib.parse_header(_lib.VERIFY_HEADER)
    assert sorted(protos) == ["onet_cascade_input", "onet_snr_moments"]
    assert protos["onet_snr_moments"][2] == MOMENTS and protos["onet_cascade_input"][2] == CASCADE
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert protos["onet_snr_moments"][:2] == (I, [P, L, P, P, P, I, L, P, P, I, I, P, L, P])
    assert protos["onet_cascade_input"][:2] == (I, [P, P, P, P, P, I, I, P])


def test_every_other_header_and_the_abi_version_unchanged():
    from onet_amd import _lib
    main = _lib.parse_header()
    assert len(main) == 108 and not {"onet_snr_moments", "onet_cascade_input"} & set(main)
    seen = set(main)
    for name, n in OTHERS.items():
        protos = _lib.parse_header(getattr(_lib, name))
        assert len(protos) == n and not seen & set(protos), name
        assert not {"onet_snr_moments", "onet_cascade_input"} & set(protos), name
        seen |= set(protos)
    assert sorted(_lib.parse_header(_lib.EVAL_HEADER)) == ["onet_label_counts", "onet_score_counts"]
    assert len(main["onet_normalise_per_frame"][1]) == 5
    assert _lib.load().onet_abi_version() == 4


def test_entries_exported_and_bound():
    from onet_amd import _lib, build
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIBPATH)
    for name, names in (("onet_snr_moments", MOMENTS), ("onet_cascade_input", CASCADE)):
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(names), name
    lib_t = os.path.getmtime(build.LIB)                   # the new header is a dependency of the build
    st = os.stat(_lib.VERIFY_HEADER)
    try:
        os.utime(_lib.VERIFY_HEADER, (lib_t + 10, lib_t + 10))
        assert build._stale()
    finally:
        os.utime(_lib.VERIFY_HEADER, ns=(st.st_atime_ns, st.st_mtime_ns))


def test_bad_arguments_are_refused_before_a_launch():
    from onet_amd import _lib
    lib = _lib.load()
    f, err = lib.onet_snr_moments, lib.onet_last_error
    ok = [16, 64, 16, 16, 16, 0, 64, 16, 16, 1, 64, 16, 64 * 88, None]     # (16: an aligned address nothing may dereference)
    for missing in (2, 3, 4, 7, 8, 11):                     # Vt, Vd, gt, moments, minmax, ws; X may be null
        a = list(ok)
        a[missing] = None
        assert f(*a) == -1 and b"null" in err(), missing

    def with_(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[MOMENTS.index(k)] = v
        return a
    for bad in (dict(B=0), dict(B=65536), dict(HW=0)):
        assert f(*with_(**bad)) == -1 and b"bad shape" in err(), bad
    for code in (4, -1):
        assert f(*with_(gt_dtype=code)) == -1 and b"dtype" in err(), code
    assert f(*with_(gt_bs=63)) == -1 and b"stride" in err()
    assert f(*with_(x_bs=63)) == -1 and b"stride" in err()
    assert f(*with_(ws_bytes=64 * 88 - 1)) == -1 and b"workspace" in err()
    assert f(*with_(B=2)) == -1 and b"workspace" in err()                  # (the need grows with the batch)
    assert f(*with_(ws=20)) == -1 and b"workspace" in err()                # (not 8-byte aligned)
    g = lib.onet_cascade_input
    for missing in (0, 1, 3, 4):                            # Vt, Vd, counts, X2; minmax may be null
        a = [16, 16, 16, 16, 16, 1, 64, None]
        a[missing] = None
        assert g(*a) == -1 and b"null" in err(), missing
    assert g(16, 16, None, 16, 16, 0, 64, None) == -1 and b"bad shape" in err()
    assert g(16, 16, None, 16, 16, 65536, 64, None) == -1 and b"bad shape" in err()
    assert g(16, 16, None, 16, 16, 1, 0, None) == -1 and b"bad shape" in err()


def test_python_surface():
    import inspect
    import onet_amd
    from onet_amd import inference, metrics, ops
    assert {"EvalSnr", "verify_step", "cascade_input", "verify_cascade"} <= set(onet_amd.__all__)
    assert list(inspect.signature(ops.snr_moments).parameters) == ["X", "Vt", "Vd", "gt", "moments", "row", "minmax"]
    assert list(inspect.signature(ops.cascade_input).parameters) == ["Vt", "Vd", "counts", "minmax", "out"]
    sig = inspect.signature(onet_amd.verify_step)
    assert list(sig.parameters) == ["onet", "X", "gt", "into", "snr", "want_labels"]
    assert [sig.parameters[k].default for k in ("into", "snr", "want_labels")] == [None, None, False]
    assert list(inspect.signature(onet_amd.cascade_input).parameters) == ["Vt", "Vd", "counts"]
    assert list(inspect.signature(onet_amd.verify_cascade).parameters) == ["onet", "onet2nd", "X", "gt", "into", "into2"]
    assert inference.Verification._fields == ("counts", "moments", "labels", "Vt", "Vd")
    assert list(inspect.signature(metrics.snr_report).parameters) == ["moment_rows", "count_rows", "batch_sizes"]
    assert list(inspect.signature(metrics.cascade_metrics).parameters) == ["rows1", "rows2", "batch_sizes"]
    # the surfaces the feature must not widen
    assert list(inspect.signature(onet_amd.validate).parameters) == ["onet", "X", "gt", "into", "want_labels", "want_S", "want_loss"]


def test_eval_snr_bookkeeping_and_value_errors():
    import torch
    import onet_amd
    cpu = torch.device("cpu")
    es = onet_amd.EvalSnr(5, cpu)
    assert es.moments.dtype == torch.float64 and tuple(es.moments.shape) == (5, 9) and not bool(es.moments.any()) and es.batch_sizes == []
    assert es.reserve(2) == 0 and es.reserve(3) == 2 and es.batch_sizes == [2, 3] and len(es) == 5 and tuple(es.rows().shape) == (5, 9)
    with pytest.raises(ValueError):
        es.reserve(1)
    es.moments += 1
    es.reset()
    assert es.batch_sizes == [] and len(es) == 0 and not bool(es.moments.any()) and tuple(es.rows().shape) == (0, 9)
    # verify_step refuses before it runs anything: an input that is not [B, 1, H, W]; an EvalCounts and an EvalSnr at different rows
    gt = torch.zeros((2, 8, 8), dtype=torch.uint8)
    for shape in ((2, 3, 8, 8), (2, 8, 8), (2, 2, 8, 8)):
        with pytest.raises(ValueError, match="one-channel"):
            onet_amd.verify_step(None, torch.zeros(shape), gt)
    ec = onet_amd.EvalCounts(5, cpu)
    ec.reserve(2)
    with pytest.raises(ValueError, match="row 2.*row 0"):
        onet_amd.verify_step(None, torch.zeros((2, 1, 8, 8)), gt, into=ec, snr=es)
    assert ec.batch_sizes == [2] and es.batch_sizes == []
    es.reserve(2)
    with pytest.raises(ValueError, match="cannot take 4 more"):         # (nor are the EvalCounts' rows taken)
        onet_amd.verify_step(None, torch.zeros((4, 1, 8, 8)), torch.zeros((4, 8, 8)), into=ec, snr=es)
    assert ec.batch_sizes == [2] and es.batch_sizes == [2]
    from onet_amd import metrics as M
    with pytest.raises(ValueError):
        M.snr_report(np.zeros((3, 9)), np.ones((3, 4), np.int64), [2, 2])
    with pytest.raises(ValueError):
        M.snr_report(np.zeros((4, 9)), np.ones((3, 4), np.int64), [2, 2])
    with pytest.raises(ValueError):
        M.cascade_metrics(np.ones((3, 4), np.int64), np.ones((3, 4), np.int64), [2, 2])


# ---------------------------------------------------------------------------------------------------------------- the fixture
def normal_per_frame(V):
    """tensor_normal_per_frame (UT:673-689) by NumPy, every step in fp32: [n, 1, H, W] -> the same shape"""
    v = V.reshape(V.shape[0], -1).astype(np.float32)
    lo, hi = v.min(axis=1, keepdims=True), v.max(axis=1, keepdims=True)
    return ((v - lo) / ((hi - lo) + np.float32(np.spacing(1)))).astype(np.float32).reshape(V.shape)


def moment_rows(X, nt, nd, gt):
    """ops.snr_moments' rows by NumPy in float64 from fp32 maps [n, ...] (X may be None): [n, 9]"""
    n = gt.shape[0]
    t = gt.reshape(n, -1) != 0
    rows = np.zeros((n, 9), dtype=np.float64)
    for s, v in enumerate((X, nt, nd)):
        if v is None:
            continue
        v = v.reshape(n, -1)
        assert v.dtype == np.float32
        sq = v.astype(np.float64) ** 2
        rows[:, 3 * s] = np.where(t, sq, 0.0).sum(axis=1)
        rows[:, 3 * s + 1] = np.where(t, 0.0, sq).sum(axis=1)
        rows[:, 3 * s + 2] = np.where(t, v, np.float32(0)).max(axis=1).clip(min=0)
    return rows


def count_rows(Vt, Vd, gt):
    """(TP, FP, FN, TN) per image of the head's labels (Vd > Vt) against gt: [n, 4]"""
    n = gt.shape[0]
    p, t = (Vd > Vt).reshape(n, -1), gt.reshape(n, -1) != 0
    return np.stack([(p & t).sum(1), (p & ~t).sum(1), (~p & t).sum(1), (~p & ~t).sum(1)], axis=1).astype(np.int64)


def load_fixture():
    g = np.load(os.path.join(G, "verify_batches.npz"))
    sizes = [int(n) for n in g["sizes"]]
    mom, cnt, cnt2 = [], [], []
    for b, n in enumerate(sizes):
        X, Vt, Vd, gt = (g[f"{k}{b}"] for k in ("X", "Vt", "Vd", "gt"))
        assert X.dtype == np.float32 and X.shape == Vt.shape == Vd.shape and X.shape[:2] == (n, 1) and gt.shape == (n,) + X.shape[2:]
        mom.append(moment_rows(X, normal_per_frame(Vt), normal_per_frame(Vd), gt))
        cnt.append(count_rows(Vt, Vd, gt))
        cnt2.append(count_rows(g[f"Vt2{b}"], g[f"Vd2{b}"], gt))
    return g, sizes, np.concatenate(mom), np.concatenate(cnt), np.concatenate(cnt2)


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def test_fixture_covers_the_cases(fixture):
    g, sizes, mom, cnt, cnt2 = fixture
    assert os.path.getsize(os.path.join(G, "verify_batches.npz")) < 200 * 1024
    assert sizes == [3, 3, 2, 2, 3]
    assert [g[f"X{b}"].shape[2:] for b in range(5)] == [(24, 40)] * 3 + [(25, 37)] * 2 and (25 * 37) % 4 != 0
    assert [g[f"gt{b}"].dtype for b in range(5)] == [np.float32, np.uint8, np.float32, np.uint8, np.float32]
    tot = [cnt[r0:r0 + n].sum(0) for r0, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
    assert [bool(t[0] + t[3] < t[1] + t[2]) for t in tot] == [True, False, False, False, True]
    assert tot[2][0] + tot[2][3] == tot[2][1] + tot[2][2]                           # the exact tie
    assert not g["gt1"][1].any() and g["gt1"][0].any() and not g["gt3"].any()      # an image, a whole batch without a positive pixel
    assert g["Vd1"][2].min() == g["Vd1"][2].max()                                   # a constant frame
    assert g["Vt4"].max() < 0 and g["Vd4"].max() < 0 and g["Vt0"].min() < 0 < g["Vt0"].max()
    assert 0 < float(g["ref_gap_db"]) < 1e-4


def test_snr_report_against_the_reference(fixture):
    from onet_amd import metrics as M
    g, sizes, mom, cnt, _ = fixture
    rep = M.snr_report(mom, cnt, sizes)
    assert sorted(rep) == sorted(KEYS + ("per_batch",)) and len(rep["per_batch"]) == 5
    assert [b["flipped"] for b in rep["per_batch"]] == [bool(v) for v in g["flipped"]]
    got = np.array([[b[k] for k in KEYS] for b in rep["per_batch"]], dtype=np.float64)
    f64, f32, gap = g["psnr_fp64"], g["psnr_fp32"], float(g["ref_gap_db"])
    fin = np.isfinite(f64)
    print("snr_report per batch", got.tolist(), "worst vs float64", np.abs(got[fin] / f64[fin] - 1).max(), "worst vs fp32 [dB]",
          np.abs(got[fin] - f32[fin]).max(), "bound", 2 * gap + 1e-9)
    assert fin.sum() == 16 and np.array_equal(fin, np.isfinite(got))
    assert np.all(np.abs(got[fin] - f64[fin]) <= 1e-12 * np.abs(f64[fin]))
    assert np.all(np.abs(got[fin] - f32[fin]) <= 2 * gap + 1e-9)
    # a batch without target pixels: what the reference gives (-inf, nan), and the epoch means that follow from it
    assert np.array_equal(got[~fin], f64[~fin], equal_nan=True) and np.array_equal(got[~fin], f32[~fin], equal_nan=True)
    assert np.array_equal(got[3], [-np.inf, np.nan, -np.inf, np.nan], equal_nan=True)
    epoch = np.array([rep[k] for k in KEYS])
    assert np.array_equal(epoch, g["epoch_fp64"], equal_nan=True) and np.array_equal(epoch, g["epoch_fp32"], equal_nan=True)
    # the epoch of the four batches with targets: TS:91-94's means
    keep = np.r_[0:8, 10:13]
    rep4 = M.snr_report(mom[keep], cnt[keep], [3, 3, 2, 3])
    epoch4 = np.array([rep4[k] for k in KEYS])
    assert np.all(np.abs(epoch4 - g["epoch_fp64_targets"]) <= 1e-12 * np.abs(g["epoch_fp64_targets"]))
    assert np.all(np.abs(epoch4 - g["epoch_fp32_targets"]) <= 2 * gap + 1e-9)
    # lists are as good as arrays; X left out (zeros): the input values are nan, the foreground's unchanged
    assert M.snr_report(mom[keep].tolist(), cnt[keep].tolist(), [3, 3, 2, 3])["per_batch"] == rep4["per_batch"]
    nox = mom.copy()
    nox[:, :3] = 0
    r0 = M.snr_report(nox[:3], cnt[:3], [3])["per_batch"][0]
    assert np.isnan(r0["input_snr"]) and r0["fg_psnr"] == rep["per_batch"][0]["fg_psnr"] and r0["fg_snr"] == rep["per_batch"][0]["fg_snr"]


def test_cascade_metrics_against_the_reference_loop(fixture):
    from onet_amd import metrics as M
    g, sizes, _, cnt, cnt2 = fixture
    got = M.cascade_metrics(cnt, cnt2, sizes)
    assert sorted(got) == ["reference_return", "stage1", "stage2"]
    assert got["stage1"] == tuple(float(v) for v in g["stage1_epoch"]), (got["stage1"], g["stage1_epoch"])
    assert got["stage2"] == tuple(float(v) for v in g["stage2_epoch"]), (got["stage2"], g["stage2_epoch"])
    assert got["reference_return"] == tuple(float(v) for v in g["cascade_return"])
    assert got["reference_return"] == got["stage2"][:4] + got["stage1"][4:]         # TS:390: the first stage's tiou
    r0 = 0
    for b, n in enumerate(sizes):                              # each batch alone: the loop body's values
        one = M.cascade_metrics(cnt[r0:r0 + n], cnt2[r0:r0 + n], [n])
        assert one["stage1"] == tuple(float(v) for v in g["stage1_batch"][b]), b
        assert one["stage2"] == tuple(float(v) for v in g["stage2_batch"][b]), b
        r0 += n
    # the second stage's own flip decisions are the reference's
    tot2 = [cnt2[r0:r0 + n].sum(0) for r0, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
    assert [bool(t[0] + t[3] < t[1] + t[2]) for t in tot2] == [bool(v) for v in g["flipped2"]]
