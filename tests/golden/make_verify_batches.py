"""Mint tests/golden/verify_batches.npz from the REAL reference's utils_20231218 ("UT"; run in the build container only).

    python tests/golden/make_verify_batches.py

Five validation batches (X, Vt, Vd, gt) -- three of 24 x 40 maps, two of 25 x 37 (HW % 4 != 0) -- and what the bodies of the reference's
measure_snr_on_fg (TS:60-89) and test_2nd_stage_simclutter (TS:312-350) produce on them with the reference's own functions, the
forward's outputs being the recorded Vt, Vd (and a recorded second pair Vt2, Vd2 standing in for the second model's output):
  0  24 x 40, 3 images, gt float32: the hard re-assignment flips the batch (Vt is the foreground)
  1  24 x 40, 3 images, gt uint8: kept; image 1 has no positive pixel, image 2's Vd is one constant (max == min: the denominator is
     spacing(1), the foreground map of that image is 0)
  2  24 x 40, 2 images, gt float32: an exact tie over the batch (kept)
  3  25 x 37, 2 images, gt uint8: no positive pixel in the whole batch (get_psnr gives -inf and nan)
  4  25 x 37, 3 images, gt float32: every V negative; flipped
The values of X, V are multiples of 1/64 (the file compresses; every fp32 step of the reference still rounds).
Recorded per batch: get_psnr(X, label) and get_psnr(fg, label) as the reference returns them (fp32 tensors' .item()), the flip flag,
X2 = tensor_normal_per_frame(the selected V), the five metrics of each stage; over the epoch measure_snr_on_fg's four means and
test_2nd_stage_simclutter's means; the same get_psnr -- the reference's function, called on the same fp32 inputs converted to float64 --
and ref_gap_db, the largest finite |fp32 result - float64 result|.
Only DATA is written.  Nothing of the reference's source is copied."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402

SHAPES = [(3, 24, 40), (3, 24, 40), (2, 24, 40), (2, 25, 37), (3, 25, 37)]
GT_DTYPES = [np.float32, np.uint8, np.float32, np.uint8, np.float32]
Q = 64.0


def _quant(a):
    return (np.round(a * Q) / Q).astype(np.float32)


def _scores(rng, pred, offset=0.0):
    """(Vt, Vd) whose head label (Vd > Vt) is `pred`: a gap of at least 1/2 either way, negative values among them"""
    vt = _quant(rng.standard_normal(pred.shape) * 1.5 + offset)
    gap = _quant(0.5 + rng.random(pred.shape) * 1.5)
    return vt, (vt + np.where(pred == 1, gap, -gap)).astype(np.float32)


def _noisy(rng, gt, right):
    """a label map that agrees with gt on about `right` of the pixels"""
    return np.where(rng.random(gt.shape) < right, gt, 1 - gt).astype(np.uint8)


def batches():
    """-> [(X, Vt, Vd, gt, Vt2, Vd2)]: fp32 [n, 1, H, W] maps, gt [n, H, W] in the batch's dtype"""
    rng = np.random.Generator(np.random.PCG64(20250407))
    out = []
    for b, (n, H, W) in enumerate(SHAPES):
        gt = (rng.random((n, H, W)) > 0.85).astype(np.uint8)
        if b == 1:
            gt[1] = 0
        if b == 3:
            gt[:] = 0
        if b == 2:                                            # an exact tie: 600 + 360 of 2 x 960 pixels right
            pred = gt.copy().reshape(n, -1)
            for i, right in enumerate((600, 360)):
                wrong = rng.permutation(H * W)[right:]
                pred[i, wrong] = 1 - pred[i, wrong]
            pred = pred.reshape(gt.shape)
        else:
            pred = _noisy(rng, gt, 0.15 if b in (0, 4) else 0.9)
        vt, vd = _scores(rng, pred, offset=-10.0 if b == 4 else 0.0)
        if b == 1:                                            # a constant Vd frame; the labels stay pred's
            gap = _quant(0.5 + rng.random((H, W)))
            vd[2] = 0.25
            vt[2] = np.float32(0.25) + np.where(pred[2] == 1, -gap, gap)
        if b == 4:
            assert vt.max() < 0 and vd.max() < 0
        X = _quant(np.clip(rng.random((n, H, W)) * 0.6 + gt * (0.3 + 0.4 * rng.random((n, H, W))), 0, 1))
        pred2 = _noisy(rng, gt, 0.1 if b in (1, 3) else 0.95)
        vt2, vd2 = _scores(rng, pred2)
        f = lambda a: np.ascontiguousarray(a.reshape(n, 1, H, W), dtype=np.float32)
        out.append((f(X), f(vt), f(vd), gt.astype(GT_DTYPES[b]), f(vt2), f(vd2)))
    return out


def _labels(Vt, Vd):
    """predict_label of the head's S (OV:193-201)"""
    return torch.argmax(torch.softmax(torch.cat([Vt, Vd], dim=1), dim=1), dim=1)


def main():
    make_golden.import_reference()
    import utils_20231218 as ut
    out, flips, flips2, psnr32, psnr64, stage1, stage2 = {}, [], [], [], [], [], []
    for b, arrays in enumerate(batches()):
        for name, a in zip(("X", "Vt", "Vd", "gt", "Vt2", "Vd2"), arrays):
            out[f"{name}{b}"] = a
        X, Vt, Vd, label, Vt2, Vd2 = (torch.from_numpy(a) for a in arrays)
        raw = _labels(Vt, Vd)
        assert torch.equal(raw, (Vd > Vt).squeeze(1).long())
        # TS:68-89
        nt, nd = ut.tensor_normal_per_frame(Vt), ut.tensor_normal_per_frame(Vd)
        pred = ut.re_assign_label(raw, label)
        kept = torch.equal(raw, pred)
        fg = (nd if kept else nt).squeeze(dim=1)
        flips.append(not kept)
        psnr32.append(list(ut.get_psnr(X.squeeze(dim=1), label)) + list(ut.get_psnr(fg, label)))
        psnr64.append(list(ut.get_psnr(X.squeeze(dim=1).double(), label.double())) + list(ut.get_psnr(fg.double(), label.double())))
        # TS:315-345
        stage1.append([float(v) for v in ut.evaluate_nau_segmentation_v2(pred, label)])
        X2 = ut.tensor_normal_per_frame(Vd if kept else Vt)
        out[f"X2_{b}"] = X2.numpy()
        raw2 = _labels(Vt2, Vd2)
        pred2 = ut.re_assign_label(raw2, label)
        flips2.append(not torch.equal(raw2, pred2))
        stage2.append([float(v) for v in ut.evaluate_nau_segmentation_v2(pred2, label)])
    assert flips == [True, False, False, False, True], flips
    a32, a64 = np.array(psnr32, dtype=np.float64), np.array(psnr64, dtype=np.float64)
    fin = np.isfinite(a32) & np.isfinite(a64)
    assert np.array_equal(np.isnan(a32), np.isnan(a64)) and np.array_equal(a32[~fin], a64[~fin], equal_nan=True)
    out["sizes"] = np.array([s[0] for s in SHAPES], dtype=np.int64)
    out["flipped"] = np.array(flips)
    out["flipped2"] = np.array(flips2)
    out["psnr_fp32"] = a32                                    # [batch][input_psnr, input_snr, fg_psnr, fg_snr]: the reference's values
    out["psnr_fp64"] = a64                                    # ... its formulas on the same inputs in float64
    mean = lambda a: np.array([np.array(list(a[:, k])).mean() for k in range(a.shape[1])], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        out["epoch_fp32"], out["epoch_fp64"] = mean(a32), mean(a64)       # TS:91-94 over all five batches (nan / inf with batch 3)
        out["epoch_fp32_targets"], out["epoch_fp64_targets"] = mean(a32[[0, 1, 2, 4]]), mean(a64[[0, 1, 2, 4]])   # ... without batch 3
    out["ref_gap_db"] = np.float64(np.abs(a32[fin] - a64[fin]).max())
    s1, s2 = np.array(stage1, dtype=np.float64), np.array(stage2, dtype=np.float64)
    out["stage1_batch"], out["stage2_batch"] = s1, s2         # [batch][acc, miou, dr, far, tiou]
    out["stage1_epoch"], out["stage2_epoch"] = mean(s1), mean(s2)
    out["cascade_return"] = np.concatenate([out["stage2_epoch"][:4], out["stage1_epoch"][4:]])      # TS:390
    path = os.path.join(HERE, "verify_batches.npz")
    np.savez_compressed(path, **out)
    print("verify_batches:", os.path.getsize(path), "bytes; flipped", flips, flips2, "ref_gap_db", float(out["ref_gap_db"]))
    print("fp32", a32.round(4).tolist())
    print("fp64", a64.round(4).tolist())
    print("stage1", out["stage1_epoch"].round(4).tolist(), "stage2", out["stage2_epoch"].round(4).tolist())


if __name__ == "__main__":
    main()
