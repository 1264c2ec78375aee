"""Mint tests/golden/eval_batches.npz from the REAL reference's utils_20231218 ("UT"; run in the build container only).

    python tests/golden/make_eval_batches.py

Three validation batches of label maps (uint8, 24 x 40; 4, 4 and 2 images) and the numbers the bodies of the reference's two
validation loops produce on them with the reference's own functions:
  simclutter (TS:110-159)  per batch re_assign_label -> evaluate_nau_segmentation_v2, then the mean over batches;
  zy3 (UZ:161-208)         per batch reorder_segmentation -> evaluate_segmentation (its (acc, miou) stored per batch), per image
                           evaluate_nau_segmentation_v2 on the relabelled maps, then the mean over images.
Batch 0 is one the hard re-assignment flips, batch 1 one it keeps, batch 2 an exact tie (as many pixels right as wrong over the batch).
Only DATA is written: the maps and the recorded float64 values.  Nothing of the reference's source is copied."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402

H, W = 24, 40
SIZES = (4, 4, 2)


def batches():
    """-> [(pred, gt)] uint8 [n, H, W] each"""
    rng = np.random.Generator(np.random.PCG64(2025))
    out = []
    # 0: the prediction is mostly the complement of the ground truth (the hard re-assignment flips it)
    gt = (rng.random((SIZES[0], H, W)) > 0.8).astype(np.uint8)
    out.append((np.where(rng.random(gt.shape) > 0.15, 1 - gt, gt).astype(np.uint8), gt))
    # 1: mostly right (kept); one image without a single positive pixel in the ground truth
    gt = (rng.random((SIZES[1], H, W)) > 0.7).astype(np.uint8)
    gt[2] = 0
    out.append((np.where(rng.random(gt.shape) > 0.1, gt, 1 - gt).astype(np.uint8), gt))
    # 2: an exact tie over the batch: 600 of 960 pixels right in one image, 360 in the other
    gt = (rng.random((SIZES[2], H, W)) > 0.5).astype(np.uint8)
    pred = gt.copy().reshape(SIZES[2], -1)
    for i, right in enumerate((600, 360)):
        wrong = rng.permutation(H * W)[right:]
        pred[i, wrong] = 1 - pred[i, wrong]
    out.append((pred.reshape(gt.shape), gt))
    return out


def main():
    make_golden.import_reference()
    import utils_20231218 as ut
    out, sim, flips, zy3_batch, zy3_images = {}, [], [], [], []
    for b, (p, g) in enumerate(batches()):
        out[f"pred{b}"], out[f"gt{b}"] = p, g
        pred = torch.from_numpy(p.astype(np.int64))
        # TS:110-147 (the reference's label tensors are float32)
        label = torch.from_numpy(g.astype(np.float32))
        relabelled = ut.re_assign_label(pred, label)
        flips.append(not torch.equal(relabelled, pred))
        sim.append([float(v) for v in ut.evaluate_nau_segmentation_v2(relabelled, label)])
        # UZ:161-203
        label = torch.from_numpy(g.astype(np.int64))
        Y = ut.reorder_segmentation(pred, label)
        zy3_batch.append([float(v) for v in ut.evaluate_segmentation(Y, label, gt_k=2)])
        for i in range(p.shape[0]):
            zy3_images.append([float(v) for v in ut.evaluate_nau_segmentation_v2(Y[i], label[i], gt_k=2)[:4]])
    right = [int((p == g).sum()) for p, g in batches()]
    assert flips == [True, False, False] and 2 * right[2] == SIZES[2] * H * W, (flips, right)
    out["sizes"] = np.array(SIZES, dtype=np.int64)
    out["sim_flipped"] = np.array(flips)
    out["sim_batch"] = np.array(sim, dtype=np.float64)                      # [batch][acc, miou, dr, far, tiou]
    out["sim_epoch"] = np.array([np.array([r[k] for r in sim]).mean() for k in range(5)], dtype=np.float64)
    out["zy3_batch"] = np.array(zy3_batch, dtype=np.float64)                # [batch][acc, miou] of evaluate_segmentation
    out["zy3_images"] = np.array(zy3_images, dtype=np.float64)              # [image][acc, miou, dr, far]
    out["zy3_epoch"] = np.array([np.array([r[k] for r in zy3_images]).mean() for k in range(4)], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "eval_batches.npz"), **out)
    print("eval_batches: sim", out["sim_epoch"].round(4).tolist(), "flipped", flips, "| zy3", out["zy3_epoch"].round(4).tolist(),
          "per batch", out["zy3_batch"].round(4).tolist())


if __name__ == "__main__":
    main()
