"""Evaluation step either side of the hot path, mirroring the reference's helpers in
utils_20231218.py ("UT"): same names, argument meaning and edge-case behaviour, with the O(B*H*W)
work done by HIP kernels (per-frame min/max, per-image confusion counts) and only 4 integers per
image brought to the host."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .ops import _p, _stream, require_gpu
from .ops import label_counts as ops_label_counts

_EPS = float(np.spacing(1))


def tensor_normal_per_frame(input: torch.Tensor) -> torch.Tensor:
    """Scale every (b, c) frame to [0,1]: (x - min) / (max - min + np.spacing(1))  (UT:673-689)."""
    assert input.dim() == 4
    require_gpu(input)
    x = input.contiguous()
    nb, nc, h, w = x.shape
    y = torch.empty_like(x)
    _lib.call("onet_normalise_per_frame", _p(x), _p(y), nb * nc, h * w, _stream())
    return y


def confusion_counts(preds: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """[B, 4] int64 = (TP, FP, FN, TN) per image, positive class 1.  preds/targets: [B, H, W] (any integer
    or float dtype holding 0/1, as the reference's label tensors do)."""
    require_gpu(preds, targets)
    assert preds.shape == targets.shape
    B = preds.shape[0]
    p = preds.reshape(B, -1).to(torch.int64).contiguous()
    t = targets.reshape(B, -1).to(torch.int64).contiguous()
    counts = torch.empty((B, 4), dtype=torch.int64, device=p.device)
    _lib.call("onet_confusion2", _p(p), _p(t), _p(counts), B, p.shape[1], _stream())
    return counts


def _tot(counts):
    if not isinstance(counts, torch.Tensor):                 # host rows (EvalCounts.rows() as numpy, a list): [4] or [n, 4]
        c = np.asarray(counts, dtype=np.int64)
        return [int(v) for v in (c.sum(axis=0) if c.ndim == 2 else c)]
    c = counts.sum(dim=0).tolist() if counts.dim() == 2 else counts.tolist()
    return [int(v) for v in c]


def label_counts(preds: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """[1, 4] int64 = (TP, FP, FN, TN) of two label tensors of one shape taken as ONE image, each read in its own dtype (uint8 / bool,
    int32, int64, float32: no conversion pass) by ops.label_counts -- what the reference-signature forms of the helpers below count with."""
    assert isinstance(preds, torch.Tensor) and isinstance(targets, torch.Tensor)
    assert preds.shape == targets.shape
    counts = torch.zeros((1, 4), dtype=torch.int64, device=preds.device)
    return ops_label_counts(preds.reshape(1, -1), targets.reshape(1, -1), counts)


def _counts_of(preds, targets):
    """The helpers below take confusion counts ([4] or [n, 4], summed) or, like the reference's, (preds, targets[, num_k]) label
    tensors: -> the counts either way"""
    return preds if targets is None else label_counts(preds, targets)


def _acc(preds, targets=None, num_k=2) -> float:
    """(TP + TN) / all  (UT:100-117).  _acc(counts) | _acc(preds, targets, num_k)."""
    tp, fp, fn, tn = _tot(_counts_of(preds, targets))
    return (tp + tn) / float(tp + fp + fn + tn)


def _miou(preds, targets=None, num_k=2) -> float:
    """_miou(counts) | _miou(preds, targets, num_k): mean IoU over the 2 classes with the reference's empty-class rules (UT:119-155): a class absent from
    both prediction and ground truth scores 1, absent from exactly one scores 0.  The reference accumulates
    `torch.sum(inter) / torch.sum(union)` (a float32 tensor) and ends with `miou.item() / nums`: when NEITHER class
    takes the tensor branch -- prediction and ground truth each a single, different class -- `miou` is still a python
    float there and UT:152 raises AttributeError; mirrored, since "same error behaviour" is the drop-in rule."""
    assert num_k == 2
    tp, fp, fn, tn = _tot(_counts_of(preds, targets))
    miou, is_tensor = np.float32(0.0), False
    for inter, gt, pd in ((tn, tn + fp, tn + fn), (tp, tp + fn, tp + fp)):      # class 0, class 1
        if gt == 0 and pd == 0:
            miou = np.float32(miou + np.float32(1.0))
        elif gt == 0 or pd == 0:
            pass
        else:
            miou = np.float32(miou + np.float32(inter) / np.float32(gt + pd - inter))   # int64 / int64 -> float32 tensor
            is_tensor = True
    if not is_tensor:
        raise AttributeError("'float' object has no attribute 'item'")
    return float(miou) / 2


def _ratio32(num: int, den: int) -> float:
    """`torch.sum(a) / (torch.sum(b) + np.spacing(1))` as the reference evaluates it: int64 tensor + python float ->
    float32 tensor, int64 / float32 -> float32."""
    return float(np.float32(num) / (np.float32(den) + np.float32(_EPS)))


def _target_iou(preds, targets=None) -> float:
    tp, fp, fn, tn = _tot(_counts_of(preds, targets))
    return _ratio32(tp, tp + fp + fn)                                            # UT:157-173


def _detection_rate(preds, targets=None) -> float:
    tp, fp, fn, tn = _tot(_counts_of(preds, targets))
    return _ratio32(tp, tp + fn)                                                 # UT:175-186


def _false_alarm_rate(preds, targets=None) -> float:
    tp, fp, fn, tn = _tot(_counts_of(preds, targets))
    return _ratio32(fp, fp + tn)                                                 # UT:188-192


def flipped(counts):
    """confusion counts of 1 - pred: TP<->FN, FP<->TN."""
    return counts[..., [2, 3, 0, 1]]


def evaluate_nau_segmentation_v2(predict_label, gt_label=None, gt_k=2):
    """UT:213-234 -> (acc, miou, dr, far, t_iou).  (predict_label, gt_label) label tensors as in the reference, or confusion counts
    alone."""
    if gt_label is not None:
        assert predict_label.numel() == gt_label.numel()
        predict_label = label_counts(predict_label.reshape(-1), gt_label.reshape(-1))
    c = _tot(predict_label)                                    # (one copy to the host, then integers)
    return _acc(c), _miou(c), _detection_rate(c), _false_alarm_rate(c), _target_iou(c)


def _matched(counts):
    """Confusion counts of the prediction relabelled by its Hungarian match with the ground truth (UT:397-402): kept, or flipped"""
    c = np.asarray(_tot(counts), dtype=np.int64)
    return flipped(c) if dict(_hungarian_match(c, 2)).get(0, 0) == 1 else c


def evaluate_segmentation(predict_label, gt_label=None, gt_k=2, verbose=0):
    """UT:377-407 for two classes -> (acc, miou) of the prediction relabelled by its Hungarian match with the ground truth.
    (predict_label, gt_label) label tensors as in the reference, or confusion counts alone."""
    assert gt_k == 2
    if gt_label is not None:
        assert predict_label.numel() == gt_label.numel()
        predict_label = label_counts(predict_label.reshape(-1), gt_label.reshape(-1))
    c = _tot(predict_label)
    if verbose == 2:
        print("num_test: %d" % sum(c))
        for k, n in enumerate((c[1] + c[3], c[0] + c[2])):
            print("gt_k: %d count: %d" % (k, n))
    c = _matched(c)
    return _acc(c), _miou(c)


def epoch_metrics(rows, batch_sizes, protocol):
    """The metrics of a validation epoch from the per-image confusion counts alone: `rows` [n, 4] (EvalCounts.rows()), `batch_sizes`
    the images of each batch in order (EvalCounts.batch_sizes).  Host integer arithmetic, the reference's float32 steps included.
    protocol "simclutter" (TS:98-172): per batch the hard re-assignment on the batch totals (UT:439-453: the flip TP<->FN, FP<->TN
      where acc < acc of the flipped counts), the five metrics of evaluate_nau_segmentation_v2 on them, the mean over batches
      -> (acc, miou, dr, far, tiou).
    protocol "zy3" (UZ:151-208): per batch the Hungarian match on the batch totals (reorder_segmentation) and evaluate_segmentation
      on the relabelled batch (its values are not part of the epoch's result, its AttributeError is), then acc, miou, dr, far of every
      image on its relabelled counts (evaluate_nau_segmentation_v2), the mean over images -> (acc, miou, dr, far).
    UT:149's AttributeError is raised where the reference raises it: a batch (simclutter, zy3) or an image (zy3) whose prediction and
    ground truth are each one class, and different ones."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    if sum(batch_sizes) != rows.shape[0]:
        raise ValueError(f"epoch_metrics: {rows.shape[0]} rows for batches of {list(batch_sizes)}")
    if protocol not in ("simclutter", "zy3"):
        raise ValueError(f"epoch_metrics: protocol must be 'simclutter' or 'zy3', not {protocol!r}")
    vals, r0 = [], 0
    for n in batch_sizes:
        batch = rows[r0:r0 + n]
        r0 += n
        tot = batch.sum(axis=0)
        if protocol == "simclutter":
            if _acc(tot) < _acc(flipped(tot)):
                tot = flipped(tot)
            vals.append(evaluate_nau_segmentation_v2(tot))
        else:
            flip = dict(_hungarian_match(tot, 2)).get(0, 0) == 1
            evaluate_segmentation(flipped(tot) if flip else tot)
            for c in batch:
                vals.append(evaluate_nau_segmentation_v2(flipped(c) if flip else c)[:4])
    # (np.array(list).mean() of each list like the reference: numpy's pairwise sum of a 1-D array, not a row-by-row one)
    return tuple(float(np.array([v[k] for v in vals], dtype=np.float64).mean()) for k in range(len(vals[0])))


def _hungarian_match(counts, num_k: int = 2):
    """UT:258-285 on the confusion counts: votes[c1][c2] = #(pred == c1 and gt == c2), assignment minimising
    N - votes (scipy's linear_sum_assignment, the reference's own dependency, so ties resolve identically).
    -> [(pred class, gt class), ...]."""
    assert num_k == 2
    from scipy.optimize import linear_sum_assignment
    tp, fp, fn, tn = _tot(counts)
    votes = np.array([[tn, fn], [fp, tp]], dtype=np.float64)
    rows, cols = linear_sum_assignment(float(tp + fp + fn + tn) - votes)
    return [(int(r), int(c)) for r, c in zip(rows, cols)]


def reorder_segmentation(predict_label: torch.Tensor, gt_label: torch.Tensor) -> torch.Tensor:
    """UT:360-375: relabel the prediction by the Hungarian match between predicted and ground-truth classes (2 classes:
    keep, or swap 0 <-> 1); returns a new tensor of gt_label's shape."""
    require_gpu(predict_label, gt_label)
    assert predict_label.numel() == gt_label.numel()
    c = confusion_counts(predict_label.reshape(1, -1), gt_label.reshape(1, -1))
    match = dict(_hungarian_match(c, 2))
    p = predict_label.reshape(gt_label.shape).to(torch.int64).contiguous()
    if match.get(0, 0) == 1:                                                     # swap
        out = torch.empty_like(p)
        _lib.call("onet_flip_labels", _p(p), _p(out), p.numel(), _stream())
    else:
        out = p.clone()
    return out.to(predict_label.dtype)


def re_assign_label(predict_label: torch.Tensor, gt_label: torch.Tensor, gt_k: int = 2) -> torch.Tensor:
    """Hard re-assignment of UT:410-453: return 1 - pred if that has the higher pixel accuracy."""
    require_gpu(predict_label, gt_label)
    c = confusion_counts(predict_label.reshape(1, -1), gt_label.reshape(1, -1))
    if _acc(c) < _acc(flipped(c)):
        p = predict_label.to(torch.int64).contiguous()
        out = torch.empty_like(p)
        _lib.call("onet_flip_labels", _p(p), _p(out), p.numel(), _stream())
        return out.to(predict_label.dtype)
    return predict_label


def evaluate(onet, X, labels):
    """One eval step like TS:98-172 (forward in eval mode -> predict_label -> re_assign_label -> metrics)."""
    with torch.no_grad():
        Lt, Vt, Ld, Vd, S = onet(X)
        pred = re_assign_label(onet.predict_label(S), labels)
        c = confusion_counts(pred, labels)
    return {"acc": _acc(c), "miou": _miou(c), "target_iou": _target_iou(c), "dr": _detection_rate(c),
            "far": _false_alarm_rate(c)}


# ----------------------------------------------------------------------------- the performance report: SNR gain, two-stage cascade
def _get_psnr(sum_t, sum_bg, peak, n_t, numel):
    """get_psnr's statements after its sums (UT:466-476) in float64, in its order; a batch without target pixels gives what it gives
    (0 / 0 -> nan, log10(0) -> -inf), not an exception.  -> (psnr, snr)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        n_t = np.float64(n_t)
        target_power = np.float64(sum_t) / n_t
        erc = np.float64(sum_bg) / (np.float64(numel) - n_t)
        psnr = 10 * np.log10(np.float64(peak) ** 2 / erc)
        snr = 10 * np.log10(target_power / erc)
    return float(psnr), float(snr)


def snr_report(moment_rows, count_rows, batch_sizes):
    """measure_snr_on_fg's result (TS:46-95) from an epoch's per-image rows alone: `moment_rows` [n, 9] (EvalSnr.rows(): per image
    (sum v^2 on the target, sum v^2 off it, max v on it) of X, n(Vt), n(Vd)), `count_rows` [n, 4] (EvalCounts.rows()), `batch_sizes`
    the images of each batch in order.  Per batch get_psnr's formulas (UT:457-476) on the batch totals, float64: peak = the largest of
    the images' maxima, target pixels = TP + FN, all pixels = the four counts' sum; the foreground is n(Vt) where the hard
    re-assignment flips the batch (acc < acc of the flipped counts, compared as integers: both are the counts over one float64
    numel) and n(Vd) where it keeps it (TS:80-83).  -> {"input_psnr", "input_snr", "fg_psnr", "fg_snr": the means over batches
    (TS:91-94), "per_batch": [{"flipped", "input_psnr", "input_snr", "fg_psnr", "fg_snr"}]}"""
    mom = np.asarray(moment_rows, dtype=np.float64).reshape(-1, 9)
    cnt = np.asarray(count_rows, dtype=np.int64).reshape(-1, 4)
    if sum(batch_sizes) != mom.shape[0] or mom.shape[0] != cnt.shape[0]:
        raise ValueError(f"snr_report: {mom.shape[0]} moment rows and {cnt.shape[0]} count rows for batches of {list(batch_sizes)}")
    per_batch, r0 = [], 0
    for n in batch_sizes:
        m, c = mom[r0:r0 + n], cnt[r0:r0 + n]
        r0 += n
        tp, fp, fn, tn = (int(v) for v in c.sum(axis=0))
        flip = (tp + tn) < (fp + fn)
        vals = {}
        for name, s in (("input", 0), ("fg", 1 if flip else 2)):
            vals[name] = _get_psnr(m[:, 3 * s].sum(), m[:, 3 * s + 1].sum(), m[:, 3 * s + 2].max(), tp + fn, tp + fp + fn + tn)
        per_batch.append({"flipped": flip, "input_psnr": vals["input"][0], "input_snr": vals["input"][1],
                          "fg_psnr": vals["fg"][0], "fg_snr": vals["fg"][1]})
    out = {k: float(np.array([b[k] for b in per_batch], dtype=np.float64).mean()) for k in ("input_psnr", "input_snr", "fg_psnr", "fg_snr")}
    out["per_batch"] = per_batch
    return out


def cascade_metrics(rows1, rows2, batch_sizes):
    """test_2nd_stage_simclutter's numbers (TS:296-390) from the two stages' per-image confusion counts (the EvalCounts.rows() that
    verify_cascade filled): each stage through epoch_metrics(..., "simclutter").  -> {"stage1": (acc, miou, dr, far, tiou), "stage2":
    (...), "reference_return": (acc2, miou2, dr2, far2, tiou1) -- what TS:390 returns, the FIRST stage's tiou included as there}"""
    s1 = epoch_metrics(rows1, batch_sizes, "simclutter")
    s2 = epoch_metrics(rows2, batch_sizes, "simclutter")
    return {"stage1": s1, "stage2": s2, "reference_return": s2[:4] + s1[4:]}
