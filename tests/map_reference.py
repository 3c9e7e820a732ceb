"""Plain numpy model of mean average precision (csrc/metrics.hip): what the kernels' integer results are compared with exactly.

No tiling, no grouping by (image, class), no structure shared with the device code:

`prediction_order`  one np.lexsort on (row, -score, class), rows of a foreign class (c < 0 or c >= num_classes) last.
`outcomes`          a literal transliteration of the loop of detection/metrics/mean_average_precision.py:40-70: ONE pass over all
                    predictions in global descending-score order (ties: lower row first), a matched set per (image, class).  The IoU is
                    computed in float32 in the operation order of bf/utils/box_utils.py:49-101, so that `iou > threshold` is decided on
                    the same number as on the device (test_box_utils_gpu.py pins the device's IoU bit-equal to that arithmetic).
                    0 = neither counter moves, 1 = true positive, 2 = false positive, by prediction row.
`average_precision` :71-111 in float64 from the integer counts: cumulative tp / fp -> precision (0 / 0 = NaN when the first ranked
                    prediction of a class hits a `difficult` box), the reverse NaN-propagating running maximum, area or 11-point AP.
                    The 11-point thresholds k / 10 are compared with the recall tp / total as exact rationals (k * total > 10 * tp):
                    that is what the reference's float32 comparison decides whenever total < 10^5 (equal rationals round to equal
                    floats; unequal ones differ by >= 1 / (10 total), far more than a float32 rounding).

Ground truth comes packed as for the library: rows [total_gt, stride] float32 + offsets int32 [num_images + 1]; `pack` makes that
from a list of per-image arrays.  Class at column 4; difficult flag at column 6 when stride > 6.  An image id outside
[0, num_images) has no ground truth: such a prediction is a false positive.
"""
import numpy as np

F32 = np.float32


def pack(gts, stride=None):
    """list of [G_i, stride] -> (rows [sum G_i, stride] float32, offsets int32 [len + 1])"""
    if stride is None:
        stride = int(gts[0].shape[1]) if len(gts) else 6
    counts = [int(g.shape[0]) for g in gts]
    rows = np.concatenate([np.asarray(g, F32).reshape(-1, stride) for g in gts], 0) if sum(counts) else np.zeros((0, stride), F32)
    return np.ascontiguousarray(rows, F32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _as_int(col):
    """C's (int) of a float column: truncation towards zero"""
    return np.trunc(np.asarray(col, np.float64)).astype(np.int64)


def prediction_order(pred, num_classes):
    """-> int64 [n]: rows in (class ascending, score descending, row ascending) order, foreign classes last in row order.
    The scores are compared as floats: -0.0 == +0.0 (row order decides), +inf first, negative scores last."""
    pred = np.asarray(pred, F32).reshape(-1, 7)
    c = _as_int(pred[:, 5])
    foreign = (c < 0) | (c >= num_classes)
    cls = np.where(foreign, num_classes, c)
    neg = np.where(foreign, F32(0), -pred[:, 6])
    return np.lexsort((np.arange(pred.shape[0]), neg, cls)).astype(np.int64)


def _iou_f32(box, gt_boxes):
    """box [4], gt_boxes [G, 4] float32 -> [G] float32: intersection = clamp(min of max corners - max of min corners, 0) product,
    iou = inter / ((area_a + area_b) - inter); NaN (0 / 0) for two degenerate boxes, as the reference has it."""
    zero = F32(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        def area(x1, y1, x2, y2):
            w, h = x2 - x1, y2 - y1
            return np.where(w < zero, zero, w) * np.where(h < zero, zero, h)
        area_a = area(box[0], box[1], box[2], box[3])
        area_b = area(gt_boxes[:, 0], gt_boxes[:, 1], gt_boxes[:, 2], gt_boxes[:, 3])
        inter = area(np.maximum(box[0], gt_boxes[:, 0]), np.maximum(box[1], gt_boxes[:, 1]),
                     np.minimum(box[2], gt_boxes[:, 2]), np.minimum(box[3], gt_boxes[:, 3]))
        out = inter / ((area_a + area_b) - inter)
    assert out.dtype == F32
    return out


def outcomes(pred, rows, offs, num_classes, iou_threshold):
    """-> uint8 [n] by prediction row (see the module docstring)"""
    pred = np.asarray(pred, F32).reshape(-1, 7)
    rows = np.asarray(rows, F32)
    n, stride, num_images = pred.shape[0], rows.shape[1], len(offs) - 1
    ignore_difficult = stride > 6                                                   # :22
    thr = F32(iou_threshold)
    gt_class = _as_int(rows[:, 4])
    grouped = {}                                                                    # (image, class) -> ground-truth row numbers (:27-38)

    def group(id_, c):
        if (id_, c) not in grouped:
            lo, hi = (int(offs[id_]), int(offs[id_ + 1])) if 0 <= id_ < num_images else (0, 0)
            grouped[(id_, c)] = lo + np.flatnonzero(gt_class[lo:hi] == c)
        return grouped[(id_, c)]

    out = np.zeros(n, np.uint8)
    ids, cls = _as_int(pred[:, 0]), _as_int(pred[:, 5])
    matched = {}
    for r in np.lexsort((np.arange(n), -pred[:, 6])):                               # :40-41, stable: lower row first
        id_, c = int(ids[r]), int(cls[r])
        if c < 0 or c >= num_classes:
            continue                                                                # a foreign class is in no class's lists
        g = group(id_, c)
        if g.size == 0:                                                             # :55-57
            out[r] = 2
            continue
        iou = _iou_f32(pred[r, 1:5], rows[g, :4])                                   # :59
        nan = np.flatnonzero(np.isnan(iou))
        index = int(nan[0]) if nan.size else int(np.argmax(iou))                    # :60 torch.max: NaN wins, else the first maximum
        value = iou[index]
        if value > thr:                                                             # :61
            if not ignore_difficult or rows[g[index], 6] == 0:                      # :62
                seen = matched.setdefault((id_, c), set())
                if index not in seen:                                               # :63-65
                    out[r] = 1
                    seen.add(index)
                else:
                    out[r] = 2                                                      # :67
        else:
            out[r] = 2                                                              # :69
    return out


def total_positive(rows, num_classes):
    """counted ground truths per class (:27-35): int64 [num_classes]"""
    rows = np.asarray(rows, F32)
    c = _as_int(rows[:, 4])
    ok = (c >= 0) & (c < num_classes)
    if rows.shape[1] > 6:
        ok &= rows[:, 6] == 0
    return np.bincount(c[ok], minlength=num_classes).astype(np.int64)


def class_ap(flags, total, voc):
    """AP of one class from its outcomes in rank order (uint8 [m]) and its count of counted ground truths (> 0), float64 (:80-106)"""
    if len(flags) == 0:
        tp, fp = np.array([0], np.int64), np.array([1], np.int64)                   # :81-89
    else:
        tp, fp = np.cumsum(flags == 1).astype(np.int64), np.cumsum(flags == 2).astype(np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        precision = np.concatenate([tp / (tp + fp).astype(np.float64), [0.0]])       # :90-92, 0 / 0 = NaN
    for i in range(len(precision) - 1, 0, -1):                                      # :93-94, torch.max propagates NaN
        a, b = precision[i - 1], precision[i]
        precision[i - 1] = a if (a != a or a > b) else b
    if voc:                                                                         # :98-102
        # indexes[k] = #(k / 10 > recall), recall = [tp / total ..., 1]; as exact rationals (module docstring); k / 10 > 1 never holds
        idx = [int(np.count_nonzero(k * int(total) > 10 * tp)) for k in range(11)]
        return float(np.mean(precision[idx]))
    recall = np.concatenate([[0.0], tp / float(total), [1.0]])                      # :104-105
    return float(np.dot(recall[1:] - recall[:-1], precision))


def mean_average_precision(pred, rows, offs, num_classes, iou_threshold=0.5, voc=False, order=None, outcome=None):
    """-> (mAP float, ap float64 [num_classes] with NaN for classes without counted ground truth, order int64 [n], outcome uint8 [n]).
    `order` / `outcome`: results of an earlier call on the same input (they do not depend on `voc`)."""
    pred = np.asarray(pred, F32).reshape(-1, 7)
    if order is None:
        order = prediction_order(pred, num_classes)
    if outcome is None:
        outcome = outcomes(pred, rows, offs, num_classes, iou_threshold)
    tot = total_positive(rows, num_classes)
    cls = _as_int(pred[order, 5])
    ap = np.full(num_classes, np.nan, np.float64)
    for c in range(num_classes):
        if tot[c]:                                                                  # :73-75, :79
            ap[c] = class_ap(outcome[order[cls == c]], tot[c], voc)
    counted = ap[tot > 0]
    return (float(np.sum(counted) / counted.size) if counted.size else float('nan')), ap, order, outcome   # :111
