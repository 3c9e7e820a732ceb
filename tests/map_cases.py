"""Directed inputs of the exact mean-average-precision tests (test_map_reference.py on the CPU, test_map_exact_gpu.py on the device).

Every builder returns (pred [n, 7] float32, gts: list of [G_i, stride] float32, num_classes); `CASES` names them.  The sizes are chosen
against the constants of csrc/metrics.hip: the radix sort's tile of 4096 keys (four wave quarters of 1024), map_ap_kernel's rounds of
256 positions, the four 8-bit digits of the image key."""
import functools

import numpy as np

from single_shot_detection_amd import synthetic as syn

F32 = np.float32
SIZE = 300.0


def _boxes(rng, g):
    xy = rng.uniform(0, 0.7 * SIZE, (g, 2))
    wh = rng.uniform(0.05, 0.4, (g, 2)) * SIZE
    return np.concatenate([xy, np.minimum(xy + wh, SIZE - 1)], 1)


def _gt_rows(box, cls, difficult, stride=7):
    g = box.shape[0]
    out = np.zeros((g, stride), np.float64)
    out[:, :4], out[:, 4] = box, cls
    if stride > 5:
        out[:, 5] = 1.0
    if stride > 6:
        out[:, 6] = difficult
    if stride > 7:
        out[:, 7:] = 7.5                                   # attribute columns the metric never reads
    return out


def _jitter(rng, box, scale=0.06):
    wh = np.tile(box[2:] - box[:2], 2)
    return box + rng.normal(0, scale, 4) * wh


def _finish(rng, preds, gts, stride=7):
    pred = np.concatenate(preds, 0).astype(F32)
    pred = pred[rng.permutation(pred.shape[0])]
    gts = [np.ascontiguousarray(np.asarray(g, np.float64).reshape(-1, stride), F32) for g in gts]
    return np.ascontiguousarray(pred), gts


def across_tiles():
    """~13.5 thousand predictions: three full sort tiles and a ragged one, image ids past 256 (two non-trivial digits of the image key),
    scores rounded to 1 / 20 so that exact ties lie inside (image, class) groups: the matcher's result needs both sorts to be stable."""
    pred, gts = syn.make_map_case(seed=201, num_images=1100, num_classes=21, with_difficult=True, max_gt=9, noise_fp=16, difficult_p=0.08,
                                  unique_scores=False)
    return pred, gts, 21


def wide_image_ids():
    """num_images = 66 000 with ~200 populated images spread over the id range (0, 255, 256, 65 535, 65 536, 65 999 among them): the image
    key has three non-trivial digits; predictions of images -1, num_images and 2^24 have no ground truth and are false positives."""
    rng = np.random.default_rng(202)
    num_images, num_classes = 66000, 7
    ids = np.unique(np.concatenate([[0, 255, 256, 65535, 65536, 65999], rng.integers(0, num_images, 194)]))
    gts = [np.zeros((0, 7))] * num_images
    preds = []
    for i in ids:
        g = int(rng.integers(1, 6))
        box, cls = _boxes(rng, g), rng.integers(1, num_classes, g)
        gts[i] = _gt_rows(box, cls, rng.random(g) < 0.1)
        rows = [np.concatenate([[i], _jitter(rng, box[k]), [cls[k]], [rng.uniform(0.2, 1.0)]]) for k in range(g) for _ in range(int(rng.integers(0, 3)))]
        rows += [np.concatenate([[i], _boxes(rng, 1)[0], [rng.integers(1, num_classes)], [rng.uniform(0.01, 0.6)]]) for _ in range(int(rng.integers(0, 4)))]
        if rows:
            preds.append(np.stack(rows))
    for bad in (-1, num_images, 2 ** 24):
        # (copies of real ground-truth boxes of image 0, with high scores: only the image id makes them false positives)
        preds.append(np.stack([np.concatenate([[bad], gts[0][k % len(gts[0]), :4], [gts[0][k % len(gts[0]), 4]], [0.95 - 0.01 * k]]) for k in range(3)]))
    pred, gts = _finish(rng, preds, gts)
    return pred, gts, num_classes


def score_range():
    """Negative scores, +inf, equal scores, and both zeros in one class.  As floats -0.0 == +0.0: the reference's comparison (and the
    oracle's comparator) leave them in row order."""
    rng = np.random.default_rng(203)
    num_classes, num_images = 4, 6
    special = np.array([np.inf, np.inf, 2.5, 1.0, 1.0, 0.5, 0.0, -0.0, 0.0, -0.0, -0.0, 0.0, -1e-30, -0.25, -0.25, -3.0, -1e30, 1e-40, -1e-40], np.float64)
    gts, preds = [], []
    for i in range(num_images):
        g = 4
        box, cls = _boxes(rng, g), np.array([1, 1, 2, 3])
        gts.append(_gt_rows(box, cls, rng.random(g) < 0.2))
        rows = []
        for c in (1, 2):
            for s in rng.permutation(special):
                k = int(rng.integers(0, g))
                b = _jitter(rng, box[k]) if rng.random() < 0.6 else _boxes(rng, 1)[0]
                rows.append(np.concatenate([[i], b, [c], [s]]))
        rows += [np.concatenate([[i], _jitter(rng, box[3]), [3], [rng.uniform(-1, 1)]]) for _ in range(3)]
        preds.append(np.stack(rows))
    pred, gts = _finish(rng, preds, gts)
    return pred, gts, num_classes


def _segment_edges(difficult_head):
    rng = np.random.default_rng(204)
    num_classes, num_images = 10, 40
    gts = [[] for _ in range(num_images)]
    preds = []
    for c, m in ((0, 255), (1, 256), (2, 257), (3, 512)):      # map_ap_kernel's 256-wide rounds: one short, one exact, one + 1, two exact
        rows = []
        for i in range(num_images):
            box = _boxes(rng, 2)
            gts[i].append(_gt_rows(box, [c, c], rng.random(2) < 0.15))
            rows += [np.concatenate([[i], _jitter(rng, box[k]), [c], [rng.uniform(0.2, 1.0)]]) for k in range(2) for _ in range(int(rng.integers(0, 3)))]
        rows = rows[:m // 2]
        while len(rows) < m:
            rows.append(np.concatenate([[rng.integers(0, num_images)], _boxes(rng, 1)[0], [c], [rng.uniform(0.01, 0.6)]]))
        preds.append(np.stack(rows))
    # class 4: ground truth and no prediction (AP 0)
    gts[0].append(_gt_rows(_boxes(rng, 1), [4], [0]))
    # class 5: predictions, and only a difficult ground truth: nothing counted (AP NaN, not part of the mean); one prediction hits it
    box = _boxes(rng, 1)
    gts[1].append(_gt_rows(box, [5], [1]))
    preds.append(np.stack([np.concatenate([[1], box[0], [5], [0.9]])] +
                          [np.concatenate([[rng.integers(0, num_images)], _boxes(rng, 1)[0], [5], [rng.uniform(0.01, 0.6)]]) for _ in range(19)]))
    # foreign class ids on both sides, in predictions and in the ground truth
    gts[2].append(_gt_rows(_boxes(rng, 2), [-2, 12], [0, 0]))
    preds.append(np.stack([np.concatenate([[rng.integers(0, num_images)], _boxes(rng, 1)[0], [c], [rng.uniform(0.01, 1.0)]])
                           for c in (-3, -1, 10, 15, -3, 10, 1000000)]))
    if difficult_head:
        # class 6: the best prediction hits a difficult box: tp = fp = 0 at rank 0, precision 0 / 0 = NaN -> AP NaN, mAP NaN
        box = _boxes(rng, 2)
        gts[3].append(_gt_rows(box, [6, 6], [1, 0]))
        preds.append(np.stack([np.concatenate([[3], box[0], [6], [0.99]]), np.concatenate([[3], box[1], [6], [0.7]]),
                               np.concatenate([[4], box[1], [6], [0.5]])]))
    # class 7: exactly 10 counted positives, each hit exactly once: the recalls are k / 10, exactly the 11-point thresholds
    rows = []
    for i in range(10):
        box = _boxes(rng, 1)
        gts[10 + i].append(_gt_rows(box, [7], [0]))
        rows.append(np.concatenate([[10 + i], box[0], [7], [rng.uniform(0.2, 1.0)]]))
        rows += [np.concatenate([[10 + i], _boxes(rng, 1)[0], [7], [rng.uniform(0.01, 1.0)]]) for _ in range(int(rng.integers(0, 3)))]
    preds.append(np.stack(rows))
    pred, gts = _finish(rng, preds, [np.concatenate(g, 0) for g in gts])
    return pred, gts, num_classes


def segment_edges():
    return _segment_edges(False)


def segment_edges_difficult_head():
    return _segment_edges(True)


def gt_width(stride):
    """One small input at ground-truth row widths 5 (no score column), 6, 7 (difficult flag) and 9"""
    rng = np.random.default_rng(205)
    num_classes, num_images = 5, 9
    gts, preds = [], []
    for i in range(num_images):
        g = int(rng.integers(0, 5))
        box, cls = _boxes(rng, g), rng.integers(0, num_classes, g)
        gts.append(_gt_rows(box, cls, rng.random(g) < 0.3, stride))
        rows = [np.concatenate([[i], _jitter(rng, box[k]), [cls[k]], [rng.uniform(0.2, 1.0)]]) for k in range(g) for _ in range(int(rng.integers(0, 3)))]
        rows += [np.concatenate([[i], _boxes(rng, 1)[0], [rng.integers(0, num_classes)], [rng.uniform(0.01, 0.6)]]) for _ in range(2)]
        preds.append(np.stack(rows))
    pred, gts = _finish(rng, preds, gts, stride)
    return pred, gts, num_classes


BOUNDARY = 4096   # the sort's tile: map_match_kernel's workgroups (128 threads) and the scatter's tiles both change here


def _tile_boundary(straddle):
    """(image, class) groups of 1..9 predictions laid out so that, in (image, class, score) order, a group STARTS at position 4096
    (straddle = False) or lies across it, 3 before and 4 behind (straddle = True); scores in 1 / 16 steps tie inside groups."""
    rng = np.random.default_rng(206 + int(straddle))
    num_classes = 6
    sizes, total, target = [], 0, BOUNDARY - (3 if straddle else 0)
    while total < target:
        s = int(min(rng.integers(1, 10), target - total))
        sizes.append(s)
        total += s
    sizes += [7] + [int(rng.integers(1, 10)) for _ in range(40)]
    gts, preds, image, cls = [], [], 0, 0
    per_image = []
    for s in sizes:
        if cls == 0:
            box = _boxes(rng, 2 * (num_classes - 1))
            per_image = _gt_rows(box, np.repeat(np.arange(1, num_classes), 2), rng.random(len(box)) < 0.1)
            gts.append(per_image)
        cls += 1
        mine = per_image[per_image[:, 4] == cls]
        rows = []
        for _ in range(s):
            b = _jitter(rng, mine[int(rng.integers(0, len(mine))), :4]) if rng.random() < 0.7 else _boxes(rng, 1)[0]
            rows.append(np.concatenate([[image], b, [cls], [np.round(rng.uniform(0.05, 1.0) * 16) / 16]]))
        preds.append(np.stack(rows))
        if cls == num_classes - 1:
            cls, image = 0, image + 1
    pred, gts = _finish(rng, preds, gts)
    return pred, gts, num_classes


def group_positions(pred):
    """(starts, ends) of the (image, class) groups in (image, class) order -- where the second sort puts them"""
    key = pred[:, 0].astype(np.int64) * (1 << 20) + pred[:, 5].astype(np.int64)
    _, counts = np.unique(key, return_counts=True)
    ends = np.cumsum(counts)
    return ends - counts, ends


CASES = {
    'across_tiles': across_tiles,
    'wide_image_ids': wide_image_ids,
    'score_range': score_range,
    'segment_edges': segment_edges,
    'segment_edges_difficult_head': segment_edges_difficult_head,
    'gt_width_5': functools.partial(gt_width, 5),
    'gt_width_6': functools.partial(gt_width, 6),
    'gt_width_7': functools.partial(gt_width, 7),
    'gt_width_9': functools.partial(gt_width, 9),
    'head_at_tile_boundary': functools.partial(_tile_boundary, False),
    'group_across_tile_boundary': functools.partial(_tile_boundary, True),
}

_built, _ref = {}, {}


def case(name):
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]


def reference(name, voc):
    """map_reference.mean_average_precision of a case, computed once (order and outcomes are shared by both AP modes)"""
    import map_reference as mr
    pred, gts, num_classes = case(name)
    if (name, voc) not in _ref:
        rows, offs = mr.pack(gts)
        prev = _ref.get((name, not voc))
        _ref[(name, voc)] = mr.mean_average_precision(pred, rows, offs, num_classes, 0.5, voc, order=prev and prev[2], outcome=prev and prev[3])
    return _ref[(name, voc)]
