"""Inputs of the COCO evaluation tests (tests/test_coco_eval.py on the CPU, tests/test_coco_eval_gpu.py on the GPU): hand-built cases
whose results can be worked out on paper, random cases on top of synthetic.make_map_case (column 6 read as the crowd flag), and edge
shapes built directly.  A case is a dict: pred [N, 7] fp32, gts list of [G_i, 6 or 7] fp32, num_classes, and the optional gt_areas (list
per image), image_area_scale, iou_thrs, rec_thrs, area_rngs, max_dets (None: the defaults).

Builder's condition: no (detection, gt) IoU of a generated case lies within 1e-12 of an IoU threshold, so that a last-bit difference
could never flip a match; a case that misses it is redrawn from the next seed.  The hand-built cases that sit ON a threshold do so with
exactly representable quotients (``exact=True``): there the check demands equality to the bit."""
import numpy as np

from single_shot_detection_amd import synthetic as syn
from coco_eval_reference import default_tables

KEYS = ('gt_areas', 'image_area_scale', 'iou_thrs', 'rec_thrs', 'area_rngs', 'max_dets')


def case(pred, gts, num_classes, exact=False, **kw):
    assert set(kw) <= set(KEYS), kw
    c = dict(pred=np.ascontiguousarray(np.asarray(pred, np.float32).reshape(-1, 7)), gts=[np.asarray(g, np.float32) for g in gts], num_classes=num_classes,
             exact=exact)
    c.update({k: kw.get(k) for k in KEYS})
    return c


def reference_kwargs(c):
    return {k: c[k] for k in KEYS}


def all_ious(c):
    """Every IoU a matching could look at: (detection, gt) pairs of one image and class, by the rule of that gt (crowd or not)."""
    pred, out = c['pred'].astype(np.float64), []
    for i, g in enumerate(c['gts']):
        g = g.astype(np.float64)
        d = pred[pred[:, 0].astype(np.int64) == i]
        if not len(g) or not len(d):
            continue
        iw = np.minimum(d[:, None, 3], g[None, :, 2]) - np.maximum(d[:, None, 1], g[None, :, 0])
        ih = np.minimum(d[:, None, 4], g[None, :, 3]) - np.maximum(d[:, None, 2], g[None, :, 1])
        inter = np.maximum(0.0, iw) * np.maximum(0.0, ih)
        ad = ((d[:, 3] - d[:, 1]) * (d[:, 4] - d[:, 2]))[:, None]
        ag = ((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]))[None, :]
        crowd = (g[:, 6] != 0)[None, :] if g.shape[1] > 6 else np.zeros((1, len(g)), bool)
        den = np.where(crowd, ad + 0 * ag, ad + ag - inter)
        v = np.where(den == 0, 0.0, inter / np.where(den == 0, 1.0, den))
        out.append(v[d[:, 5][:, None] == g[None, :, 4]])
    return np.concatenate(out) if out else np.zeros(0)


def off_thresholds(c):
    """The builder's condition (module docstring)."""
    thr = np.asarray(default_tables()[0] if c['iou_thrs'] is None else c['iou_thrs'], np.float64)
    thr = np.minimum(thr, 1 - 1e-10)
    v = all_ious(c)
    near = np.abs(v[:, None] - thr[None, :]) <= 1e-12
    if c['exact']:
        return bool(np.all((v[:, None] == thr[None, :])[near]))
    return not near.any()


# ---- hand-built cases: name -> (case, expected statistics) ------------------------------------------------------------------------------
def hand_cases():
    out = {}
    # IoU 0.78: matched at six of the ten thresholds
    out['iou_078'] = (case([[0, 0, 0, 100, 78, 1, .9]], [[[0, 0, 100, 100, 1, 1]]], 2),
                      dict(AP=.6, AP50=1, AP75=1, APs=-1, APm=-1, APl=.6, AR1=.6, AR10=.6, AR100=.6, ARs=-1, ARm=-1, ARl=.6))
    # IoU exactly 0.5 from exactly representable boxes: matched at t = 0.5 alone
    out['iou_half'] = (case([[0, 0, 0, 2, 1, 1, .9]], [[[0, 0, 2, 2, 1, 1]]], 2, exact=True),
                       dict(AP=.1, AP50=1, AP75=0, APs=.1, APm=-1, APl=-1, AR1=.1, AR10=.1, AR100=.1, ARs=.1, ARm=-1, ARl=-1))
    # a crowd region (0, 0, 100, 100) holding two detections: both matched and ignored.  The counted gt (20, 20, 60, 60) inside it is still
    # preferred by the detection on it, although that detection's crowd IoU (1.0) is the larger one: the break rule.
    out['crowd'] = (case([[0, 70, 70, 90, 90, 1, .9], [0, 5, 5, 15, 15, 1, .8], [0, 20, 20, 60, 59, 1, .7]],
                         [[[0, 0, 100, 100, 1, 1, 1], [20, 20, 60, 60, 1, 1, 0]]], 2),
                    dict(AP=1, AP50=1, AP75=1, APs=-1, APm=1, APl=-1, AR1=0, AR10=1, AR100=1, ARs=-1, ARm=1, ARl=-1))
    # two gts with IoU exactly 0.5 against the first detection: it takes the LATER one, which leaves the earlier one to the second detection.
    # t = 0.5: both hit.  Above: a false positive, then a hit on one of two gts -- precision 0.5 up to recall 0.5 (51 of the 101 points).
    out['equal_iou'] = (case([[0, 0, 0, 20, 10, 1, .9], [0, 0, 0, 10, 10, 1, .8]], [[[0, 0, 10, 10, 1, 1], [10, 0, 20, 10, 1, 1]]], 2, exact=True),
                        dict(AP=(1 + 9 * 25.5 / 101) / 10, AP50=1, AP75=25.5 / 101, APs=(1 + 9 * 25.5 / 101) / 10, APm=-1, APl=-1, AR1=.05, AR10=.55, AR100=.55,
                             ARs=.55, ARm=-1, ARl=-1))
    # 101 detections in one group, only the lowest-scored one on the gt: rank 100 is past every max_dets
    rows = [[0, 200 + i, 200, 230 + i, 230, 1, .99 - .005 * i] for i in range(100)] + [[0, 0, 0, 50, 50, 1, .01]]
    out['cap_101'] = (case(rows, [[[0, 0, 50, 50, 1, 1]]], 2), dict(AP=0, AP50=0, AP75=0, APs=-1, APm=0, APl=-1, AR1=0, AR10=0, AR100=0, ARs=-1, ARm=0, ARl=-1))
    # a 32 x 32 box: area 1024 lies in the small AND the medium range (both ends inclusive)
    out['area_1024'] = (case([[0, 0, 0, 32, 32, 1, .9]], [[[0, 0, 32, 32, 1, 1]]], 2),
                        dict(AP=1, AP50=1, AP75=1, APs=1, APm=1, APl=-1, AR1=1, AR10=1, AR100=1, ARs=1, ARm=1, ARl=-1))
    # an unmatched small detection ahead of the hit on a large gt: a false positive for 'all', ignored for 'large'
    out['unmatched_outside'] = (case([[0, 200, 200, 210, 210, 1, .9], [0, 0, 0, 100, 100, 1, .8]], [[[0, 0, 100, 100, 1, 1]]], 2),
                                dict(AP=.5, AP50=.5, AP75=.5, APs=-1, APm=-1, APl=1, AR1=0, AR10=1, AR100=1, ARs=-1, ARm=-1, ARl=1))
    # equal scores across two images resolve by image, then row: the false positive of image 0 (row 1) comes before the hit of image 1 (row 0)
    out['tie_images'] = (case([[1, 0, 0, 100, 100, 1, .8], [0, 0, 0, 100, 100, 1, .8]], [np.zeros((0, 6)), [[0, 0, 100, 100, 1, 1]]], 2),
                         dict(AP=.5, AP50=.5, AP75=.5, APs=-1, APm=-1, APl=.5, AR1=1, AR10=1, AR100=1, ARs=-1, ARm=-1, ARl=1))
    # the annotation's area moves a 100 x 100 box into the small bin
    out['gt_area'] = (case([[0, 0, 0, 100, 100, 1, .9]], [[[0, 0, 100, 100, 1, 1]]], 2, gt_areas=[np.array([500.0])]),
                      dict(AP=1, AP50=1, AP75=1, APs=1, APm=-1, APl=-1, AR1=1, AR10=1, AR100=1, ARs=1, ARm=-1, ARl=-1))
    # normalised boxes: area 0.04 x 512 x 512 = 10485.76 is large
    out['area_scale'] = (case([[0, .1, .1, .3, .3, 1, .9]], [[[.1, .1, .3, .3, 1, 1]]], 2, image_area_scale=np.array([512.0 * 512.0])),
                         dict(AP=1, AP50=1, AP75=1, APs=-1, APm=-1, APl=1, AR1=1, AR10=1, AR100=1, ARs=-1, ARm=-1, ARl=1))
    return out


# ---- random cases -----------------------------------------------------------------------------------------------------------------------
def random_case(seed, num_classes, with_crowd=True, areas=False, tables=None, **kw):
    """make_map_case with column 6 as the crowd flag; ``areas``: generated gt_areas (a mask covers 50-100 % of its box) and per-image scales.
    Redrawn from seed + 1000, seed + 2000, ... until the builder's condition holds."""
    for attempt in range(20):
        pred, gts = syn.make_map_case(seed=seed + 1000 * attempt, num_classes=num_classes, with_difficult=with_crowd, **kw)
        extra = dict(tables or {})
        if areas:
            rng = np.random.default_rng(seed + 7)
            extra['gt_areas'] = [((g[:, 2].astype(np.float64) - g[:, 0]) * (g[:, 3].astype(np.float64) - g[:, 1])) * rng.uniform(.5, 1, len(g)) for g in gts]
            extra['image_area_scale'] = rng.uniform(.5, 2.0, len(gts))
        c = case(pred, gts, num_classes, **extra)
        if off_thresholds(c):
            return c
    raise AssertionError('no draw off the thresholds in 20 attempts')


RANDOM_CASES = {
    'small_crowd': dict(seed=11, num_images=12, num_classes=6, areas=True),
    'many_classes': dict(seed=13, num_images=40, num_classes=21, max_gt=8, noise_fp=4),
    'no_flag_column': dict(seed=15, num_images=25, num_classes=81, with_crowd=False, max_gt=5, empty_images=False),
    'past_a_tile': dict(seed=101, num_images=400, num_classes=9, max_gt=9, noise_fp=16, difficult_p=0.1, areas=True),
    'score_ties': dict(seed=104, num_images=60, num_classes=5, unique_scores=False, dup=0.6, noise_fp=5),
}

TABLE_CASES = {
    'one_of_each': dict(iou_thrs=np.array([0.5]), rec_thrs=np.array([0.5]), area_rngs=np.array([[0.0, 1e10]]), max_dets=np.array([100], np.int32)),
    'all_64_lanes': dict(iou_thrs=np.linspace(.2, .95, 16)),
    'max_dets_3': dict(max_dets=np.array([3], np.int32)),
    'unsorted_recall': dict(rec_thrs=np.array([.9, 0.0, .3, 1.0, 1.5, -0.5, .3])),
    'four_max_dets': dict(max_dets=np.array([1, 2, 5, 100], np.int32)),
}


# ---- edge shapes ------------------------------------------------------------------------------------------------------------------------
def group_case(seed, n_det, n_gt):
    """One (image, class) group of n_det detections against n_gt gts of its class (every fifth a crowd region, sizes across the three
    bins), beside a second class and a second image; image 2 has ground truth and no detection."""
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000 * attempt)
        xy = rng.uniform(0, 400, (n_gt, 2))
        wh = np.exp(rng.uniform(np.log(12), np.log(160), (n_gt, 2)))
        g0 = np.concatenate([xy, xy + wh, np.full((n_gt, 1), 1.0), np.ones((n_gt, 1)), (np.arange(n_gt) % 5 == 3).astype(np.float64)[:, None]], 1)
        other = np.array([[10, 10, 60, 60, 2, 1, 0], [100, 100, 130, 120, 2, 1, 1]], np.float64)
        rows = []
        for d in range(n_det):
            if n_gt and rng.random() < 0.7:
                k = int(rng.integers(n_gt))
                b = g0[k, :4] + rng.normal(0, 0.08, 4) * np.tile(wh[k], 2)
            else:
                p = rng.uniform(0, 400, 2)
                b = np.concatenate([p, p + np.exp(rng.uniform(np.log(12), np.log(160), 2))])
            rows.append(np.concatenate([[0], b, [1], [rng.uniform(0.05, 1.0)]]))
        rows.append(np.array([0, 12, 10, 60, 58, 2, .5]))
        rows.append(np.array([1, 12, 10, 60, 58, 2, .4]))
        pred = np.stack(rows).astype(np.float32)
        assert np.unique(pred[:, 6]).size == pred.shape[0]
        pred = pred[rng.permutation(pred.shape[0])]
        c = case(pred, [np.concatenate([g0, other]), other[:1], other], 3)
        if off_thresholds(c):
            return c
    raise AssertionError('no draw off the thresholds in 20 attempts')


GROUP_SHAPES = [(1, 0), (100, 1), (101, 64), (257, 65), (40, 130)]


def special_cases():
    base = random_case(seed=21, num_classes=5, num_images=6)
    pred, gts = base['pred'], base['gts']
    out = {}
    out['no_predictions'] = case(np.zeros((0, 7)), gts, 5)
    out['no_ground_truth'] = case(pred, [np.zeros((0, 7), np.float32) for _ in gts], 5)
    out['no_images'] = case(pred, [], 5)
    extra = np.array([[99, 10, 10, 50, 50, 1, .95], [-3, 10, 10, 50, 50, 1, .94], [99, 12, 10, 50, 50, 1, .93], [2, 10, 10, 50, 50, 7, .92],
                      [2, 10, 10, 50, 50, -1, .91], [0, 10, 10, 20, 20, 1, .90]], np.float32)
    out['foreign_ids'] = case(np.concatenate([extra[:3], pred, extra[3:]]), gts, 5)
    return out


_CASES = {}


def gpu_cases():
    """name -> case: everything tests/test_coco_eval_gpu.py runs against the reference (built once)."""
    if not _CASES:
        for name, (c, _) in hand_cases().items():
            _CASES['hand_' + name] = c
        for name, kw in RANDOM_CASES.items():
            _CASES['random_' + name] = random_case(**kw)
        for name, tables in TABLE_CASES.items():
            _CASES['tables_' + name] = random_case(seed=31, num_classes=6, num_images=16, dup=0.6, noise_fp=4, areas=True, tables=tables)
        for n_det, n_gt in GROUP_SHAPES:
            _CASES[f'group_{n_det}_dets_{n_gt}_gts'] = group_case(500 + n_det, n_det, n_gt)
        for name, c in special_cases().items():
            _CASES['special_' + name] = c
    return _CASES
