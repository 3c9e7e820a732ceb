"""Case builders for the augmentation tests (test_augment.py on the CPU, test_augment_gpu.py on the device)."""
import numpy as np

import augment_reference as R

F32 = np.float32

SSD_AUGMENTATIONS = [
    {'name': 'RandomAdjustHueSaturation', 'args': {'max_hue_delta': .1, 'saturation_delta_range': (.5, 1.5)}},
    {'name': 'ToFloat'},
    {'name': 'RandomAdjustBrightness', 'args': {'max_brightness_delta': .15}},
    {'name': 'RandomAdjustContrast', 'args': {'contrast_delta_range': (.5, 1.5)}},
    {'name': 'RandomExpand', 'args': {'aspect_ratio_range': (0.5, 2.0), 'area_range': (1.0, 16.0)}},
    {'name': 'OneOf', 'args': {'transforms': [{'name': 'Identity'}] + [{'name': 'RandomCrop', 'args': {'min_iou': v}} for v in (.0, .1, .3, .5, .7, .9)]}},
    {'name': 'RandomHorizontalFlip'},
]
SSD_PREPROCESSING = [
    {'name': 'ToFloatTensor', 'args': {'normalize': True}},
    {'name': 'Normalize', 'args': {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}},
]


def rows(boxes, classes=None, width=6):
    """[n, 4] corners -> [n, width] rows: class, score 1, then column c = 100 * c + row index (so a row that travels is recognised)"""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    out = np.zeros((len(b), width), F32)
    out[:, :4] = b
    if width > 4:
        out[:, 4] = np.arange(1, len(b) + 1) if classes is None else classes
    if width > 5:
        out[:, 5] = 1.0
    for c in range(6, width):
        out[:, c] = 100 * c + np.arange(len(b))
    return out


def box_cases():
    """name -> dict(size=(H, W), target, p, candidates, out_size=(w, h), attempt, boxes): `attempt` and `boxes` are worked out by hand."""
    C = {}
    # region [8, 8, 23, 23]; box A's centre is (23, 12): ON the region's edge, so A goes although half of it is inside; B stays, shifted by 8
    C['centre_on_edge'] = dict(size=(32, 32), target=rows([[20, 10, 26, 14], [10, 10, 14, 14]]), p=R.params(R.CROP, min_iou=0.0, min_objects_kept=1),
                               candidates=[[8, 8, 16, 16]], out_size=(16, 16), attempt=0, boxes=[[2, 2, 6, 6]], classes=[2])
    # region [0, 0, 4, 15]: the 8 x 8 box is cut to 4 x 8, IoU = 32 / 64 = 0.5 exactly = min_iou: rejected, the test is strict
    C['iou_equals_min_iou'] = dict(size=(16, 16), target=rows([[0, 0, 8, 8]]), p=R.params(R.CROP, min_iou=0.5, min_objects_kept=1),
                                   candidates=[[0, 0, 5, 16]], out_size=(16, 16), attempt=-1, boxes=[[0, 0, 8, 8]], classes=[1])
    # the box misses the window: the intersection is zeroed, IoU = 0 / 9 = 0, and 0 > 0 is false
    C['min_iou_zero_box_outside'] = dict(size=(16, 16), target=rows([[0, 0, 3, 3]]), p=R.params(R.CROP, min_iou=0.0, min_objects_kept=1),
                                         candidates=[[8, 8, 8, 8]], out_size=(16, 16), attempt=-1, boxes=[[0, 0, 3, 3]], classes=[1])
    # a zero-area input box: its IoU is 0 / 0 = NaN, max is NaN, every window is rejected; the degenerate box is then dropped by the filter
    C['zero_area_box'] = dict(size=(16, 16), target=rows([[2, 2, 2, 6], [4, 4, 12, 12]]), p=R.params(R.CROP, min_iou=0.0, min_objects_kept=1),
                              candidates=[[0, 0, 16, 16], [2, 2, 12, 12]], out_size=(16, 16), attempt=-1, boxes=[[4, 4, 12, 12]], classes=[2])
    # no boxes: the first VALID window (the first candidate is marked larger than the image)
    C['no_boxes'] = dict(size=(16, 16), target=rows(np.zeros((0, 4))), p=R.params(R.CROP, min_iou=0.9, min_objects_kept=1),
                         candidates=[[0, 0, 0, 0], [3, 4, 8, 8]], out_size=(8, 8), attempt=1, boxes=np.zeros((0, 4)), classes=[])
    # fifty windows that all miss the box: the image is left as it is
    C['fifty_rejected'] = dict(size=(64, 64), target=rows([[1, 1, 5, 5]]), p=R.params(R.CROP, min_iou=0.1, min_objects_kept=1),
                               candidates=[[10 + (i % 7), 10 + (i % 5), 20, 20] for i in range(50)], out_size=(64, 64), attempt=-1,
                               boxes=[[1, 1, 5, 5]], classes=[1])
    # min_objects_kept = 2: the first window holds one centre only, the second holds both
    C['min_objects_kept_2'] = dict(size=(32, 32), target=rows([[2, 2, 6, 6], [20, 20, 28, 28]]), p=R.params(R.CROP, min_iou=0.0, min_objects_kept=2),
                                   candidates=[[0, 0, 16, 16], [0, 0, 32, 32]], out_size=(32, 32), attempt=1,
                                   boxes=[[2, 2, 6, 6], [20, 20, 28, 28]], classes=[1, 2])
    # 8 x 8 -> 4 x 4: (7.25, 1, 7.75, 5) * 0.5 = (3.625, .5, 3.875, 2.5), clipped to [0, 3]: x1 = x2 = 3, degenerate, dropped
    C['degenerate_after_clip'] = dict(size=(8, 8), target=rows([[7.25, 1, 7.75, 5], [2, 2, 6, 4]]), p=R.params(0), candidates=[[0, 0, 0, 0]],
                                      out_size=(4, 4), attempt=-2, boxes=[[1, 1, 3, 2]], classes=[2])
    # flips in a 10 x 8 image: x -> 9 - x, y -> 7 - y, corners swapped
    C['hflip_box'] = dict(size=(8, 10), target=rows([[1, 2, 4, 6]]), p=R.params(R.HFLIP), candidates=[[0, 0, 0, 0]], out_size=(10, 8), attempt=-2,
                          boxes=[[5, 2, 8, 6]], classes=[1])
    C['vflip_box'] = dict(size=(8, 10), target=rows([[1, 2, 4, 6]]), p=R.params(R.VFLIP), candidates=[[0, 0, 0, 0]], out_size=(10, 8), attempt=-2,
                          boxes=[[1, 1, 4, 5]], classes=[1])
    # expand: the 4 x 4 image sits at (2, 3) of an 8 x 8 canvas
    C['expand_box'] = dict(size=(4, 4), target=rows([[0, 0, 2, 2]]), p=R.params(R.EXPAND, expand=(8, 8, 2, 3)), candidates=[[0, 0, 0, 0]],
                           out_size=(8, 8), attempt=-2, boxes=[[2, 3, 4, 5]], classes=[1])
    # keep_criterion 'iou': region [0, 0, 15, 15]; A inside (IoU 1) stays; B (12, 12, 20, 20) is cut to 3 x 3 of 8 x 8, IoU 9 / 64 <= 0.5: goes;
    # C (10, 2, 18, 6) is cut to 5 x 4 of 8 x 4, IoU 20 / 32 > 0.5: stays, clipped to (10, 2, 15, 6)
    C['keep_iou'] = dict(size=(32, 32), target=rows([[2, 2, 6, 6], [12, 12, 20, 20], [10, 2, 18, 6]]),
                         p=R.params(R.CROP | R.KEEP_IOU, min_iou=0.5, min_objects_kept=1), candidates=[[0, 0, 16, 16]], out_size=(16, 16), attempt=0,
                         boxes=[[2, 2, 6, 6], [10, 2, 15, 6]], classes=[1, 3])
    return C


def pad_candidates(cands, attempts):
    out = np.zeros((len(cands), attempts, 4), np.int32)
    for i, c in enumerate(cands):
        c = np.asarray(c, np.int32).reshape(-1, 4)[:attempts]
        out[i, :len(c)] = c
    return out


def random_box_batch(seed, B, max_rows, width, attempts, size_range=(20, 90), counts=None):
    """A ragged batch with every flag combination somewhere: -> (targets, sizes, records (list of dicts), candidates [B, attempts, 4])"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, max_rows + 1, B) if counts is None else np.asarray(counts)
    targets, sizes, recs, cands = [], [], [], []
    for b in range(B):
        H, W = (int(v) for v in rng.integers(size_range[0], size_range[1], 2))
        n = int(counts[b])
        x1, y1 = rng.uniform(0, W - 2, n), rng.uniform(0, H - 2, n)
        x2, y2 = x1 + rng.uniform(1, W / 2, n), y1 + rng.uniform(1, H / 2, n)
        t = rows(np.stack([x1, y1, np.minimum(x2, W - 1), np.minimum(y2, H - 1)], axis=1), classes=rng.integers(1, 21, n), width=width)
        if n and rng.random() < 0.5:
            t[:, :4] = np.round(t[:, :4])                   # integer corners: centres on region edges and equal IoUs do occur
        flags = int(rng.integers(0, 2)) * R.EXPAND | int(rng.integers(0, 2)) * R.HFLIP | int(rng.integers(0, 2)) * R.VFLIP
        flags |= (R.CROP if rng.random() < 0.8 else 0) | int(rng.integers(0, 2)) * R.KEEP_IOU
        cw, ch, ex, ey = W, H, 0, 0
        if flags & R.EXPAND:
            cw, ch = W + int(rng.integers(0, 2 * W)), H + int(rng.integers(0, 2 * H))
            ex, ey = int(rng.integers(0, cw - W + 1)), int(rng.integers(0, ch - H + 1))
        c = np.zeros((attempts, 4), np.int64)
        c[:, 2], c[:, 3] = rng.integers(1, cw + 1, attempts), rng.integers(1, ch + 1, attempts)
        c[:, 0], c[:, 1] = rng.integers(0, cw - c[:, 2] + 1), rng.integers(0, ch - c[:, 3] + 1)
        c[rng.random(attempts) < 0.2] = 0                   # candidates marked larger than the image
        recs.append(R.params(flags, expand=(cw, ch, ex, ey) if flags & R.EXPAND else (0, 0, 0, 0),
                             min_iou=float(rng.choice([0.0, 0.1, 0.3, 0.5, 0.7, 0.9])), min_objects_kept=int(rng.integers(0, 3))))
        targets.append(t)
        sizes.append((H, W))
        cands.append(c)
    return targets, sizes, recs, np.asarray(cands, np.int32)


def integer_mean_image(rng, H, W):
    """uint8 [H, W, 3] whose mean over all channels is an INTEGER: the fill is then exact in float32 AND survives the weights .25 / .75 of
    the exact geometry cases without rounding (a general mean has 24 significant bits; three quarters of it need two more)."""
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    flat = img.reshape(-1)
    r = int(flat.astype(np.int64).sum()) % flat.size
    i = 0
    while r:
        d = min(r, int(flat[i]))
        flat[i] -= d
        r -= d
        i += 1
    assert int(img.astype(np.int64).sum()) % img.size == 0
    return img


GEOMETRY_SOURCES = [(1, 1), (3, 5), (37, 53), (64, 48)]      # H, W
GEOMETRY_OUTPUTS = [(16, 16), (20, 12), (21, 13)]            # w, h; 21 is a row length that is no multiple of 4


def geometry_cases(out_size, seed=0):
    """-> [(name, img, p, window)] for one output size: colour off, every scale 1, 2 or 1/2, so every weight is 0, .25, .5, .75 or 1"""
    ow, oh = out_size
    rng = np.random.default_rng(1000 * ow + oh + seed)
    cases = []
    for H, W in GEOMETRY_SOURCES:
        img = integer_mean_image(rng, H, W)
        tag = f'{H}x{W}'
        cases.append((f'identity_{tag}', img, R.params(0), (0, 0, ow, oh)))
        cases.append((f'hflip_{tag}', img, R.params(R.HFLIP), (0, 0, ow, oh)))
        cases.append((f'vflip_{tag}', img, R.params(R.VFLIP), (0, 0, ow, oh)))
        ex, ey = min(3, max(ow - W, 0)), min(2, max(oh - H, 0))
        cases.append((f'expand_canvas_{tag}', img, R.params(R.EXPAND, expand=(ow, oh, ex, ey)), (-ex, -ey, ow, oh)))
        # a crop of an expanded image that straddles the source's edge: fill and source meet inside one bilinear footprint
        cases.append((f'straddle_down2_{tag}', img, R.params(R.EXPAND, expand=(4 * ow, 4 * oh, 5, 3)), (-5, -3, 2 * ow, 2 * oh)))
        cases.append((f'straddle_far_{tag}', img, R.params(R.EXPAND, expand=(4 * ow + W, 4 * oh + H, 5, 3)), (W - ow, H - oh, 2 * ow, 2 * oh)))
        if ow % 2 == 0 and oh % 2 == 0:
            cases.append((f'straddle_up2_{tag}', img, R.params(R.EXPAND, expand=(4 * ow, 4 * oh, 3, 2)), (-3, -2, ow // 2, oh // 2)))
            cases.append((f'inside_up2_{tag}', img, R.params(0), (W // 3, H // 3, ow // 2, oh // 2)))
        cases.append((f'composed_{tag}', img, R.params(R.EXPAND | R.HFLIP | R.VFLIP, expand=(4 * ow + W, 4 * oh + H, 7, 4)), (W // 2 - ow, H // 2 - oh, 2 * ow, oh)))
    return cases


def general_cases(seed=7):
    """-> [(name, img, p, window)]: non-integer scales, every colour step.  All for the output 21 x 13."""
    rng = np.random.default_rng(seed)
    cases = []
    every = R.HUE_SATURATION | R.BRIGHTNESS | R.CONTRAST | R.EXPAND
    for H, W in [(37, 53), (64, 48), (3, 5), (1, 1)]:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        tag = f'{H}x{W}'
        colour = dict(hue_delta=0.07, saturation=1.3, brightness=-21.5, contrast=1.4)
        cases.append((f'all_{tag}', img, R.params(every, expand=(3 * W, 2 * H, W // 2, H // 3), **colour), (-(W // 2), -(H // 3), 3 * W, 2 * H)))
        cases.append((f'all_flipped_crop_{tag}', img, R.params(every | R.HFLIP | R.VFLIP, expand=(3 * W, 2 * H, W, H // 2), hue_delta=-0.1, saturation=0.5,
                                                              brightness=38.25, contrast=0.5), (-(W // 3) - 1, -1, W + 2, H + 1)))
        cases.append((f'hue_only_{tag}', img, R.params(R.HUE_SATURATION, hue_delta=0.1, saturation=1.0), (0, 0, W, H)))
        cases.append((f'saturation_only_{tag}', img, R.params(R.HUE_SATURATION, hue_delta=0.0, saturation=1.5), (0, 0, W, H)))
        cases.append((f'brightness_only_{tag}', img, R.params(R.BRIGHTNESS, brightness=30.0), (0, 0, W, H)))
        cases.append((f'contrast_only_{tag}', img, R.params(R.CONTRAST, contrast=0.75), (0, 0, W, H)))
        cases.append((f'expand_only_{tag}', img, R.params(R.EXPAND, expand=(2 * W + 1, 2 * H + 3, 1, 2)), (-1, -2, 2 * W + 1, 2 * H + 3)))
    return cases


NORMALISE = dict(divide_255=True, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def tolerance(img, p, window, out_size, **norm):
    """-> (want fp64, tol, largest float32-vs-fp64 difference): 8 times the largest difference between the float32 and the fp64 evaluation of
    the restatement on this case, with a floor of one float32 ulp at the output's largest magnitude."""
    want = R.image_reference(img, p, window, out_size, dtype=np.float64, **norm)
    low = R.image_reference(img, p, window, out_size, dtype=np.float32, **norm)
    diff = float(np.abs(low.astype(np.float64) - want).max())
    floor = float(np.spacing(F32(np.abs(want).max())))
    return want, max(8.0 * diff, floor), diff
