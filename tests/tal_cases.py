"""Task Alignment Learning (TaskAlignedAssigner, ssdk_encode_ground_truth_tal): the numpy restatement of its eight rules -- the executable
form of the specification in include/ssdk.h, the reference has no such assigner -- and the cases ``tests/test_tal*.py`` and
``tests/tal_graph_worker.py`` share.  ``tal_image_np(..., dtype)`` evaluates the rule in fp32, one operation at a time as the library
does, or in fp64 from the same fp32 inputs.  expf, the sigmoid and __powf are not bit-equal between the device and numpy, so a generated
case is used only when every decision in it has a margin (``margins``): that is a condition on the inputs, not a tolerance on the
result; a case that misses it gets another seed.  The inside test compares inputs and is exact."""
import functools
import os

import numpy as np

import atss_cases as ac

GOLDEN = ac.GOLDEN
NOT_MATCHED = -2
F = np.float32
MIN_RANK_GAP = 2e-4      # (a) relative gap between the metrics at rank topk and topk + 1 of a box with more than topk inside anchors
MIN_U_GAP = 2e-5         # (b) gap between the two largest u at an anchor that several boxes claim
TINY = 1e-20             # (c) no metric among a box's first topk + 1 lies in (0, TINY)
XY_SCALE, WH_SCALE = 10.0, 5.0


class Coder(object):
    """What the assigner reads of a box coder."""
    def __init__(self, xy_scale=XY_SCALE, wh_scale=WH_SCALE):
        self.xy_scale, self.wh_scale = xy_scale, wh_scale


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def _clamp0(v):
    return np.where(v < 0, v.dtype.type(0), v)


def _area(x1, y1, x2, y2):
    return _clamp0(x2 - x1) * _clamp0(y2 - y1)


def decode_corners_np(locs, anchors, xy_scale, wh_scale, dtype=F):
    """Rule 1: corners [n, 4] of the decoded predictions, op for op the library's decode_corners."""
    t, p = np.asarray(locs, F).astype(dtype), np.asarray(anchors, F).astype(dtype)
    xy, wh, two = dtype(xy_scale), dtype(wh_scale), dtype(2)
    cx, cy = p[:, 0] + p[:, 2] * t[:, 0] / xy, p[:, 1] + p[:, 3] * t[:, 1] / xy
    w, h = p[:, 2] * np.exp(t[:, 2] / wh), p[:, 3] * np.exp(t[:, 3] / wh)
    return np.stack([cx - w / two, cy - h / two, cx + w / two, cy + h / two], axis=1)


def quality_np(P, box):
    """Rule 2: the plain IoU of corner boxes P [n, 4] with one corner box, in [0, 1], 0 where undefined (the library's box_quality)."""
    dt = P.dtype.type
    b = np.asarray(box, F).astype(P.dtype)
    with np.errstate(all='ignore'):
        inter = _area(np.maximum(P[:, 0], b[0]), np.maximum(P[:, 1], b[1]), np.minimum(P[:, 2], b[2]), np.minimum(P[:, 3], b[3]))
        uni = _area(P[:, 0], P[:, 1], P[:, 2], P[:, 3]) + _area(b[0:1], b[1:2], b[2:3], b[3:4]) - inter
        q = inter / uni
        bad = ~(uni > 0) | ~np.isfinite(q)
        return np.where(bad, dt(0), np.minimum(np.maximum(q, dt(0)), dt(1))).astype(P.dtype)


def _pow(x, e, six):
    """Rule 5: 0, 1, 2 (and 6 for u) are multiplies."""
    dt = x.dtype.type
    if e == 0.0:
        return np.ones_like(x)
    if e == 1.0:
        return x
    if e == 2.0:
        return x * x
    if six and e == 6.0:
        x2 = x * x
        return x2 * x2 * x2
    return np.power(x, dt(e)).astype(x.dtype)


def inside_np(box, anchors):
    """Rule 4, on the fp32 inputs: exact."""
    a = np.asarray(anchors, F)
    x1, y1, x2, y2 = np.asarray(box, F)[:4]
    return (x1 < a[:, 0]) & (a[:, 0] < x2) & (y1 < a[:, 1]) & (a[:, 1] < y2)


def box_metrics_np(box, anchors, scores, locs, xy_scale, wh_scale, alpha, beta, dtype=F):
    """(inside anchors ascending, their m, their u) of one box -- rules 1 to 5."""
    ins = np.nonzero(inside_np(box, anchors))[0]
    P = decode_corners_np(locs[ins], anchors[ins], xy_scale, wh_scale, dtype)
    u = quality_np(P, box[:4])
    C = scores.shape[1]
    cls = box[4]
    if cls >= 1 and cls <= C:
        x = np.asarray(scores, F)[ins, int(cls) - 1].astype(dtype)
        with np.errstate(over='ignore'):
            s = dtype(1) / (dtype(1) + np.exp(-x))
    else:
        s = np.zeros(len(ins), dtype)
    with np.errstate(all='ignore'):
        m = _pow(s, alpha, False) * _pow(u, beta, True)
    return ins, m.astype(dtype), u


def _ranked(ins, m):
    """Rule 6's order: largest m first, a NaN below every number, ties to the lower anchor (``ins`` ascends, the sort is stable)."""
    key = np.where(np.isnan(m), -np.inf, m.astype(np.float64))
    return np.argsort(-key, kind='stable')


def tal_image_np(gt, anchors, scores, locs, topk=13, alpha=1.0, beta=6.0, xy_scale=XY_SCALE, wh_scale=WH_SCALE, dtype=F, info=None):
    """One image: (box_idx int32 [A], column 5 of the target as ``dtype`` [A]).  ``info`` (a dict) receives the margins of the decisions:
    'rank_gap' the smallest (a), 'u_gap' the smallest (b), 'tiny' the count of (c), and per box the first topk + 1 metrics."""
    anchors = np.asarray(anchors, F)
    scores = np.asarray(scores, F).reshape(len(anchors), -1)
    locs = np.asarray(locs, F).reshape(len(anchors), 4)
    gt = np.asarray(gt, F).reshape(-1, 6)
    A = len(anchors)
    box_idx = np.full(A, NOT_MATCHED, np.int32)
    best_u = np.zeros(A, dtype)
    second_u, second_g = np.full(A, -np.inf), np.full(A, -1, np.int32)
    kept_m = np.zeros(A, dtype)
    claims = np.zeros(A, np.int32)
    rank_gap, tiny, heads = np.inf, 0, []
    for g, box in enumerate(gt):
        ins, m, u = box_metrics_np(box, anchors, scores, locs, xy_scale, wh_scale, alpha, beta, dtype)
        order = _ranked(ins, m)
        head = m[order[:topk + 1]].astype(np.float64)
        heads.append((ins[order[:topk + 1]], head))
        tiny += int(((head > 0) & (head < TINY)).sum())
        if len(ins) > topk:
            hi, lo = head[topk - 1], head[topk]
            if not (hi == 0 and lo == 0):
                rank_gap = min(rank_gap, (hi - lo) / hi if hi > 0 else 0.0)
        for j in order[:topk]:                                                            # rule 7: strict >, boxes ascending
            a = ins[j]
            claims[a] += 1
            if box_idx[a] < 0 or u[j] > best_u[a]:
                if box_idx[a] >= 0 and float(best_u[a]) > second_u[a]:
                    second_u[a], second_g[a] = float(best_u[a]), box_idx[a]
                box_idx[a], best_u[a], kept_m[a] = g, u[j], m[j]
            elif float(u[j]) > second_u[a]:
                second_u[a], second_g[a] = float(u[j]), g
    col5 = np.ones(A, dtype)
    one_e9 = dtype(F(1e-9))
    for g, box in enumerate(gt):                                                          # rule 8
        kept = np.nonzero(box_idx == g)[0]
        if not len(kept):
            continue
        m, u = kept_m[kept], best_u[kept]
        m_max = np.max(np.where(np.isnan(m), dtype(0), m))
        with np.errstate(all='ignore'):
            col5[kept] = dtype(box[5]) * (m / (m_max + one_e9) * np.max(u))
    if info is not None:
        multi = claims > 1
        info.update(rank_gap=rank_gap, tiny=tiny, heads=heads, contested=int(multi.sum()), best_u=best_u.astype(np.float64), second_u=second_u,
                    second_g=second_g, best_g=box_idx.copy(), multi=multi)
    return box_idx, col5


def tal_np(gt_list, anchors, scores, locs, dtype=F, info=None, **kw):
    """(box_idx int32 [B, A], column 5 [B, A]); ``info`` collects the per-image margins."""
    out = []
    for i, gt in enumerate(gt_list):
        one = {} if info is not None else None
        out.append(tal_image_np(gt, anchors, scores[i], locs[i], dtype=dtype, info=one, **kw))
        if info is not None:
            info.setdefault('images', []).append(one)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def target_np(box_idx, col5, gt_list):
    """target [B, A, 6] in col5's dtype: a matched anchor copies the box's columns 0..4, every other row is (0, 0, 0, 0, 0, 1)."""
    b, a = box_idx.shape
    target = np.zeros((b, a, 6), col5.dtype)
    for i, gt in enumerate(gt_list):
        pos = box_idx[i] >= 0
        target[i, pos, :5] = np.asarray(gt, F).reshape(-1, 6)[box_idx[i][pos], :5]
    target[..., 5] = col5
    return target


def margins(gt_list, anchors, scores, locs, **kw):
    """Evaluates a case in fp64 and in fp32 and returns its figures: 'rank_gap' (a), 'u_gap' (b), 'tiny' (c), 'm_dev' the largest relative
    |fp32 - fp64| over the boxes' first topk + 1 metrics, 'u_dev' the largest |fp32 - fp64| of u at a contested anchor, 'col5_dev' the largest
    |fp32 - fp64| of column 5, and the two restatements' results."""
    i64, i32 = {}, {}
    idx64, c64 = tal_np(gt_list, anchors, scores, locs, dtype=np.float64, info=i64, **kw)
    idx32, c32 = tal_np(gt_list, anchors, scores, locs, dtype=F, info=i32, **kw)
    rank_gap = min(im['rank_gap'] for im in i64['images'])
    tiny = sum(im['tiny'] for im in i64['images'])
    u_gap, u_dev, m_dev = np.inf, 0.0, 0.0
    for gt, a, b in zip(gt_list, i64['images'], i32['images']):
        multi = a['multi']
        if multi.any():
            gap = a['best_u'][multi] - a['second_u'][multi]
            rows = np.asarray(gt, F).reshape(-1, 6)[:, :4]
            same = (rows[a['best_g'][multi]].view(np.uint32) == rows[a['second_g'][multi]].view(np.uint32)).all(axis=1)
            gap = np.where(same & (gap == 0), np.inf, gap)   # bit-identical corners: the same u on every side, the box index decides
            u_gap = min(u_gap, float(gap.min()))
            u_dev = max(u_dev, float(np.abs(a['best_u'][multi] - b['best_u'][multi]).max()))
        for (an64, h64), (an32, h32) in zip(a['heads'], b['heads']):
            pos = h64 > 0
            if pos.any() and np.array_equal(an64, an32):
                m_dev = max(m_dev, float(np.max(np.abs(h32[pos] - h64[pos]) / h64[pos])))
    return dict(rank_gap=rank_gap, u_gap=u_gap, tiny=tiny, m_dev=m_dev, u_dev=u_dev, col5_dev=float(np.nanmax(np.abs(c32.astype(np.float64) - c64))),
                idx64=idx64, col64=c64, idx32=idx32, col32=c32)


def assert_margins(fig):
    assert fig['rank_gap'] >= MIN_RANK_GAP, f"(a) rank gap {fig['rank_gap']:.3g} < {MIN_RANK_GAP}: take another seed"
    assert fig['u_gap'] >= MIN_U_GAP, f"(b) u gap {fig['u_gap']:.3g} < {MIN_U_GAP}: take another seed"
    assert fig['tiny'] == 0, f"(c) {fig['tiny']} metrics in (0, {TINY}): take another seed"
    assert np.array_equal(fig['idx64'], fig['idx32']), 'the fp32 and fp64 restatements decide differently'
    if np.isfinite(fig['rank_gap']):
        assert fig['m_dev'] <= fig['rank_gap'] / 10, (fig['m_dev'], fig['rank_gap'])
    if np.isfinite(fig['u_gap']):
        assert fig['u_dev'] <= fig['u_gap'] / 10, (fig['u_dev'], fig['u_gap'])


# ---- the hand-worked grid (tests/atss_cases.py: 42 anchors, (cx, cy, w, h), levels 4x4x2 / 2x2x2 / 1x1x2 on 64 pixels) -----------------------
GRID_TOPK = 3
GRID_C = 3
FAR = 100.0     # an encoded tx that moves every predicted box 10 widths to the right: off the image, u = 0


def _box(x1, y1, x2, y2, cls, score=1.0):
    return [x1, y1, x2, y2, cls, score]


# name -> (boxes, tx of every anchor's loc, {anchor: (box, t)} worked out by hand -- see tests/test_tal.py for the working).  Every logit is 0
# (s = 0.5 exactly) and every other loc entry is 0 (the predicted box is the anchor), so the grid's arithmetic is exact in fp32.
GRID_CASES = {
    # the box IS anchor 32 (level 1, cell (0, 0)): ten anchors inside; u = 1, 704/1288, then the four 16x16 anchors tie at 1/4: the lowest, 0
    'box_on_one_cell': ([_box(0, 0, 32, 32, 1)], 0.0, {32: (0, 1.0), 33: (0, (704 / 1288) ** 6), 0: (0, 0.25 ** 6)}),
    # only the two anchors of level-0 cell (1, 1) have their centre inside: fewer than topk
    'fewer_inside_than_topk': ([_box(16, 16, 32, 32, 2)], 0.0, {10: (0, 1.0), 11: (0, (176 / 322) ** 6)}),
    # a sliver between the columns of centres
    'no_inside_anchor': ([_box(33, 1, 37, 63, 3)], 0.0, {}),
    # two identical boxes: every u ties, the lower index keeps every anchor
    'identical_boxes': ([_box(0, 0, 32, 32, 1), _box(0, 0, 32, 32, 1)], 0.0, {32: (0, 1.0), 33: (0, (704 / 1288) ** 6), 0: (0, 0.25 ** 6)}),
    # anchors 10 and 11 are the candidates of both boxes.  Box 0 has the larger m (box 1's class is outside 1..C: its m is 0), box 1 the
    # larger u (1 against 196/256, 176/322 against 154/284): box 1 wins both, and its t is 0
    'larger_u_beats_larger_m': ([_box(17, 17, 31, 31, 1), _box(16, 16, 32, 32, 9)], 0.0, {10: (1, 0.0), 11: (1, 0.0)}),
    # every prediction is off the image: u = 0, all ten metrics tie at 0 and the lowest indices are positives with t = 0
    'all_u_zero': ([_box(0, 0, 32, 32, 2)], FAR, {0: (0, 0.0), 1: (0, 0.0), 2: (0, 0.0)}),
    # x1 = 24 and x2 = 40 pass through level 0's centres, y2 = 32 through the last level's: strictly inside fails everywhere
    'edge_through_centres': ([_box(24, 16, 40, 32, 1)], 0.0, {}),
    'empty_image': ([], 0.0, {}),
    # s = 0: all metrics tie at 0, the lowest indices are positives with t = 0
    'class_outside_1_to_C': ([_box(0, 0, 32, 32, 5, 0.5)], 0.0, {0: (0, 0.0), 1: (0, 0.0), 2: (0, 0.0)}),
}


def grid_anchors():
    return ac.grid_anchors()


def grid_gt(name):
    return np.array(GRID_CASES[name][0], F).reshape(-1, 6)


def grid_prediction(name):
    """(scores [42, GRID_C], locs [42, 4]) of a grid case."""
    locs = np.zeros((42, 4), F)
    locs[:, 0] = GRID_CASES[name][1]
    return np.zeros((42, GRID_C), F), locs


def grid_expected(name):
    """(box_idx int32 [42], column 5 fp64 [42]) worked out by hand."""
    idx, col5 = np.full(42, NOT_MATCHED, np.int32), np.ones(42, np.float64)
    gt = grid_gt(name)
    for a, (g, t) in GRID_CASES[name][2].items():
        idx[a], col5[a] = g, float(gt[g, 5]) * t
    return idx, col5


# ---- generated cases -----------------------------------------------------------------------------------------------------------------------
# name -> (config, batch, C, make_ground_truth keywords, emptied image or None, keep (boxes kept in the images after the first, or None),
#          keywords of the rule, seed of the prediction, gt scores below 1 (mixup))
GENERATED = {
    'mb2_one_empty': ('ssd_mb2_voc', 3, 20, dict(seed=1), 1, None, dict(topk=13), 11, False),
    'mb2_g32': ('ssd_mb2_voc', 3, 20, dict(seed=1, fixed_g=32), None, None, dict(topk=13), 12, False),
    'mb2_g140_topk5': ('ssd_mb2_voc', 3, 20, dict(seed=2, fixed_g=140), None, 6, dict(topk=5), 13, False),   # past the 128-box LDS chunk
    'mb2_topk32': ('ssd_mb2_voc', 3, 20, dict(seed=3), None, None, dict(topk=32), 14, False),
    'mb2_one_class': ('ssd_mb2_voc', 3, 1, dict(seed=4), None, None, dict(topk=13), 15, False),
    'mb2_powf': ('ssd_mb2_voc', 3, 20, dict(seed=5), None, None, dict(topk=13, alpha=0.5, beta=2.5), 16, False),   # the __powf path
    'mb2_mixup_scores': ('ssd_mb2_voc', 3, 20, dict(seed=6), None, None, dict(topk=13), 17, True),
    'retina_c80': ('retina_rn50_500_coco', 2, 80, dict(seed=1, fixed_g=32), None, None, dict(topk=13), 18, False),   # 47 961 anchors
}


def make_prediction(batch, num_anchors, C, seed):
    """Logits 2 * N(0, 1) - 2 [B, A * C] and locs N(0, 1) * (1.5, 1.5, 1, 1) [B, A * 4], fp32, from a fixed seed."""
    rng = np.random.default_rng(seed)
    scores = (2.0 * rng.standard_normal((batch, num_anchors, C), dtype=F) - 2.0).astype(F)
    locs = (rng.standard_normal((batch, num_anchors, 4), dtype=F) * np.array([1.5, 1.5, 1.0, 1.0], F)).astype(F)
    return scores.reshape(batch, -1), locs.reshape(batch, -1)


def build_case(config, batch, C, gt_kw, emptied, keep, rule_kw, pred_seed, mixup):
    from single_shot_detection_amd import synthetic as syn
    cfg = syn.CONFIGS[config]
    gt = syn.make_ground_truth(batch, cfg['size'], C + 1, **gt_kw)          # classes 1..C
    if keep is not None:
        gt = [g if i == 0 else g[:keep] for i, g in enumerate(gt)]
    if emptied is not None:
        gt[emptied] = np.zeros((0, 6), F)
    if mixup:
        rng = np.random.default_rng(pred_seed + 1000)
        for g in gt:
            g[:, 5] = rng.uniform(0.3, 1.0, len(g)).astype(F)
    anchors = np.load(os.path.join(GOLDEN, f'{config}.npz'))['anchors'].astype(F)
    scores, locs = make_prediction(batch, len(anchors), C, pred_seed)
    return gt, anchors, scores, locs, dict(rule_kw)


@functools.lru_cache(maxsize=None)
def generated(name):
    """(gt list, anchors [A, 4], scores [B, A * C], locs [B, A * 4], rule keywords, the figures of ``margins``) -- computed once, margins
    asserted."""
    gt, anchors, scores, locs, kw = build_case(*GENERATED[name])
    fig = margins(gt, anchors, scores.reshape(len(gt), len(anchors), -1), locs.reshape(len(gt), len(anchors), 4), **kw)
    assert_margins(fig)
    return gt, anchors, scores, locs, kw, fig


SWEEP_THREADS = 1024     # kTalThreads / kSimotaThreads: a sweep thread owns the anchors congruent to it mod 1 024


def three_anchors_of_one_thread(C, seed, logit, shrink=4):
    """(gt list of one image, anchors [2 503, 4], scores [1, A, C], locs [1, A, 4]): random anchors and predictions, except that anchors 5,
    1 029 and 2 053 -- 1 024 apart, so ONE sweep thread owns all three -- sit on the first box, predict themselves (loc 0: u = 1, then
    smaller by ``shrink`` pixels a side each: about 0.86 and 0.73 at 4) and carry ``logit`` for the box's class.  On the model of ``atss_cases.one_thread_owns_three_candidates``."""
    rng = np.random.default_rng(seed)
    n = 2503
    anchors = np.concatenate([rng.uniform(0, 300, (n, 2)), rng.uniform(20, 120, (n, 2))], axis=1).astype(F)
    gt = [np.array([_box(100, 100, 160, 150, 2), _box(30, 200, 90, 260, 3)], F)]
    scores, locs = make_prediction(1, n, C, seed + 1)
    scores, locs = scores.reshape(1, n, C), locs.reshape(1, n, 4)
    for j, a in enumerate((5, 1029, 2053)):
        anchors[a] = (130 + j, 125 - j, 60 - shrink * j, 50 - shrink * j)
        locs[0, a] = 0
        scores[0, a] = logit
    return gt, anchors, scores, locs


@functools.lru_cache(maxsize=None)
def one_thread_owns_three_candidates():
    """The first box's three best anchors are 5, 1 029 and 2 053: the sweep thread that owns them keeps two keys in registers and finds the
    third only by re-reading its anchors, and with topk = 4 that key is popped and the box's cutoff lies behind it.  Same tuple as
    ``generated``; the congruence and the margins are asserted here, on the CPU."""
    gt, anchors, scores, locs = three_anchors_of_one_thread(4, 41, (-2.0, 3.0, -2.0, -2.0))
    kw = dict(topk=4)
    ins, m, _ = box_metrics_np(gt[0][0], anchors, scores[0], locs[0], XY_SCALE, WH_SCALE, 1.0, 6.0)
    best = ins[_ranked(ins, m)[:3]]
    assert best.tolist() == [5, 1029, 2053] and len(set(best % SWEEP_THREADS)) == 1 and len(ins) > kw['topk']
    fig = margins(gt, anchors, scores, locs, **kw)
    assert_margins(fig)
    return gt, anchors, scores.reshape(1, -1), locs.reshape(1, -1), kw, fig
