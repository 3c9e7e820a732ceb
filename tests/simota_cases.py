"""SimOTA (SimOtaAssigner, ssdk_encode_ground_truth_simota): the numpy restatement of its eight rules -- the executable form of the
specification in include/ssdk.h, the reference has no such assigner -- and the cases ``tests/test_simota*.py`` and
``tests/simota_graph_worker.py`` share.  ``simota_image_np(..., dtype)`` evaluates the rule in fp32, one operation at a time as the library
does, or in fp64 from the same fp32 inputs (the region test compares fp32 inputs and is exact: it is fp32 in both).  __expf and __logf are
not bit-equal between the device and numpy, so a generated case is used only when every decision in it has a margin (``margins``): that
is a condition on the inputs, not a tolerance on the result; a case that misses it gets another seed.

The three margins and where their values come from (``test_simota.py`` prints the figures of every case; DESIGN.md section 32 has the table):
  (a) MIN_RANK_GAP   relative cost gap between rank k_g and k_g + 1 of a box with more than k_g region anchors, when the two are of the
                     same penalty class (a boundary between the classes is decided by the exact region test);
  (b) MIN_CLAIM_GAP  relative cost gap between the two best claims of a contested anchor when they are of the same penalty class, unless
                     the two boxes are bit-identical in columns 0..4 (then the costs are the same bits and the box index decides);
  (c) MIN_SUM_GAP    distance of rule 5's sum from the nearest integer m in 2..q' (crossing 0 or 1 does not move k_g = max((int)sum, 1),
                     and nothing above q' = min(q, n_g) does either).
Over the generated cases the fp32 restatement deviates from the fp64 one by at most 8.2e-7 (relative) on a cost that a decision reads
and by 1.1e-6 on a sum (the figures 'cost_dev' and 'sum_dev'; a cost is a sum of up to 80 softplus terms and one logarithm, each a few
fp32 roundings; a sum adds up to 32 IoUs of a few roundings each).  The thresholds are ten times a bound on those, 3e-6 and 2e-6: 3e-5
for the two cost gaps, 2e-5 for the sum, and ``assert_margins`` checks the factor of ten case by case."""
import functools
import os

import numpy as np

import atss_cases as ac
import tal_cases as tc

GOLDEN = ac.GOLDEN
NOT_MATCHED = -2
F = np.float32
MIN_RANK_GAP = 3e-5
MIN_CLAIM_GAP = 3e-5
MIN_SUM_GAP = 2e-5
XY_SCALE, WH_SCALE = tc.XY_SCALE, tc.WH_SCALE
Coder = tc.Coder


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def softplus_np(x):
    """softplus(x) = max(x, 0) + log(1 + exp(-|x|)) in x's dtype."""
    dt = x.dtype.type
    return np.maximum(x, dt(0)) + np.log(dt(1) + np.exp(-np.abs(x)))


def class_sum_np(scores, dtype=F):
    """Rule 3's S_a of logits [A, C] in the library's order: eight partial sums, partial l over the column quads 4j..4j+3 with
    j = l, l + 8, ... in ascending column order, then the butterfly p[l] += p[l ^ 4], p[l ^ 2], p[l ^ 1]."""
    sp = softplus_np(np.asarray(scores, F).astype(dtype))
    part = np.zeros((sp.shape[0], 8), dtype)
    for c in range(sp.shape[1]):
        part[:, (c // 4) % 8] = part[:, (c // 4) % 8] + sp[:, c]
    for m in (4, 2, 1):
        part = part + part[:, np.arange(8) ^ m]
    assert (part == part[:, :1]).all() or np.isnan(part).any()
    return part[:, 0].copy()


def level_radii_np(level_sizes, level_strides, center_radius):
    """(rx, ry) fp32 [A]: center_radius * (sx, sy) of every anchor's level, one fp32 product each."""
    strides = [(s, s) if np.isscalar(s) else tuple(s) for s in level_strides]
    rx = np.concatenate([np.full(n, F(center_radius) * F(s[0]), F) for n, s in zip(level_sizes, strides)])
    ry = np.concatenate([np.full(n, F(center_radius) * F(s[1]), F) for n, s in zip(level_sizes, strides)])
    return rx, ry


def region_np(box, anchors, rx, ry):
    """Rule 2, on the fp32 inputs: (region [A], penalised [A], in_box [A], in_centre [A])."""
    a = np.asarray(anchors, F)
    x1, y1, x2, y2 = np.asarray(box, F)[:4]
    cx, cy = a[:, 0], a[:, 1]
    with np.errstate(invalid='ignore'):
        in_box = (x1 < cx) & (cx < x2) & (y1 < cy) & (cy < y2)
        gcx, gcy = (x1 + x2) * F(0.5), (y1 + y2) * F(0.5)
        in_centre = (gcx - rx < cx) & (cx < gcx + rx) & (gcy - ry < cy) & (cy < gcy + ry)
    return in_box | in_centre, ~(in_box & in_centre), in_box, in_centre


def box_costs_np(box, anchors, scores, locs, S, rx, ry, iou_weight=3.0, xy_scale=XY_SCALE, wh_scale=WH_SCALE, dtype=F):
    """(region anchors ascending, their penalised flag, their cost, their u) of one box -- rules 1 to 4.  ``S`` = class_sum_np(scores, dtype)."""
    reg, pen, _, _ = region_np(box, anchors, rx, ry)
    ins = np.nonzero(reg)[0]
    P = tc.decode_corners_np(locs[ins], anchors[ins], xy_scale, wh_scale, dtype)
    u = tc.quality_np(P, box[:4])
    C = scores.shape[1]
    cls = box[4]
    c = S[ins]
    if cls >= 1 and cls <= C:
        c = c - np.asarray(scores, F)[ins, int(cls) - 1].astype(dtype)
    with np.errstate(all='ignore'):
        cost = c + dtype(F(iou_weight)) * (-np.log(u + dtype(F(1e-8))))
    return ins, pen[ins], cost.astype(dtype), u


def dynamic_k_np(u, q):
    """Rule 5: (k_g, the fp64 sum, q') from the region anchors' u: the q' = min(q, n) largest, added largest first in fp64."""
    n = len(u)
    qq = min(q, n)
    total = 0.0
    for v in np.sort(np.asarray(u).astype(np.float64))[::-1][:qq]:
        total += float(v)
    return (min(max(int(total), 1), qq) if n else 0), total, qq


def _rank_key(pen, cost):
    """(penalised, cost with NaN above every number) as sortable columns."""
    nan = np.isnan(cost)
    return pen.astype(np.int8), np.where(nan, np.inf, cost.astype(np.float64)), nan.astype(np.int8)


def ranked(ins, pen, cost):
    """Rule 6's order of a box's region anchors: (penalised, cost, anchor index), a NaN cost above every number."""
    p, c, nan = _rank_key(pen, cost)
    return np.lexsort((ins, nan, c, p))


def _rel_gap(lo, hi):
    """(hi - lo) / hi for costs 0 <= lo <= hi; 0 where that is undefined (equal, not finite, not positive)."""
    if not (np.isfinite(lo) and np.isfinite(hi)) or hi <= 0:
        return 0.0
    return (hi - lo) / hi


def simota_image_np(gt, anchors, scores, locs, level_sizes, level_strides, center_radius=2.5, candidate_topk=10, iou_weight=3.0,
                    xy_scale=XY_SCALE, wh_scale=WH_SCALE, dtype=F, info=None):
    """One image: (box_idx int32 [A], dynamic_k int32 [G]).  ``info`` (a dict) receives the margins of the decisions: 'rank_gap' the smallest
    (a), 'claim_gap' the smallest (b), 'sum_gap' the smallest (c), and per box what ``margins`` compares between the two precisions."""
    anchors = np.asarray(anchors, F)
    A = len(anchors)
    scores = np.asarray(scores, F).reshape(A, -1)
    locs = np.asarray(locs, F).reshape(A, 4)
    gt = np.asarray(gt, F).reshape(-1, 6)
    assert sum(level_sizes) == A
    rx, ry = level_radii_np(level_sizes, level_strides, center_radius)
    S = class_sum_np(scores, dtype)
    box_idx = np.full(A, NOT_MATCHED, np.int32)
    dyn = np.zeros(len(gt), np.int32)
    claims = [[] for _ in range(A)]                      # per anchor: (penalised, nan, cost, box)
    rank_gap, sum_gap, boxes = np.inf, np.inf, []
    for g, box in enumerate(gt):
        ins, pen, cost, u = box_costs_np(box, anchors, scores, locs, S, rx, ry, iou_weight, xy_scale, wh_scale, dtype)
        kg, total, qq = dynamic_k_np(u, candidate_topk)
        dyn[g] = kg
        for m in range(2, qq + 1):
            sum_gap = min(sum_gap, abs(total - m))
        order = ranked(ins, pen, cost)
        if len(ins) > kg > 0:
            lo, hi = order[kg - 1], order[kg]
            if pen[lo] == pen[hi]:
                rank_gap = min(rank_gap, _rel_gap(float(cost[lo]), float(cost[hi])))
        boxes.append(dict(anchors=ins, cost=cost.astype(np.float64), total=total, head=order[:kg + 1]))
        p, c, nan = _rank_key(pen, cost)
        for j in order[:kg]:
            claims[ins[j]].append((int(p[j]), int(nan[j]), float(c[j]), g))
    claim_gap, contested = np.inf, 0
    for a, cl in enumerate(claims):                     # rule 7: the smallest (penalised, cost), then the lowest box index
        if not cl:
            continue
        cl.sort()
        box_idx[a] = cl[0][3]
        if len(cl) > 1:
            contested += 1
            (p0, n0, c0, g0), (p1, n1, c1, g1) = cl[0], cl[1]
            if p0 == p1:
                same = np.array_equal(gt[g0, :5].view(np.uint32), gt[g1, :5].view(np.uint32))
                if not (same and c0 == c1 and n0 == n1):
                    claim_gap = min(claim_gap, _rel_gap(c0, c1))
    if info is not None:
        info.update(rank_gap=rank_gap, claim_gap=claim_gap, sum_gap=sum_gap, contested=contested, boxes=boxes)
    return box_idx, dyn


def simota_np(gt_list, anchors, scores, locs, level_sizes, level_strides, dtype=F, info=None, **kw):
    """(box_idx int32 [B, A], list of dynamic_k int32 [G_i]); ``info`` collects the per-image margins."""
    out = []
    for i, gt in enumerate(gt_list):
        one = {} if info is not None else None
        out.append(simota_image_np(gt, anchors, scores[i], locs[i], level_sizes, level_strides, dtype=dtype, info=one, **kw))
        if info is not None:
            info.setdefault('images', []).append(one)
    return np.stack([o[0] for o in out]), [o[1] for o in out]


target_np = ac.target_from_box_idx      # a matched anchor copies the box's six columns, every other row is (0, 0, 0, 0, 0, 1)


def margins(gt_list, anchors, scores, locs, level_sizes, level_strides, **kw):
    """Evaluates a case in fp64 and in fp32 and returns its figures: 'rank_gap' (a), 'claim_gap' (b), 'sum_gap' (c) of the fp64 evaluation,
    'cost_dev' the largest relative |fp32 - fp64| of a cost over every box's first k_g + 1 region anchors (the costs a decision reads), 'sum_dev' the largest |fp32 - fp64| of rule 5's
    sum, and the two restatements' results."""
    i64, i32 = {}, {}
    idx64, k64 = simota_np(gt_list, anchors, scores, locs, level_sizes, level_strides, dtype=np.float64, info=i64, **kw)
    idx32, k32 = simota_np(gt_list, anchors, scores, locs, level_sizes, level_strides, dtype=F, info=i32, **kw)
    cost_dev, sum_dev = 0.0, 0.0
    for a, b in zip(i64['images'], i32['images']):
        for b64, b32 in zip(a['boxes'], b['boxes']):
            sum_dev = max(sum_dev, abs(b64['total'] - b32['total']))
            head = b64['head']                       # the anchors a decision reads: the k_g candidates (rule 7) and rank k_g + 1
            c64, c32 = b64['cost'][head], b32['cost'][head]
            ok = np.isfinite(c64) & (c64 > 0)
            if ok.any():
                cost_dev = max(cost_dev, float(np.max(np.abs(c32[ok] - c64[ok]) / c64[ok])))
    return dict(rank_gap=min(im['rank_gap'] for im in i64['images']), claim_gap=min(im['claim_gap'] for im in i64['images']),
                sum_gap=min(im['sum_gap'] for im in i64['images']), contested=sum(im['contested'] for im in i64['images']),
                cost_dev=cost_dev, sum_dev=sum_dev, idx64=idx64, k64=k64, idx32=idx32, k32=k32)


def assert_margins(fig):
    assert fig['rank_gap'] >= MIN_RANK_GAP, f"(a) rank gap {fig['rank_gap']:.3g} < {MIN_RANK_GAP}: take another seed"
    assert fig['claim_gap'] >= MIN_CLAIM_GAP, f"(b) claim gap {fig['claim_gap']:.3g} < {MIN_CLAIM_GAP}: take another seed"
    assert fig['sum_gap'] >= MIN_SUM_GAP, f"(c) sum gap {fig['sum_gap']:.3g} < {MIN_SUM_GAP}: take another seed"
    assert np.array_equal(fig['idx64'], fig['idx32']), 'the fp32 and fp64 restatements decide differently'
    assert all(np.array_equal(a, b) for a, b in zip(fig['k64'], fig['k32'])), 'the fp32 and fp64 restatements count differently'
    assert fig['cost_dev'] <= min(MIN_RANK_GAP, MIN_CLAIM_GAP) / 10, (fig['cost_dev'], MIN_RANK_GAP)
    assert fig['sum_dev'] <= MIN_SUM_GAP / 10, (fig['sum_dev'], MIN_SUM_GAP)


# ---- the hand-worked grid (tests/atss_cases.py: 42 anchors, (cx, cy, w, h), levels 4x4x2 / 2x2x2 / 1x1x2 on 64 pixels) -----------------------
GRID_LEVELS = ac.GRID_LEVELS             # (32, 8, 2)
GRID_STRIDES = (16.0, 32.0, 64.0)
GRID_RADIUS = 0.5                        # the centre square is one cell of the anchor's level: half sides 8 / 16 / 32
GRID_C = 3
FAR = tc.FAR                             # an encoded tx that moves a predicted box 10 widths to the right: off the image, u = 0


def _box(x1, y1, x2, y2, cls, score=1.0):
    return [x1, y1, x2, y2, cls, score]


# name -> (boxes, the anchors whose prediction is off the image ('all' or a tuple), candidate_topk, {anchor: box}, [k_g]) worked out by hand --
# see tests/test_simota.py for the working.  Every logit is 0 (cls = 3 log 2 for every anchor and class) and every predicted box is its anchor
# or off the image, so the order of the costs is the reverse order of exact IoUs.
GRID_CASES = {
    # the box IS anchor 10 (level 0, cell (1, 1)); q = 2: the sum of the two largest u is 1 + 176/322 = 1.547, k = 1: the unpenalised anchor 10
    'sum_just_above_1': ([_box(16, 16, 32, 32, 1)], (), 2, {10: 0}, [1]),
    # the same box, q = 10 > its six region anchors: the sum runs over all six, 2.107, k = 2: the two unpenalised anchors
    'fewer_region_anchors_than_q': ([_box(16, 16, 32, 32, 2)], (), 10, {10: 0, 11: 0}, [2]),
    # two level-0 cells side by side: all eight region anchors are penalised, the sum is 2.864, k = 2; anchors 8, 10 and 32 tie at u = 1/2
    'sum_above_2_tie_to_the_lower_index': ([_box(0, 16, 32, 32, 1)], (), 10, {8: 0, 10: 0}, [2]),
    # every prediction off the image: the sum is 0, k clamps to 1 and, every cost equal, the lowest UNPENALISED index wins: 32, not 0
    'all_u_zero': ([_box(0, 0, 32, 32, 2)], 'all', 10, {32: 0}, [1]),
    # the box IS anchor 32: sum 3.390, k = 3: the unpenalised 32 and 33, then the best penalised: 0, 2, 8, 10 (in the box, outside the level-0
    # square) and 40 (in the square, outside the box) tie at u = 1/4 and the lowest index, 0, is taken
    'in_the_box_outside_the_square': ([_box(0, 0, 32, 32, 1)], (), 10, {32: 0, 33: 0, 0: 0}, [3]),
    # sum 3.100, k = 3: the unpenalised 32 and 33 run out and the third is anchor 40, in the square but outside the box (u = 5/16 beats 1/5)
    'in_the_square_outside_the_box': ([_box(0, 0, 40, 32, 3)], (), 10, {32: 0, 33: 0, 40: 0}, [3]),
    # off the image: no centre inside the box or any square
    'no_region_anchor': ([_box(100, 100, 120, 120, 1)], (), 10, {}, [0]),
    # the box's edges AND the level-0 and level-1 squares' edges pass through centres: only level 2's square holds one; u = 1/16 and 2/25
    'edges_through_centres': ([_box(24, 16, 40, 32, 1)], (), 10, {41: 0}, [1]),
    # two identical boxes: every claim ties, the lower index keeps every anchor
    'identical_boxes': ([_box(0, 0, 32, 32, 1), _box(0, 0, 32, 32, 1)], (), 10, {32: 0, 33: 0, 0: 0}, [3, 3]),
    # anchor 32 is the one candidate of both boxes: penalised and cheap (u = 1/2) for box 0, unpenalised and dear (u = 1/16) for box 1.  Box 1 wins
    'unpenalised_claim_beats_the_cheaper_penalised_one': ([_box(0, 16, 32, 32, 1), _box(12, 12, 20, 20, 2)], (8, 10, 33), 10, {32: 1}, [1, 1]),
    # cls = S_a for every anchor, as it is with every logit 0 anyway: the decisions of the box that is anchor 32; the score travels to column 5
    'class_outside_1_to_C': ([_box(0, 0, 32, 32, 5, 0.5)], (), 10, {32: 0, 33: 0, 0: 0}, [3]),
    'empty_image': ([], (), 10, {}, []),
}


def grid_anchors():
    return ac.grid_anchors()


def grid_gt(name):
    return np.array(GRID_CASES[name][0], F).reshape(-1, 6)


def grid_prediction(name):
    """(scores [42, GRID_C], locs [42, 4]) of a grid case."""
    locs = np.zeros((42, 4), F)
    far = GRID_CASES[name][1]
    if far == 'all':
        locs[:, 0] = FAR
    else:
        locs[list(far), 0] = FAR
    return np.zeros((42, GRID_C), F), locs


def grid_kw(name):
    return dict(center_radius=GRID_RADIUS, candidate_topk=GRID_CASES[name][2])


def grid_expected(name):
    """(box_idx int32 [42], dynamic_k int32 [G]) worked out by hand."""
    idx = np.full(42, NOT_MATCHED, np.int32)
    for a, g in GRID_CASES[name][3].items():
        idx[a] = g
    return idx, np.array(GRID_CASES[name][4], np.int32)


# ---- generated cases -----------------------------------------------------------------------------------------------------------------------
# name -> (config, batch, C, make_ground_truth keywords, emptied image or None, keep (boxes kept in the images after the first, or None),
#          keywords of the rule, seed of the prediction)
GENERATED = {
    'mb2_one_empty': ('ssd_mb2_voc', 3, 20, dict(seed=1), 1, None, dict(), 11),
    'mb2_g32': ('ssd_mb2_voc', 3, 20, dict(seed=1, fixed_g=32), None, None, dict(), 12),
    'mb2_g140_then_6': ('ssd_mb2_voc', 3, 20, dict(seed=2, fixed_g=140), None, 6, dict(), 13),   # past the 128-box LDS chunk
    'mb2_q32': ('ssd_mb2_voc', 3, 20, dict(seed=3), None, None, dict(candidate_topk=32), 14),
    'mb2_q1': ('ssd_mb2_voc', 3, 20, dict(seed=3), None, None, dict(candidate_topk=1), 15),
    'mb2_one_class': ('ssd_mb2_voc', 3, 1, dict(seed=4), None, None, dict(), 16),
    'mb2_iou_weight_0': ('ssd_mb2_voc', 3, 20, dict(seed=5), None, None, dict(iou_weight=0.0), 17),   # the class term alone
    'mb2_radius_05': ('ssd_mb2_voc', 3, 20, dict(seed=6), None, None, dict(center_radius=0.5), 18),
    'retina_c80': ('retina_rn50_500_coco', 2, 80, dict(seed=1, fixed_g=32), None, None, dict(), 19),   # 47 961 anchors, five levels
}


def config_levels(config):
    """(level sizes, level strides) of a synthetic config: image size / map size."""
    from single_shot_detection_amd import synthetic as syn
    cfg = syn.CONFIGS[config]
    return ac.config_level_sizes(config), tuple(float(cfg['size']) / float(h) for _, h, _ in cfg['levels'])


def build_case(config, batch, C, gt_kw, emptied, keep, rule_kw, pred_seed):
    gt, anchors, scores, locs, kw = tc.build_case(config, batch, C, gt_kw, emptied, keep, rule_kw, pred_seed, False)
    sizes, strides = config_levels(config)
    assert sum(sizes) == len(anchors)
    return gt, anchors, scores, locs, sizes, strides, kw


@functools.lru_cache(maxsize=None)
def generated(name):
    """(gt list, anchors [A, 4], scores [B, A * C], locs [B, A * 4], level sizes, level strides, rule keywords, the figures of ``margins``)
    -- computed once, margins asserted."""
    gt, anchors, scores, locs, sizes, strides, kw = build_case(*GENERATED[name])
    fig = margins(gt, anchors, scores.reshape(len(gt), len(anchors), -1), locs.reshape(len(gt), len(anchors), 4), sizes, strides, **kw)
    assert_margins(fig)
    return gt, anchors, scores, locs, sizes, strides, kw, fig


@functools.lru_cache(maxsize=None)
def one_thread_owns_three_candidates():
    """``tal_cases.three_anchors_of_one_thread`` for SimOTA: the first box's three largest-u anchors AND its three cheapest are 5, 1 029 and
    2 053, which one sweep thread owns, so in both pop loops that thread's third key comes from the re-read of its anchors.  Both keys
    decide the result: with candidate_topk = 7 the sum of the box's largest u is 5.05 with anchor 2 053's u (0.86) in it and 4.71 with the
    next u in its place, so k_g is 5 or 4; and 2 053 is among the k_g cheapest.  Same tuple as ``generated``; the congruence, the count,
    what a lost third u does to it and the margins are asserted here, on the CPU."""
    gt, anchors, scores, locs = tc.three_anchors_of_one_thread(4, 43, (-2.0, 3.0, -2.0, -2.0), shrink=2)
    sizes, strides, kw = (2500, 3), (16.0, 32.0), dict(candidate_topk=7)
    rx, ry = level_radii_np(sizes, strides, 2.5)
    ins, pen, cost, u = box_costs_np(gt[0][0], anchors, scores[0], locs[0], class_sum_np(scores[0]), rx, ry)
    by_u = np.argsort(-u.astype(np.float64), kind='stable')[:3]
    by_cost = ins[ranked(ins, pen, cost)[:3]]
    assert sorted(ins[by_u].tolist()) == [5, 1029, 2053] and sorted(by_cost.tolist()) == [5, 1029, 2053]
    assert len(set(ins[by_u] % tc.SWEEP_THREADS)) == 1 and len(set(by_cost % tc.SWEEP_THREADS)) == 1
    fig = margins(gt, anchors, scores, locs, sizes, strides, **kw)
    assert_margins(fig)
    k_g = int(fig['k64'][0][0])
    k_without = dynamic_k_np(np.delete(u, by_u[2]), kw['candidate_topk'])[0]     # the owner's re-read finds nothing: the next u is popped
    assert k_g >= 3 and k_without != k_g, (k_g, k_without)
    return gt, anchors, scores.reshape(1, -1), locs.reshape(1, -1), sizes, strides, kw, fig
