"""CPU: the numpy restatement of SimOTA (tests/simota_cases.py) against cases worked by hand on the 42-anchor, three-level grid of
tests/atss_cases.py (strides 16 / 32 / 64 on 64 pixels, center_radius 0.5: the centre square is one cell of the anchor's level), which is
what lets the GPU tests check seeded cases against it; the softplus form of the class term against a direct BCE sum; the margins of every
generated case; the host-side argument checks of ssdk_encode_ground_truth_simota; the constructor and the config-name surface."""
import ctypes

import numpy as np
import pytest

import simota_cases as sc
from single_shot_detection_amd import _lib

F = np.float32


# ---- the restatement on the hand-worked grid -----------------------------------------------------------------------------------------------
def _region(name, g=0):
    """{region anchor: (penalised, in_box, in_centre, u)} of box g of a grid case, from the restatement's own pieces, in fp64."""
    scores, locs = sc.grid_prediction(name)
    anchors, box = sc.grid_anchors(), sc.grid_gt(name)[g]
    rx, ry = sc.level_radii_np(sc.GRID_LEVELS, sc.GRID_STRIDES, sc.GRID_RADIUS)
    _, _, in_box, in_centre = sc.region_np(box, anchors, rx, ry)
    ins, pen, cost, u = sc.box_costs_np(box, anchors, scores, locs, sc.class_sum_np(scores, np.float64), rx, ry, dtype=np.float64)
    assert np.all(np.diff(cost[np.argsort(-u, kind='stable')]) >= 0)          # every logit 0: the cost falls as u grows
    return {int(a): (bool(p), bool(in_box[a]), bool(in_centre[a]), float(v)) for a, p, v in zip(ins, pen, u)}


def _sum(name, g=0):
    reg = _region(name, g)
    return sc.dynamic_k_np(np.array([v[3] for v in reg.values()]), sc.GRID_CASES[name][2])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('name', list(sc.GRID_CASES))
def test_restatement_equals_the_hand_worked_case(name, dtype):
    scores, locs = sc.grid_prediction(name)
    gt = sc.grid_gt(name)
    idx, k = sc.simota_image_np(gt, sc.grid_anchors(), scores, locs, sc.GRID_LEVELS, sc.GRID_STRIDES, dtype=dtype, **sc.grid_kw(name))
    ref_idx, ref_k = sc.grid_expected(name)
    assert np.array_equal(idx, ref_idx), {int(a): int(idx[a]) for a in np.nonzero(idx >= 0)[0]}
    assert np.array_equal(k, ref_k), k.tolist()
    target = sc.target_np(idx[None], [gt])[0]
    for a in range(42):
        assert target[a].tolist() == (gt[idx[a]].tolist() if idx[a] >= 0 else [0, 0, 0, 0, 0, 1])


def test_the_box_that_is_anchor_10_by_hand():
    """Box (16, 16, 32, 32), gc = (24, 24).  In the box: only level 0's centre (24, 24) -- anchors 10 and 11; level 1's 16 is ON x1.  Squares:
    level 0, (16, 32)^2, again 10 and 11: both UNPENALISED; level 1, (8, 40)^2, holds (16, 16): anchors 32 and 33, outside the box; level 2,
    (-8, 56)^2, holds (32, 32): 40 and 41.  u: 10 is the box, 1; 11 (22 x 11) overlaps 16 x 11 = 176 of 256 + 242 - 176 = 322; 32 (32 x 32)
    holds the box, 256 / 1024; 33 (44 x 22 at (16, 16): x -6..38, y 5..27) overlaps 16 x 11 = 176 of 256 + 968 - 176 = 1048; 40 holds it,
    256 / 4096; 41 (80 x 40: y 12..52) holds it, 256 / 3200.  q = 2: 1 + 176/322 = 1.547, k = 1.  q = 10: all six, 2.107, k = 2."""
    reg = _region('sum_just_above_1')
    assert sorted(reg) == [10, 11, 32, 33, 40, 41]
    assert [a for a in reg if not reg[a][0]] == [10, 11] and all(reg[a][1:3] == (False, True) for a in (32, 33, 40, 41))
    want = {10: 1.0, 11: 176 / 322, 32: .25, 33: 176 / 1048, 40: .0625, 41: .08}
    assert all(np.isclose(reg[a][3], want[a], rtol=1e-12) for a in want)
    k, total, qq = _sum('sum_just_above_1')
    assert (k, qq) == (1, 2) and np.isclose(total, 1 + 176 / 322, rtol=1e-12)
    k, total, qq = _sum('fewer_region_anchors_than_q')
    assert (k, qq) == (2, 6) and np.isclose(total, sum(want.values()), rtol=1e-12) and 2 < total < 3


def test_a_tie_at_the_cutoff_goes_to_the_lower_indices():
    """Box (0, 16, 32, 32) = level-0 cells (0, 1) and (1, 1), gc = (16, 24).  In the box: (8, 24) and (24, 24), anchors 8..11.  Level 0's square
    is (8, 24) x (16, 32): 8 and 24 are ON its edges, nothing.  Level 1's, (0, 32) x (8, 40), holds (16, 16): 32, 33; level 2's holds 40, 41.
    All eight are penalised.  u: 8, 10 (16 x 16 inside) 256 / 512; 32 overlaps 32 x 16 = 512 of 1024; 9, 11 overlap 19 x 11 = 209 of
    512 + 242 - 209 = 545; 33 overlaps 32 x 11 = 352 of 512 + 968 - 352 = 1128; 41 holds it, 512 / 3200; 40 holds it, 512 / 4096.
    Sum 2.864, k = 2: of the three anchors at 1/2 the two lower indices."""
    reg = _region('sum_above_2_tie_to_the_lower_index')
    assert sorted(reg) == [8, 9, 10, 11, 32, 33, 40, 41] and all(v[0] for v in reg.values())
    assert reg[8][3] == reg[10][3] == reg[32][3] == 0.5
    assert np.isclose(reg[9][3], 209 / 545, rtol=1e-12) and np.isclose(reg[33][3], 352 / 1128, rtol=1e-12)
    k, total, _ = _sum('sum_above_2_tie_to_the_lower_index')
    assert k == 2 and np.isclose(total, 1.5 + 2 * 209 / 545 + 352 / 1128 + .16 + .125, rtol=1e-12)


def test_penalty_classes_by_hand():
    """Box (0, 0, 32, 32) = anchor 32, gc = (16, 16).  In the box: level 0's four cells (anchors 0..3, 8..11) and level 1's (16, 16): 32, 33;
    level 2's (32, 32) is ON the corner.  Level 0's square (8, 24)^2 has 8 and 24 ON its edges: nothing -- those eight are in the box but
    outside the square.  Level 1's square holds 32, 33: unpenalised.  Level 2's holds 40, 41: in the square, outside the box.  u: 32 1;
    33 704 / 1288; the 16 x 16 anchors and 40 (1024 / 4096) 1/4; the 22 x 11 209 / 1057; 41 640 / 3584.  The ten largest sum to 3.390: k = 3:
    32, 33, then the lowest index at 1/4: 0.  With every prediction off the image every cost is equal: k = 1 and 32, not 0.
    Box (0, 0, 40, 32), gc = (20, 16): the same twelve anchors.  u: 32 1024 / 1280; 33 836 / 1412; 40 1280 / 4096 = 5/16; 41 800 / 3680; the
    16 x 16 256 / 1280 = 1/5.  Sum 3.100, k = 3: 32, 33, then 40."""
    reg = _region('in_the_box_outside_the_square')
    assert sorted(reg) == [0, 1, 2, 3, 8, 9, 10, 11, 32, 33, 40, 41]
    assert all(reg[a][:3] == (True, True, False) for a in (0, 1, 2, 3, 8, 9, 10, 11))
    assert all(reg[a][:3] == (False, True, True) for a in (32, 33)) and all(reg[a][:3] == (True, False, True) for a in (40, 41))
    assert reg[32][3] == 1.0 and all(reg[a][3] == .25 for a in (0, 2, 8, 10, 40)) and np.isclose(reg[41][3], 640 / 3584, rtol=1e-12)
    k, total, _ = _sum('in_the_box_outside_the_square')
    assert k == 3 and np.isclose(total, 1 + 704 / 1288 + 5 * .25 + 3 * 209 / 1057, rtol=1e-12)
    assert _sum('all_u_zero')[:2] == (1, 0.0) and all(v[3] == 0 for v in _region('all_u_zero').values())
    reg = _region('in_the_square_outside_the_box')
    assert sorted(reg) == [0, 1, 2, 3, 8, 9, 10, 11, 32, 33, 40, 41] and [a for a in reg if not reg[a][0]] == [32, 33]
    assert reg[32][3] == F(.8) or np.isclose(reg[32][3], .8, rtol=1e-12)
    assert reg[40][3] == 5 / 16 and np.isclose(reg[41][3], 800 / 3680, rtol=1e-12) and np.isclose(reg[0][3], .2, rtol=1e-12)
    k, total, _ = _sum('in_the_square_outside_the_box')
    assert k == 3 and 3 < total < 3.2


def test_no_region_edges_and_nan():
    assert _region('no_region_anchor') == {} and _sum('no_region_anchor')[0] == 0
    # box (24, 16, 40, 32), gc = (32, 24): 24 and 40 are ON the box's and level 0's square's edges, 16 and 48 ON level 1's square (16, 48)
    reg = _region('edges_through_centres')
    assert sorted(reg) == [40, 41] and reg[40][3] == .0625 and np.isclose(reg[41][3], .08, rtol=1e-12)
    anchors = sc.grid_anchors()
    rx, ry = sc.level_radii_np(sc.GRID_LEVELS, sc.GRID_STRIDES, sc.GRID_RADIUS)
    assert rx[0] == 8 and rx[32] == 16 and rx[40] == 32 and np.array_equal(rx, ry)
    region, pen, _, _ = sc.region_np(np.array([np.nan, 0, 64, 64], F), anchors, rx, ry)
    assert not region.any() and pen.all()                                                      # NaN is in neither
    sx_sy = sc.level_radii_np((2, 1), ((16.0, 8.0), 32.0), 2.5)
    assert sx_sy[0].tolist() == [40, 40, 80] and sx_sy[1].tolist() == [20, 20, 80]


def test_unpenalised_claim_beats_the_cheaper_penalised_one_by_hand():
    """Predictions of anchors 8, 10 and 33 off the image.  Box 0 = (0, 16, 32, 32): all penalised (see above); u: 32 1/2, 9 and 11 209/545,
    41 .16, 40 .125, the rest 0: sum 1.552, k = 1: anchor 32.  Box 1 = (12, 12, 20, 20), gc = (16, 16): in the box and in level 1's square:
    32, 33, unpenalised; 40, 41 in level 2's square.  u: 32 64 / 1024, 33 0, 41 64 / 3200, 40 64 / 4096: sum 0.098, k = 1: anchor 32.  Both claim
    32: box 0 at the lower cost, box 1 unpenalised -- box 1 keeps it, box 0 has no positive."""
    name = 'unpenalised_claim_beats_the_cheaper_penalised_one'
    r0, r1 = _region(name, 0), _region(name, 1)
    assert r0[32][0] and not r1[32][0] and r0[32][3] == .5 and r1[32][3] == .0625
    assert _sum(name, 0)[0] == _sum(name, 1)[0] == 1
    idx, _ = sc.grid_expected(name)
    assert idx[32] == 1 and (idx >= 0).sum() == 1


def test_dynamic_k():
    assert sc.dynamic_k_np(np.array([], F), 10) == (0, 0.0, 0)
    assert sc.dynamic_k_np(np.array([0.0, 0.0], F), 10)[0] == 1                 # clamps to 1
    assert sc.dynamic_k_np(np.array([1.0, 1.0], F), 10)[0] == 2                 # (int)sum = q' = n: the upper clamp
    assert sc.dynamic_k_np(np.array([.5, .5, .5, .5, .5], F), 4) == (2, 2.0, 4)  # the q largest only
    assert sc.dynamic_k_np(np.array([.5, .5, .5, .4], F), 10)[0] == 1            # truncation, not rounding
    order = sc.ranked(np.arange(5), np.array([True, False, False, True, False]), np.array([0.0, np.nan, 2.0, 1.0, 2.0]))
    assert order.tolist() == [2, 4, 1, 0, 3]                                     # unpenalised first, NaN above every number, ties by index


def test_softplus_form_is_the_bce_sum():
    """S_a - x_k against the direct sum over the columns of BCE(sigmoid(x_c), [c == k]) in fp64."""
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal((50, 7)) * 4, [[0] * 7, [30, -30, 0, 5, -5, 1, -1]]]).astype(F)
    S = sc.class_sum_np(x, np.float64)
    x64 = x.astype(np.float64)
    log_p, log_1mp = -np.logaddexp(0, -x64), -np.logaddexp(0, x64)               # log sigmoid(x), log(1 - sigmoid(x))
    mild = np.abs(x64) < 10                                                      # (where 1 - p keeps its digits: the two against the plain form)
    p = 1 / (1 + np.exp(-x64))
    assert np.allclose(np.log(p)[mild], log_p[mild], rtol=1e-9) and np.allclose(np.log(1 - p)[mild], log_1mp[mild], rtol=1e-9)
    for k in range(7):
        onehot = np.zeros(7)
        onehot[k] = 1
        direct = -(onehot * log_p + (1 - onehot) * log_1mp).sum(axis=1)
        assert np.allclose(S - x64[:, k], direct, rtol=1e-12, atol=1e-12)
    assert np.allclose(S, -log_1mp.sum(axis=1), rtol=1e-12)                       # the all-zero row of a class outside 1..C
    assert sc.class_sum_np(np.zeros((1, 3), F), F)[0] == F(np.log(F(2))) + F(np.log(F(2))) + F(np.log(F(2)))
    assert sc.class_sum_np(x, F).dtype == F and np.allclose(sc.class_sum_np(x, F), S, rtol=1e-6)


@pytest.mark.parametrize('name', list(sc.GENERATED))
def test_generated_cases_keep_their_margins(name):
    gt, anchors, scores, locs, sizes, strides, kw, fig = sc.generated(name)     # (asserts the margins)
    print(name, {k: float(f'{v:.3g}') for k, v in fig.items() if np.isscalar(v)})
    assert fig['rank_gap'] >= sc.MIN_RANK_GAP and fig['claim_gap'] >= sc.MIN_CLAIM_GAP and fig['sum_gap'] >= sc.MIN_SUM_GAP
    assert 10 * fig['cost_dev'] <= min(sc.MIN_RANK_GAP, sc.MIN_CLAIM_GAP) and 10 * fig['sum_dev'] <= sc.MIN_SUM_GAP
    idx = fig['idx64']
    assert idx.shape == (len(gt), len(anchors)) and (idx >= 0).any()
    assert all((idx[i] == sc.NOT_MATCHED).all() for i, g in enumerate(gt) if not len(g))
    assert set(np.unique(idx)) - {sc.NOT_MATCHED} <= set(range(max(len(g) for g in gt)))     # no ignore band
    q = kw.get('candidate_topk', 10)
    for i, g in enumerate(gt):                                                               # at most k_g positives per box
        k = fig['k64'][i]
        assert len(k) == len(g) and (k <= q).all() and (k >= 0).all()
        assert all((idx[i] == b).sum() <= k[b] for b in range(len(g)))


def test_the_case_list_covers_what_the_kernels_branch_on():
    cases = {n: sc.build_case(*sc.GENERATED[n]) for n in sc.GENERATED}
    assert any(len(g) == 0 for g in cases['mb2_one_empty'][0]) and len(cases['mb2_one_empty'][1]) == 2268
    assert all(len(g) == 32 for g in cases['mb2_g32'][0])
    assert [len(g) for g in cases['mb2_g140_then_6'][0]] == [140, 6, 6]
    assert cases['mb2_q32'][6] == dict(candidate_topk=32) and cases['mb2_q1'][6] == dict(candidate_topk=1)
    assert cases['mb2_one_class'][2].shape[1] == 2268 and cases['mb2_g32'][2].shape[1] == 20 * 2268
    assert cases['mb2_iou_weight_0'][6] == dict(iou_weight=0.0) and cases['mb2_radius_05'][6] == dict(center_radius=0.5)
    assert len(cases['retina_c80'][1]) == 47961 and cases['retina_c80'][2].shape == (2, 47961 * 80) and len(cases['retina_c80'][4]) == 5
    assert len(cases['mb2_g32'][4]) == 6 and np.isclose(cases['mb2_g32'][5][0], 300 / 19)
    assert max(np.concatenate(sc.generated('mb2_q32')[7]['k64'])) > 10                       # more positives than the default q allows


# ---- host-side surface -----------------------------------------------------------------------------------------------------------------------
def _refused(status):
    assert status < 0
    assert b'ssdk_encode_ground_truth_simota' in _lib.lib().ssdk_last_error_string()


def test_encode_ground_truth_simota_refuses_bad_arguments_before_any_launch():
    """Host-only, as tests/test_tal.py: the device pointers are never dereferenced."""
    lib = _lib.lib()
    p = ctypes.c_void_p(256)
    need = lib.ssdk_encode_ground_truth_simota_workspace_bytes(2, 7, 100, 2)
    assert need >= 2 * 100 * 4 + 7 * 8
    assert lib.ssdk_encode_ground_truth_simota_workspace_bytes(2, 700, 100, 2) > need
    assert lib.ssdk_encode_ground_truth_simota_workspace_bytes(2, 7, 1000, 2) > need
    sizes, strides = (ctypes.c_int32 * 2)(60, 40), (ctypes.c_float * 4)(8.0, 8.0, 16.0, 16.0)

    def call(rows=p, stride=6, offs=p, batch=2, total=7, anchors=p, num_anchors=100, level_sizes=sizes, level_strides=strides, n_levels=2,
             scores=p, columns=20, locs=p, radius=2.5, q=10, weight=3.0, target=p, ws=p, nbytes=need):
        return lib.ssdk_encode_ground_truth_simota(rows, stride, offs, batch, total, anchors, num_anchors, level_sizes, level_strides, n_levels,
                                                   scores, columns, locs, 10.0, 5.0, radius, q, weight, target, None, None, ws, nbytes, None)
    _refused(call(rows=None))
    _refused(call(offs=None))
    _refused(call(anchors=None))
    _refused(call(target=None))
    _refused(call(scores=None))
    _refused(call(locs=None))
    _refused(call(level_sizes=None))
    _refused(call(level_strides=None))
    _refused(call(batch=0))
    _refused(call(num_anchors=0))
    _refused(call(total=-1))
    _refused(call(stride=5))
    _refused(call(columns=0))
    _refused(call(n_levels=0))
    _refused(call(n_levels=17))
    _refused(call(q=0))
    _refused(call(q=33))
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        _refused(call(radius=bad))
    for bad in (-0.5, float('inf'), float('nan')):
        _refused(call(weight=bad))
    _refused(call(level_sizes=(ctypes.c_int32 * 2)(60, 41)))              # do not sum to the anchors
    _refused(call(level_sizes=(ctypes.c_int32 * 2)(100, 0)))
    for bad in (0.0, -8.0, float('inf'), float('nan')):
        _refused(call(level_strides=(ctypes.c_float * 4)(8.0, 8.0, 16.0, bad)))
    _refused(call(ws=None))
    _refused(call(nbytes=need - 1))
    _refused(call(locs=ctypes.c_void_p(260)))      # the kernels move 16-byte locs and anchors


def test_constructor():
    import torch
    from single_shot_detection_amd.detection.target_assigner import SimOtaAssigner
    sa = SimOtaAssigner()
    assert (sa.center_radius, sa.candidate_topk, sa.iou_weight) == (2.5, 10, 3.0)
    sa = SimOtaAssigner(center_radius=0.5, candidate_topk=32, iou_weight=0)
    assert (sa.center_radius, sa.candidate_topk, sa.iou_weight) == (0.5, 32, 0.0)
    for bad in (0, 33, 2.5, -1, True, 'x', None, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            SimOtaAssigner(candidate_topk=bad)
    for bad in (0.0, -1.0, float('inf'), float('nan'), 'x', None):
        with pytest.raises(ValueError):
            SimOtaAssigner(center_radius=bad)
    for bad in (-1.0, float('inf'), float('nan'), 'x', None):
        with pytest.raises(ValueError):
            SimOtaAssigner(iou_weight=bad)
    gt, anchors, pred = [torch.zeros((1, 6))], torch.zeros((10, 4)), (torch.zeros((1, 30)), torch.zeros((1, 40)))
    with pytest.raises(ValueError):
        sa.encode_ground_truth(gt, anchors, None, sc.Coder(), level_sizes=(10,), level_strides=(8.0,))
    with pytest.raises(ValueError):
        sa.encode_ground_truth(gt, anchors, pred, None, level_sizes=(10,), level_strides=(8.0,))
    with pytest.raises(ValueError):
        sa.encode_ground_truth(gt, anchors, pred, sc.Coder())                                       # the levels are required
    with pytest.raises(ValueError):
        sa.encode_ground_truth(gt, anchors, pred, sc.Coder(), level_sizes=(6, 3), level_strides=(8.0, 16.0))
    with pytest.raises(ValueError):
        sa.encode_ground_truth(gt, anchors, pred, sc.Coder(), level_sizes=(6, 4), level_strides=(8.0,))
    with pytest.raises(ValueError):
        sa.encode_ground_truth(gt, anchors, pred, sc.Coder(), level_sizes=(6, 4), level_strides=(8.0, 0.0))
    with pytest.raises(_lib.SsdkError):          # no CPU fallback
        sa.encode_ground_truth(gt, anchors, pred, sc.Coder(), level_sizes=(6, 4), level_strides=(8.0, (16.0, 16.0)))
    doc = ' '.join(SimOtaAssigner.__doc__.split())
    assert 'NO force stage' in doc and 'constants of the step' in doc and 'own region' in doc


def test_config_name_selects_the_assigner():
    from single_shot_detection_amd.detection import init as det_init, matcher
    from single_shot_detection_amd.detection.detector import Detector
    from single_shot_detection_amd.detection.target_assigner import SimOtaAssigner, TargetAssigner
    assert det_init.TARGET_ASSIGNERS['SimOtaAssigner'] is SimOtaAssigner
    sa = det_init.build_target_assigner({'name': 'SimOtaAssigner'})
    assert type(sa) is SimOtaAssigner and (sa.center_radius, sa.candidate_topk, sa.iou_weight) == (2.5, 10, 3.0)
    sa = det_init.build_target_assigner({'name': 'SimOtaAssigner', 'candidate_topk': 7, 'center_radius': 1.5})
    assert (sa.center_radius, sa.candidate_topk) == (1.5, 7)
    assert type(det_init.build_target_assigner({'matched_threshold': .5, 'unmatched_threshold': .4})) is TargetAssigner   # nothing changes
    with pytest.raises(ValueError):
        det_init.build_target_assigner({'name': 'SimOtaAssigner', 'candidate_topk': 40})
    with pytest.raises(ValueError):
        det_init.build_target_assigner({'name': 'SimOta'})
    assert callable(matcher.match_simota) and callable(Detector.anchor_level_strides)


def test_abi_revision_and_limits():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ssdk.h')).read()
    assert int(re.search(r'#define\s+SSDK_VERSION\s+(\d+)', text).group(1)) >= 132
    assert int(re.search(r'#define\s+SSDK_SIMOTA_MAX_TOPK\s+(\d+)', text).group(1)) == 32
    assert _lib.lib().ssdk_version() >= 132


def test_one_thread_owns_three_candidates_case():
    """The case asserts its own conditions (three largest-u and three cheapest anchors congruent mod 1 024, k_g >= 3, the margins); all
    three are the first box's positives."""
    gt, anchors, scores, locs, sizes, strides, kw, fig = sc.one_thread_owns_three_candidates()
    assert fig['k64'][0][0] >= 3 and sum(sizes) == len(anchors)
    assert (fig['idx64'][0, [5, 1029, 2053]] == 0).all()
