"""CPU: the numpy restatement of Task Alignment Learning (tests/tal_cases.py) against cases worked by hand on the 42-anchor, three-level
grid of tests/atss_cases.py, which is what lets the GPU tests check seeded cases against it; its IoU against the oracle's bits; the margins
of every generated case; the host-side argument checks of ssdk_encode_ground_truth_tal; the constructor and the config-name surface."""
import ctypes

import numpy as np
import pytest

import tal_cases as tc
from single_shot_detection_amd import _lib

F = np.float32


# ---- the restatement on the hand-worked grid -----------------------------------------------------------------------------------------------
def _metrics(name, g=0, dtype=np.float64):
    """{inside anchor: (m, u)} of box g of a grid case, from the restatement's own pieces (topk plays no part)."""
    scores, locs = tc.grid_prediction(name)
    ins, m, u = tc.box_metrics_np(tc.grid_gt(name)[g], tc.grid_anchors(), scores, locs, tc.XY_SCALE, tc.WH_SCALE, 1.0, 6.0, dtype)
    return {int(a): (float(mm), float(uu)) for a, mm, uu in zip(ins, m, u)}


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('name', list(tc.GRID_CASES))
def test_restatement_equals_the_hand_worked_case(name, dtype):
    scores, locs = tc.grid_prediction(name)
    idx, col5 = tc.tal_image_np(tc.grid_gt(name), tc.grid_anchors(), scores, locs, topk=tc.GRID_TOPK, dtype=dtype)
    ref_idx, ref_col5 = tc.grid_expected(name)
    assert np.array_equal(idx, ref_idx), {int(a): int(idx[a]) for a in np.nonzero(idx >= 0)[0]}
    assert np.allclose(col5, ref_col5, rtol=1e-6 if dtype is np.float32 else 1e-7, atol=0)
    target = tc.target_np(idx[None], col5[None], [tc.grid_gt(name)])[0]
    gt = tc.grid_gt(name)
    for a in range(42):
        assert target[a, :5].tolist() == (gt[idx[a], :5].tolist() if idx[a] >= 0 else [0, 0, 0, 0, 0])
    assert (target[idx < 0, 5] == 1).all()


def test_box_on_one_cell_by_hand():
    """Box (0, 0, 32, 32), every logit 0 (s = 1/2), every predicted box its anchor.  Centres strictly inside (0, 32)^2: level 0's cells
    (0, 0), (0, 1), (1, 0), (1, 1) -- anchors 0, 1, 2, 3, 8, 9, 10, 11 -- and level 1's cell (0, 0), anchors 32 and 33; level 2's centre (32, 32)
    lies on the corner.  u: anchor 32 is the box, 1; anchor 33 (44 x 22 at (16, 16)) overlaps 32 x 22 = 704 of 1024 + 968 - 704 = 1288; a
    16 x 16 anchor lies inside, 256 / 1024; a 22 x 11 one overlaps 19 x 11 = 209 of 1024 + 242 - 209 = 1057.  m = u^6 / 2: the top three are
    32, 33 and -- four 16 x 16 anchors tie -- the lowest index, 0.  m_max = 1/2 and u_max = 1: t = 1, (704/1288)^6, (1/4)^6."""
    got = _metrics('box_on_one_cell')
    assert sorted(got) == [0, 1, 2, 3, 8, 9, 10, 11, 32, 33]
    assert got[32] == (0.5, 1.0)
    assert np.isclose(got[33][1], 704 / 1288, rtol=1e-12) and np.isclose(got[33][0], .5 * (704 / 1288) ** 6, rtol=1e-12)
    for a in (0, 2, 8, 10):
        assert got[a] == (.5 * .25 ** 6, .25)
    for a in (1, 3, 9, 11):
        assert np.isclose(got[a][1], 209 / 1057, rtol=1e-12) and got[a][0] < got[0][0]
    idx, col5 = tc.grid_expected('box_on_one_cell')
    assert np.nonzero(idx >= 0)[0].tolist() == [0, 32, 33] and col5[32] == 1.0 and col5[0] == .25 ** 6


def test_fewer_inside_anchors_than_topk_are_all_candidates():
    """Box (16, 16, 32, 32): only the centre (24, 24) of level-0 cell (1, 1) lies strictly inside (level 1's 16 is ON x1).  Anchor 10 is the
    box; anchor 11 (22 x 11) overlaps 16 x 11 = 176 of 256 + 242 - 176 = 322.  Two candidates for topk = 3."""
    got = _metrics('fewer_inside_than_topk')
    assert sorted(got) == [10, 11] and got[10] == (0.5, 1.0) and np.isclose(got[11][1], 176 / 322, rtol=1e-12)


def test_no_inside_anchor_and_edges_through_centres():
    assert _metrics('no_inside_anchor') == {} and _metrics('edge_through_centres') == {}
    box, anchors = tc.grid_gt('edge_through_centres')[0], tc.grid_anchors()
    assert anchors[10, 0] == box[0] and anchors[12, 0] == box[2] and anchors[40, 1] == box[3]     # ON the edges: not inside
    assert not tc.inside_np(np.array([np.nan, 0, 64, 64], F), anchors).any()                      # NaN is never inside


def test_contested_anchor_goes_to_the_larger_u_against_the_larger_m():
    """Boxes 0 = (17, 17, 31, 31), class 1, and 1 = (16, 16, 32, 32), class 9 of 3: both hold only the centre (24, 24), so anchors 10 and 11
    are the candidates of both whatever their metric.  u(10) = 196/256 against 1, u(11) = 154/284 (14 x 11 of 196 + 242 - 154) against
    176/322; m of box 0 is u^6 / 2 > 0, of box 1 it is 0 (s = 0).  Box 1 takes both, m_max = 0, t = 0."""
    b0, b1 = _metrics('larger_u_beats_larger_m', 0), _metrics('larger_u_beats_larger_m', 1)
    assert sorted(b0) == sorted(b1) == [10, 11]
    assert np.isclose(b0[10][1], 196 / 256, rtol=1e-12) and np.isclose(b0[11][1], 154 / 284, rtol=1e-12)
    assert b1[10] == (0.0, 1.0) and b1[11][0] == 0.0 and np.isclose(b1[11][1], 176 / 322, rtol=1e-12)
    for a in (10, 11):
        assert b0[a][0] > b1[a][0] and b1[a][1] > b0[a][1]
    idx, col5 = tc.grid_expected('larger_u_beats_larger_m')
    assert idx[10] == idx[11] == 1 and col5[10] == col5[11] == 0.0


def test_all_metrics_zero_take_the_lowest_indices():
    """tx = 100 moves every prediction ten widths right, off the 64-pixel image: u = 0 for the ten inside anchors, every m ties at 0, the
    candidates are anchors 0, 1, 2 and their t is 0 / (0 + 1e-9) * 0 = 0.  The same for a class outside 1..C (s = 0), where u_max = 1/4."""
    got = _metrics('all_u_zero')
    assert len(got) == 10 and all(v == (0.0, 0.0) for v in got.values())
    got = _metrics('class_outside_1_to_C')
    assert len(got) == 10 and all(m == 0.0 for m, _ in got.values()) and got[0][1] == .25
    idx, col5 = tc.grid_expected('class_outside_1_to_C')
    assert np.nonzero(idx >= 0)[0].tolist() == [0, 1, 2] and (col5[:3] == 0).all()


def test_exponents_and_nan():
    x = np.array([0.0, 0.25, 1.0], F)
    assert tc._pow(x, 0.0, False).tolist() == [1, 1, 1] and tc._pow(x, 2.0, False).tolist() == [0, .0625, 1]     # 0^0 = 1
    assert tc._pow(x, 6.0, True).tolist() == [0, .25 ** 6, 1]
    assert np.allclose(tc._pow(x, 2.5, True), [0, .03125, 1]) and tc._pow(x, 2.5, True).dtype == F
    order = tc._ranked(np.arange(4), np.array([0.0, np.nan, 0.5, 0.0]))
    assert order.tolist() == [2, 0, 3, 1]                                                                          # NaN below every number


def test_restatement_iou_is_the_oracles():
    """Rule 2 on anchors as predictions (locs = 0 decode to the anchors: exp(0) = 1) is the oracle's IoU, bit for bit, wherever it is
    defined -- and 0 where the oracle divides 0 by 0."""
    import oracle
    gt, anchors, *_ = tc.build_case(*tc.GENERATED['mb2_one_empty'])
    corners = tc.decode_corners_np(np.zeros((len(anchors), 4), F), anchors, tc.XY_SCALE, tc.WH_SCALE)
    assert np.array_equal(corners.view(np.uint32), oracle.to_corners(anchors).view(np.uint32))
    ref = oracle.iou(np.ascontiguousarray(gt[0][:, :4]), corners)
    got = np.stack([tc.quality_np(corners, b[:4]) for b in gt[0]])
    assert got.dtype == F and np.array_equal(got.view(np.uint32), np.where(np.isfinite(ref), ref, F(0)).astype(F).view(np.uint32))
    assert (got > 0).any() and got.max() <= 1


@pytest.mark.parametrize('name', list(tc.GENERATED))
def test_generated_cases_keep_their_margins(name):
    gt, anchors, scores, locs, kw, fig = tc.generated(name)     # (asserts the margins)
    print(name, {k: float(f'{v:.3g}') for k, v in fig.items() if np.isscalar(v)})
    assert fig['rank_gap'] >= tc.MIN_RANK_GAP and fig['u_gap'] >= tc.MIN_U_GAP and fig['tiny'] == 0
    idx = fig['idx64']
    assert idx.shape == (len(gt), len(anchors)) and (idx >= 0).any()
    assert all((idx[i] == tc.NOT_MATCHED).all() for i, g in enumerate(gt) if not len(g))
    assert set(np.unique(idx)) - {tc.NOT_MATCHED} <= set(range(max(len(g) for g in gt)))     # no ignore band
    col = fig['col64']
    assert (col[idx < 0] == 1).all() and (col[idx >= 0] >= 0).all() and (col[idx >= 0] <= 1 + 1e-6).all()
    for i, g in enumerate(gt):                                                               # at most topk positives per box
        assert all((idx[i] == b).sum() <= kw['topk'] for b in range(len(g)))


def test_the_case_list_covers_what_the_kernels_branch_on():
    cases = {n: tc.build_case(*tc.GENERATED[n]) for n in tc.GENERATED}
    assert any(len(g) == 0 for g in cases['mb2_one_empty'][0])
    assert all(len(g) == 32 for g in cases['mb2_g32'][0])
    assert max(len(g) for g in cases['mb2_g140_topk5'][0]) == 140 and cases['mb2_g140_topk5'][4]['topk'] == 5
    assert cases['mb2_topk32'][4]['topk'] == 32
    assert cases['mb2_one_class'][2].shape[1] == len(cases['mb2_one_class'][1]) and cases['mb2_g32'][2].shape[1] == 20 * len(cases['mb2_g32'][1])
    assert cases['mb2_powf'][4] == dict(topk=13, alpha=0.5, beta=2.5)
    assert all((g[:, 5] < 1).all() for g in cases['mb2_mixup_scores'][0])
    assert len(cases['retina_c80'][1]) == 47961 and cases['retina_c80'][2].shape == (2, 47961 * 80)


# ---- host-side surface -----------------------------------------------------------------------------------------------------------------------
def _refused(status):
    assert status < 0
    assert b'ssdk_encode_ground_truth_tal' in _lib.lib().ssdk_last_error_string()


def test_encode_ground_truth_tal_refuses_bad_arguments_before_any_launch():
    """Host-only, as tests/test_atss.py: the device pointers are never dereferenced."""
    lib = _lib.lib()
    p = ctypes.c_void_p(256)
    need = lib.ssdk_encode_ground_truth_tal_workspace_bytes(2, 7, 13)
    assert need >= 7 * 8 + 7 * 32 * 16
    assert lib.ssdk_encode_ground_truth_tal_workspace_bytes(2, 70, 13) > need

    def call(rows=p, stride=6, offs=p, batch=2, total=7, anchors=p, num_anchors=100, scores=p, columns=20, locs=p, topk=13, alpha=1.0,
             beta=6.0, target=p, ws=p, nbytes=need):
        return lib.ssdk_encode_ground_truth_tal(rows, stride, offs, batch, total, anchors, num_anchors, scores, columns, locs, 10.0, 5.0, topk,
                                                alpha, beta, target, None, ws, nbytes, None)
    _refused(call(rows=None))
    _refused(call(offs=None))
    _refused(call(anchors=None))
    _refused(call(target=None))
    _refused(call(scores=None))
    _refused(call(locs=None))
    _refused(call(batch=0))
    _refused(call(num_anchors=0))
    _refused(call(total=-1))
    _refused(call(stride=5))
    _refused(call(columns=0))
    _refused(call(topk=0))
    _refused(call(topk=33))
    for bad in (-0.5, float('inf'), float('nan')):
        _refused(call(alpha=bad))
        _refused(call(beta=bad))
    _refused(call(ws=None))
    _refused(call(nbytes=need - 1))
    _refused(call(locs=ctypes.c_void_p(260)))      # the kernels move 16-byte locs and anchors


def test_constructor():
    import torch
    from single_shot_detection_amd.detection.target_assigner import TaskAlignedAssigner
    ta = TaskAlignedAssigner()
    assert (ta.topk, ta.alpha, ta.beta) == (13, 1.0, 6.0)
    ta = TaskAlignedAssigner(topk=5, alpha=0.5, beta=2.5)
    assert (ta.topk, ta.alpha, ta.beta) == (5, 0.5, 2.5)
    for bad in (0, 33, 2.5, -1):
        with pytest.raises(ValueError):
            TaskAlignedAssigner(topk=bad)
    for bad in (-1.0, float('inf'), float('nan'), 'x'):
        with pytest.raises(ValueError):
            TaskAlignedAssigner(alpha=bad)
        with pytest.raises(ValueError):
            TaskAlignedAssigner(beta=bad)
    with pytest.raises(ValueError):
        ta.encode_ground_truth([torch.zeros((1, 6))], torch.zeros((10, 4)), None, tc.Coder())
    with pytest.raises(ValueError):
        ta.encode_ground_truth([torch.zeros((1, 6))], torch.zeros((10, 4)), (torch.zeros((1, 30)), torch.zeros((1, 40))), None)
    with pytest.raises(_lib.SsdkError):          # no CPU fallback
        ta.encode_ground_truth([torch.zeros((1, 6))], torch.zeros((10, 4)), (torch.zeros((1, 30)), torch.zeros((1, 40))), tc.Coder())
    doc = ' '.join(TaskAlignedAssigner.__doc__.split())
    assert 'NO force stage' in doc and 'constants of the step' in doc
    assert 'one more pass' in ' '.join(TaskAlignedAssigner.encode_ground_truth.__doc__.split())


def test_config_name_selects_the_assigner():
    from single_shot_detection_amd.detection import init as det_init, matcher
    from single_shot_detection_amd.detection.target_assigner import TargetAssigner, TaskAlignedAssigner
    assert det_init.TARGET_ASSIGNERS['TaskAlignedAssigner'] is TaskAlignedAssigner
    ta = det_init.build_target_assigner({'name': 'TaskAlignedAssigner', 'topk': 7, 'beta': 4.0})
    assert type(ta) is TaskAlignedAssigner and (ta.topk, ta.alpha, ta.beta) == (7, 1.0, 4.0)
    assert type(det_init.build_target_assigner({'matched_threshold': .5, 'unmatched_threshold': .4})) is TargetAssigner   # nothing changes
    with pytest.raises(ValueError):
        det_init.build_target_assigner({'name': 'TaskAlignedAssigner', 'topk': 40})
    assert callable(matcher.match_task_aligned)


def test_one_thread_owns_three_candidates_case():
    """The case asserts its own conditions (three best anchors congruent mod 1 024, the margins); all three are the first box's positives."""
    gt, anchors, scores, locs, kw, fig = tc.one_thread_owns_three_candidates()
    assert kw['topk'] >= 3 and len(anchors) > 2 * tc.SWEEP_THREADS + 5
    assert (fig['idx64'][0, [5, 1029, 2053]] == 0).all()
