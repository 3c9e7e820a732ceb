"""CPU: the numpy restatement of ATSS (tests/atss_cases.py) against cases worked by hand on a 42-anchor, three-level grid, which is what
lets the GPU tests check seeded cases against it; the host-side argument checks of ssdk_encode_ground_truth_atss; the constructor and the
config-name surface."""
import ctypes

import numpy as np
import pytest

import atss_cases as ac
from single_shot_detection_amd import _lib


# ---- the restatement on the hand-worked grid -----------------------------------------------------------------------------------------------
def _candidates(box, anchors):
    """(candidate anchors, their IoUs, t_g) of one box on the grid, from the restatement's own pieces."""
    gcx, gcy = (box[0] + box[2]) * np.float32(.5), (box[1] + box[3]) * np.float32(.5)
    d2 = (anchors[:, 0] - gcx) ** 2 + (anchors[:, 1] - gcy) ** 2
    cands, start = [], 0
    for n in ac.GRID_LEVELS:
        cands += (start + np.argsort(d2[start:start + n], kind='stable')[:min(ac.GRID_TOPK, n)]).tolist()
        start += n
    v = ac.iou_np(box[:4], ac.to_corners_np(anchors)[cands]).astype(np.float64)
    return cands, v, v.mean() + v.std(ddof=1)


def test_the_grid_is_the_one_the_cases_were_worked_on():
    a = ac.grid_anchors()
    assert a.shape == (42, 4) and sum(ac.GRID_LEVELS) == 42 and ac.GRID_LEVELS[-1] < ac.GRID_TOPK
    assert a[10].tolist() == [24, 24, 16, 16] and a[11].tolist() == [24, 24, 22, 11] and a[12].tolist() == [40, 24, 16, 16]
    assert a[32].tolist() == [16, 16, 32, 32] and a[34].tolist() == [48, 16, 32, 32] and a[41].tolist() == [32, 32, 80, 40]


@pytest.mark.parametrize('name', list(ac.GRID_CASES))
def test_restatement_equals_the_hand_worked_case(name):
    idx, _ = ac.atss_image_np(ac.grid_gt(name), ac.grid_anchors(), ac.GRID_LEVELS, ac.GRID_TOPK)
    assert np.array_equal(idx, ac.grid_expected(name)), {int(a): int(idx[a]) for a in np.nonzero(idx >= 0)[0]}


def test_centred_box_by_hand():
    """Box (16, 16, 32, 32).  Level 0: the two anchors of cell (1, 1) at d2 = 0, then four cells tie at d2 = 256 and the lowest index, anchor
    2 of cell (0, 1), is taken.  Level 1: cell (0, 0) at d2 = 128 (32, 33), then (1, 0) and (0, 1) tie at 640: anchor 34.  Level 2: both.
    IoUs 1, 176/322, 0, 256/1024, 176/1048, 0, 256/4096, 256/3200: mean 0.2634, deviation 0.3474, t = 0.6108 -- only anchor 10."""
    cands, v, t = _candidates(ac.grid_gt('centred_on_a_cell')[0], ac.grid_anchors())
    assert cands == [10, 11, 2, 32, 33, 34, 40, 41]
    assert np.allclose(v, [1, 176 / 322, 0, .25, 176 / 1048, 0, .0625, .08], atol=1e-7)
    assert abs(t - 0.6108) < 1e-4 and (v >= t).tolist() == [True] + [False] * 7


def test_distance_tie_across_cells_goes_to_the_lower_anchor():
    """Box (22, 14, 42, 34), centre (32, 24): cells (1, 1) and (1, 2) both at d2 = 64.  topk = 3 takes 10, 11 and anchor 12 but not 13."""
    cands, v, t = _candidates(ac.grid_gt('between_two_cells')[0], ac.grid_anchors())
    assert cands[:3] == [10, 11, 12] and 13 not in cands
    assert v[0] == v[2] and (v >= t).tolist()[:3] == [True, False, True]     # the two square anchors mirror each other


def test_strictly_inside_is_what_fails_on_the_edge():
    """Box (24, 16, 40, 32): IoU alone would make anchors 10, 11 and 12 positive (128/384, 121/377, 128/384 reach t), their centres lie ON
    x1 and x2."""
    box, anchors = ac.grid_gt('edge_through_centres')[0], ac.grid_anchors()
    cands, v, t = _candidates(box, anchors)
    assert np.allclose(v[:3], [128 / 384, 121 / 377, 128 / 384], atol=1e-7)
    assert [a for a, x in zip(cands, v) if x >= t] == [10, 11, 12]
    assert anchors[10, 0] == anchors[11, 0] == box[0] and anchors[12, 0] == box[2]
    assert not (ac.grid_expected('edge_through_centres') >= 0).any()


def test_restatement_iou_is_the_oracles():
    import oracle
    gt, anchors, *_ = ac.generated('mb2_default_one_empty')
    corners = ac.to_corners_np(anchors)
    assert np.array_equal(corners.view(np.uint32), oracle.to_corners(anchors).view(np.uint32))
    ref = oracle.iou(np.ascontiguousarray(gt[0][:, :4]), corners)
    got = np.stack([ac.iou_np(b[:4], corners) for b in gt[0]])
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize('name', list(ac.GENERATED))
def test_generated_cases_keep_their_margin(name):
    gt, anchors, levels, topk, box_idx, margin = ac.generated(name)
    assert margin >= ac.MIN_MARGIN
    assert box_idx.shape == (len(gt), len(anchors)) and (box_idx >= 0).any()
    assert all((box_idx[i] == ac.NOT_MATCHED).all() for i, g in enumerate(gt) if not len(g))
    assert set(np.unique(box_idx)) - {ac.NOT_MATCHED} <= set(range(max(len(g) for g in gt)))     # no ignore band


def test_three_candidates_of_one_box_1024_anchors_apart():
    gt, anchors, levels, topk, box_idx, margin = ac.one_thread_owns_three_candidates()
    cands = np.argsort(((anchors[:levels[0], :2] - [130, 125]) ** 2).sum(1), kind='stable')[:3]
    assert cands.tolist() == [5, 1029, 2053] and box_idx[0, 5] == 0 and margin >= ac.MIN_MARGIN


# ---- host-side surface -----------------------------------------------------------------------------------------------------------------------
def _refused(status):
    assert status < 0
    assert b'ssdk_encode_ground_truth_atss' in _lib.lib().ssdk_last_error_string()


def test_encode_ground_truth_atss_refuses_bad_arguments_before_any_launch():
    """Host-only, as tests/test_bipartite.py: the device pointers are never dereferenced (level_sizes is host memory and is read)."""
    lib = _lib.lib()
    p = ctypes.c_void_p(256)
    sizes = (ctypes.c_int32 * 3)(60, 30, 10)
    need = lib.ssdk_encode_ground_truth_atss_workspace_bytes(2, 7, 3)
    assert need >= 7 * 3 * 8 + 7 * 3 * 32 * 4
    assert lib.ssdk_encode_ground_truth_atss_workspace_bytes(2, 7, 4) > need

    def call(rows=p, stride=6, offs=p, batch=2, total=7, anchors=p, num_anchors=100, levels=sizes, n_levels=3, topk=9, target=p, ws=p, nbytes=need):
        return lib.ssdk_encode_ground_truth_atss(rows, stride, offs, batch, total, anchors, num_anchors, levels, n_levels, topk, target, None,
                                                 ws, nbytes, None)
    _refused(call(rows=None))
    _refused(call(offs=None))
    _refused(call(anchors=None))
    _refused(call(levels=None))
    _refused(call(target=None))
    _refused(call(batch=0))
    _refused(call(num_anchors=0))
    _refused(call(total=-1))
    _refused(call(stride=5))
    _refused(call(n_levels=0))
    _refused(call(levels=(ctypes.c_int32 * 17)(*([5] * 16 + [20])), n_levels=17))
    _refused(call(levels=(ctypes.c_int32 * 3)(60, 0, 40)))
    _refused(call(levels=(ctypes.c_int32 * 3)(60, -30, 70)))
    _refused(call(num_anchors=101))          # the sizes sum to 100
    _refused(call(num_anchors=99))
    _refused(call(topk=0))
    _refused(call(topk=33))
    _refused(call(ws=None))
    _refused(call(nbytes=need - 1))


def test_constructor_and_level_sizes():
    import torch
    from single_shot_detection_amd.detection.target_assigner import AtssTargetAssigner
    assert AtssTargetAssigner().topk == 9 and AtssTargetAssigner(topk=5).topk == 5
    for bad in (0, 33, 2.5, -1):
        with pytest.raises(ValueError):
            AtssTargetAssigner(topk=bad)
    anchors = torch.zeros((10, 4))
    with pytest.raises(ValueError):
        AtssTargetAssigner().encode_ground_truth([torch.zeros((1, 6))], anchors)
    with pytest.raises(ValueError):
        AtssTargetAssigner().encode_ground_truth([torch.zeros((1, 6))], anchors, level_sizes=(6, 3))
    doc = ' '.join(AtssTargetAssigner.__doc__.split())
    assert 'has no positive anchor' in doc and 'NO force stage' in doc


def test_config_name_selects_the_assigner():
    from single_shot_detection_amd.detection import init as det_init, matcher
    from single_shot_detection_amd.detection.target_assigner import AtssTargetAssigner, TargetAssigner
    ta = det_init.build_target_assigner({'matched_threshold': .5, 'unmatched_threshold': .4})
    assert type(ta) is TargetAssigner and ta.force_match == 'per_prediction'       # without the key nothing changes
    assert type(det_init.build_target_assigner({'name': 'TargetAssigner', 'matched_threshold': .5, 'unmatched_threshold': .4})) is TargetAssigner
    atss = det_init.build_target_assigner({'name': 'AtssTargetAssigner', 'topk': 7})
    assert type(atss) is AtssTargetAssigner and atss.topk == 7
    with pytest.raises(ValueError):
        det_init.build_target_assigner({'name': 'Nope'})
    assert callable(matcher.match_atss)


def test_detector_keeps_the_level_sizes_of_what_it_generated():
    import torch
    from single_shot_detection_amd.detection.detector import Detector

    class Gen(object):
        def __init__(self, nb):
            self.nb = nb

        def generate(self, img, source):
            return torch.zeros((source.shape[2], source.shape[3], self.nb, 4))
    det = Detector(None, [], None, [], 3, anchor_generators=[Gen(2), Gen(3)])
    img = torch.zeros((1, 3, 64, 64))
    anchors = det.generate_anchors(img, [torch.zeros((1, 8, 4, 4)), torch.zeros((1, 8, 2, 2))])
    assert anchors.shape == (44, 4) and det.anchor_level_sizes(anchors) == (32, 12)
    other = det.generate_anchors(img, [torch.zeros((1, 8, 2, 2)), torch.zeros((1, 8, 1, 1))])
    assert det.anchor_level_sizes(other) == (8, 3) and det.anchor_level_sizes(anchors) == (32, 12)
    with pytest.raises(ValueError):
        det.anchor_level_sizes(anchors.clone())
