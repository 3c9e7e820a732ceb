"""CPU: the numpy restatement of the COCO rules (tests/coco_eval_reference.py) against values worked by hand, the builders' conditions of
every case the GPU file uses, and the refusals of the API that need no GPU.  The device code is tested in tests/test_coco_eval_gpu.py."""
import ctypes

import numpy as np
import pytest

import coco_eval_cases as cases
import coco_eval_reference as ref
from single_shot_detection_amd import _lib
from single_shot_detection_amd.detection.metrics import coco_evaluation as api_function
from single_shot_detection_amd.detection.metrics.coco_evaluation import STAT_NAMES, check_tables, default_tables, summary_lines

HAND = cases.hand_cases()


def run(c):
    return ref.evaluate(c['pred'], c['gts'], c['num_classes'], **cases.reference_kwargs(c))


@pytest.mark.parametrize('name', sorted(HAND))
def test_reference_gives_the_hand_worked_statistics(name):
    c, want = HAND[name]
    got = run(c)['stats']
    assert set(got) == set(STAT_NAMES) == set(want)
    for k in STAT_NAMES:
        assert abs(got[k] - want[k]) <= 1e-12, (name, k, got[k], want[k])


def flag_table(c, row):
    """flags of one detection as a [T, A] array"""
    out = run(c)
    T = len(default_tables()[0])
    return out['flags'][row].reshape(T, -1)


def test_iou_078_matches_at_six_thresholds():
    f = flag_table(HAND['iou_078'][0], 0)
    assert (f[:, 0] & 1).tolist() == [1] * 6 + [0] * 4
    # area 7800 is medium: unmatched it is ignored for 'large', matched it inherits the (counted) gt
    assert f[:, 3].tolist() == [1] * 6 + [2] * 4
    assert f[:, 2].tolist() == [3] * 6 + [0] * 4          # the gt (area 10000) is ignored for 'medium'; the detection itself lies inside


def test_exact_half_matches_at_half():
    f = flag_table(HAND['iou_half'][0], 0)
    assert (f[:, 0] & 1).tolist() == [1] + [0] * 9


def test_crowd_rules():
    c = HAND['crowd'][0]
    out = run(c)
    f = out['flags'].reshape(3, 10, 4)
    assert (f[0, :, 0] == 3).all() and (f[1, :, 0] == 3).all()     # both inside the crowd region: matched and ignored, neither tp nor fp
    assert (f[2, :, 0] == 1).all()                                 # the counted gt is preferred to the crowd's larger IoU (the break rule)
    assert out['npig'][1].tolist() == [1, 0, 1, 0]


def test_equal_ious_take_the_later_gt():
    f = run(HAND['equal_iou'][0])['flags'].reshape(2, 10, 4)
    assert f[0, :, 0].tolist() == [1] + [0] * 9
    assert (f[1, :, 0] == 1).all()                                 # at t = 0.5 the earlier gt is still free for the second detection


def test_the_cap_cuts_rank_100():
    out = run(HAND['cap_101'][0])
    assert out['rank'].tolist() == list(range(101))
    assert not out['flags'][100].any() and out['recall'][:, 1, 0, 2].tolist() == [0.0] * 10


def test_bounds_are_inclusive_and_unmatched_outside_is_ignored():
    assert run(HAND['area_1024'][0])['npig'][1].tolist() == [1, 1, 1, 0]
    f = run(HAND['unmatched_outside'][0])['flags'].reshape(2, 10, 4)
    assert (f[0, :, 0] == 0).all() and (f[0, :, 1] == 0).all()     # inside 'all' and 'small': a false positive
    assert (f[0, :, 2] == 2).all() and (f[0, :, 3] == 2).all()     # outside 'medium' and 'large': ignored


def test_equal_scores_order_by_image_then_row():
    out = run(HAND['tie_images'][0])
    assert out['order'].tolist() == [1, 0]


def test_gt_areas_and_image_scale_move_boxes_between_bins():
    c = HAND['gt_area'][0]
    assert run(c)['npig'][1].tolist() == [1, 1, 0, 0]
    assert run(dict(c, gt_areas=None))['npig'][1].tolist() == [1, 0, 0, 1]
    c = HAND['area_scale'][0]
    assert run(c)['npig'][1].tolist() == [1, 0, 0, 1]
    assert run(dict(c, image_area_scale=None))['npig'][1].tolist() == [1, 1, 0, 0]


def test_custom_tables_without_the_named_entries():
    c = dict(HAND['iou_078'][0], iou_thrs=np.array([0.6, 0.7]), area_rngs=np.array([[0.0, 1e10]]), max_dets=np.array([5], np.int32))
    s = run(c)['stats']
    assert abs(s['AP'] - 1.0) <= 1e-12 and s['AR1'] == 1.0          # (precision is 1 / (1 + 2^-52))
    assert [s[k] for k in ('AP50', 'AP75', 'APs', 'APm', 'APl', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')] == [-1.0] * 10


@pytest.mark.parametrize('name', sorted(cases.gpu_cases()))
def test_builders_conditions_hold(name):
    c = cases.gpu_cases()[name]
    assert cases.off_thresholds(c), name
    assert c['pred'].dtype == np.float32 and c['pred'].shape[1] == 7
    if name.startswith(('random_', 'group_')) and name != 'random_score_ties':
        assert np.unique(c['pred'][:, 6]).size == c['pred'].shape[0]


def test_the_shapes_the_gpu_cases_are_meant_to_reach():
    g = cases.gpu_cases()
    big = g['random_past_a_tile']
    assert big['pred'].shape[0] > 4096 and len(big['gts']) == 400
    s = g['random_score_ties']['pred'][:, 6]
    assert np.unique(s).size < s.size / 2
    assert any(gt.shape[1] == 7 and gt[:, 6].any() for gt in g['random_small_crowd']['gts'])
    assert all(gt.shape[1] == 6 for gt in g['random_no_flag_column']['gts'])
    for n_det, n_gt in cases.GROUP_SHAPES:
        c = g[f'group_{n_det}_dets_{n_gt}_gts']
        assert int(((c['pred'][:, 0] == 0) & (c['pred'][:, 5] == 1)).sum()) == n_det and int((c['gts'][0][:, 4] == 1).sum()) == n_gt
        assert n_gt < 5 or c['gts'][0][:, 6].any()


# ---- refusals that need no GPU ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [
    dict(iou_thresholds=np.linspace(.3, .95, 13), area_ranges=np.tile([[0.0, 1e10]], (5, 1))),     # T * A = 65
    dict(max_detections=(100, 10, 1)),
    dict(max_detections=(1, 1, 10)),
    dict(max_detections=(0, 10)),
    dict(max_detections=(1, 2, 3, 4, 5)),
    dict(recall_thresholds=np.zeros(0)),
    dict(recall_thresholds=np.linspace(0, 1, 1025)),
    dict(iou_thresholds=[]),
    dict(area_ranges=np.zeros((0, 2))),
    dict(area_ranges=np.zeros((4, 3))),
])
def test_python_api_refuses_unsupported_tables(kw):
    full = dict(iou_thresholds=None, recall_thresholds=None, area_ranges=None, max_detections=(1, 10, 100))
    full.update(kw)
    with pytest.raises(ValueError):
        check_tables(**full)
    import torch
    with pytest.raises(ValueError):   # refused before anything touches a device
        api_function(torch.zeros((0, 7)), [], {0: 'a'}, verbose=False, **kw)


@pytest.mark.parametrize('T,A,M,R,max_dets', [(13, 5, 3, 101, (1, 10, 100)), (10, 4, 3, 101, (100, 10, 1)), (10, 4, 3, 0, (1, 10, 100)),
                                              (10, 4, 5, 101, (1, 2, 3, 4, 5)), (10, 4, 3, 1025, (1, 10, 100)), (0, 4, 3, 101, (1, 10, 100))])
def test_c_abi_refuses_unsupported_tables(T, A, M, R, max_dets):
    """SSDK_E_INVALID before any launch: the call returns on the host, so it can be made without a GPU (the buffers are never touched)."""
    lib = _lib.lib()
    host = np.zeros(4096, np.float64)
    p = ctypes.c_void_p(host.ctypes.data)
    md = np.asarray(max_dets, np.int32)
    rc = lib.ssdk_coco_eval(p, 0, p, 6, p, 0, 0, 3, None, None, p, T, p, R, p, A, ctypes.c_void_p(md.ctypes.data), M, p, p, p, p, 1 << 20, None)
    assert rc == -1, rc
    assert b'ssdk_coco_eval' in lib.ssdk_last_error_string()
    assert not host.any()


def test_workspace_size_of_refused_shapes_is_zero():
    lib = _lib.lib()
    assert lib.ssdk_coco_eval_workspace_bytes(10, 10, 3, 13, 5) == 0
    assert lib.ssdk_coco_eval_workspace_bytes(-1, 10, 3, 10, 4) == 0
    small, large = lib.ssdk_coco_eval_workspace_bytes(10, 10, 3, 10, 4), lib.ssdk_coco_eval_workspace_bytes(100000, 10, 3, 10, 4)
    assert 0 < small < large


def test_summary_lines_use_the_published_wording():
    iou, _, area, md = default_tables()
    lines = summary_lines({k: 0.5 for k in STAT_NAMES}, iou, area, md)
    assert lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500'
    assert lines[1] == ' Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.500'
    assert lines[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.500'
    assert lines[11] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 0.500'
