"""GPU: the integer quantities behind mean average precision -- the (class, score, row) order and the per-prediction outcome
(ssdk_mean_average_precision_ex, csrc/metrics.hip) -- EXACTLY equal to the plain model of tests/map_reference.py, on the directed inputs
of tests/map_cases.py: several sort tiles, wide image ids, the whole float range of scores, map_ap_kernel's 256-wide rounds, every
ground-truth row width, (image, class) groups at a tile boundary.  AP and mAP against the float64 model at 2e-6.
test_map_reference.py (CPU) ties the model to the recorded values of the reference project and to the oracle."""
import numpy as np
import pytest
import torch

import map_cases
import map_reference as mr
from single_shot_detection_amd import _lib
from single_shot_detection_amd.detection.metrics.mean_average_precision import average_precisions

pytestmark = pytest.mark.gpu

AP_TOL = 2e-6


def check(name, voc, got):
    pred, gts, num_classes = map_cases.case(name)
    m_ref, ap_ref, order_ref, outcome_ref = map_cases.reference(name, voc)
    m, ap, order, outcome = got
    order, outcome = np.asarray(order), np.asarray(outcome)
    bad = np.flatnonzero(order != order_ref)
    assert bad.size == 0, f'{name}: order differs at {bad.size} positions, first {bad[:5]}: device rows {order[bad[:5]]}, reference rows {order_ref[bad[:5]]}'
    bad = np.flatnonzero(outcome != outcome_ref)
    assert bad.size == 0, f'{name}: outcome differs for {bad.size} rows, first {bad[:5]}: device {outcome[bad[:5]]}, reference {outcome_ref[bad[:5]]}'
    np.testing.assert_allclose(np.asarray(ap, np.float64), ap_ref, atol=AP_TOL, rtol=0, equal_nan=True)
    assert (np.isnan(m) and np.isnan(m_ref)) or abs(m - m_ref) <= AP_TOL, (m, m_ref)


def run_wrapper(name, voc):
    pred, gts, num_classes = map_cases.case(name)
    m, ap, order, outcome = average_precisions(torch.from_numpy(pred), [torch.from_numpy(g) for g in gts], num_classes, 0.5, voc=voc, details=True)
    return m, ap.numpy(), order.numpy(), outcome.numpy()


def run_ex(name, voc, with_details=True):
    """ssdk_mean_average_precision_ex called directly on numpy-built packed rows and offsets"""
    lib = _lib.lib()
    pred, gts, num_classes = map_cases.case(name)
    rows, offs = mr.pack(gts)
    n, total = len(pred), len(rows)
    d_pred, d_rows, d_offs = torch.from_numpy(pred).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(offs).cuda()
    ws = torch.empty((max(lib.ssdk_mean_average_precision_workspace_bytes(n, total, num_classes), 256),), dtype=torch.uint8, device='cuda')
    ap = torch.empty((num_classes,), dtype=torch.float32, device='cuda')
    mean = torch.empty((1,), dtype=torch.float64, device='cuda')
    order = torch.full((n,), -1, dtype=torch.int32, device='cuda')
    outcome = torch.full((n,), 255, dtype=torch.uint8, device='cuda')
    _lib.check(lib.ssdk_mean_average_precision_ex(_lib.ptr(d_pred), n, _lib.ptr(d_rows), rows.shape[1], _lib.ptr(d_offs), len(gts), total, num_classes, 0.5,
                                                  int(voc), _lib.ptr(ap), _lib.ptr(mean), _lib.ptr(order) if with_details else None,
                                                  _lib.ptr(outcome) if with_details else None, _lib.ptr(ws), ws.numel(), _lib.current_stream()),
               'ssdk_mean_average_precision_ex')
    return float(mean.item()), ap.cpu().numpy(), order.cpu().numpy().astype(np.int64), outcome.cpu().numpy()


@pytest.mark.parametrize('voc', [False, True])
@pytest.mark.parametrize('name', ['across_tiles', 'score_range', 'segment_edges', 'segment_edges_difficult_head', 'gt_width_5', 'gt_width_6', 'gt_width_7',
                                  'gt_width_9', 'head_at_tile_boundary', 'group_across_tile_boundary'])
def test_order_and_outcomes_exact(name, voc):
    check(name, voc, run_wrapper(name, voc))


@pytest.mark.parametrize('voc', [False, True])
def test_wide_image_ids_exact(voc):
    """66 000 images: image keys with three non-trivial digits, and ids outside [0, num_images) (false positives)"""
    check('wide_image_ids', voc, run_ex('wide_image_ids', voc))


def test_outputs_are_optional_and_the_old_entry_agrees():
    name = 'gt_width_7'
    full = run_ex(name, False)
    check(name, False, full)
    m, ap, order, outcome = run_ex(name, False, with_details=False)
    assert np.all(order == -1) and np.all(outcome == 255)                 # two NULLs: nothing else is written
    assert np.array_equal([m], [full[0]], equal_nan=True) and np.array_equal(ap, full[1], equal_nan=True)
    pred, gts, num_classes = map_cases.case(name)
    m_old, ap_old = average_precisions(torch.from_numpy(pred), [torch.from_numpy(g) for g in gts], num_classes, 0.5, voc=False)
    assert np.array_equal([m_old], [full[0]], equal_nan=True) and np.array_equal(ap_old.numpy(), full[1], equal_nan=True)
