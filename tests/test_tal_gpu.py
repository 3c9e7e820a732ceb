"""GPU: TaskAlignedAssigner / matcher.match_task_aligned (ssdk_encode_ground_truth_tal) against the numpy restatement of the rule that
tests/test_tal.py pins to hand-worked cases.  Every generated case keeps a margin at each of its decisions (checked on the CPU in
tests/tal_cases.py), so ``box_idx`` and target columns 0..4 are compared exactly; column 5 is compared to the fp64 restatement with
atol = 4 x max|fp32 restatement - fp64 restatement| over the case, which every test prints."""
import numpy as np
import pytest
import torch

import tal_cases as tc
from single_shot_detection_amd.detection import matcher
from single_shot_detection_amd.detection.box_coder import BoxCoder, IntegralBoxCoder
from single_shot_detection_amd.detection.target_assigner import PackedGroundTruth, TaskAlignedAssigner

pytestmark = pytest.mark.gpu


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tensors(gt_list):
    return [torch.from_numpy(np.ascontiguousarray(g, np.float32).reshape(-1, 6)) for g in gt_list]


def coder():
    return BoxCoder(tc.XY_SCALE, tc.WH_SCALE)


def encode(gt, anchors, scores, locs, kw, assigner=None, box_coder=None):
    ta = assigner or TaskAlignedAssigner(**kw)
    t, idx = ta.encode_ground_truth(gt if isinstance(gt, PackedGroundTruth) else tensors(gt), anchors, (scores, locs), box_coder or coder(),
                                    return_box_idx=True)
    assert t.is_cuda and t.dtype == torch.float32 and idx.dtype == torch.int32
    return t, idx


def check(name, t, idx, gt, ref_idx, ref_col64, col5_dev):
    """box_idx and columns 0..4 exactly; column 5 within 4 x the fp32 restatement's own deviation from the fp64 one."""
    got_idx, got = idx.cpu().numpy(), t.cpu().numpy()
    assert np.array_equal(got_idx, ref_idx), (name, int((got_idx != ref_idx).sum()))
    ref = tc.target_np(ref_idx, ref_col64, gt)
    assert np.array_equal(bits(got[..., :5]), bits(ref[..., :5].astype(np.float32))), name
    atol = 4.0 * col5_dev
    err = float(np.abs(got[..., 5].astype(np.float64) - ref[..., 5]).max())
    print(f'{name}: positives {int((ref_idx >= 0).sum())}, max|fp32 - fp64| of column 5 = {col5_dev:.3e}, atol = {atol:.3e}, '
          f'max|device - fp64| = {err:.3e}')
    assert err <= atol, (name, err, atol)


def test_hand_worked_grid():
    """The nine hand-worked images as one batch (every logit 0, every predicted box its anchor or off the image: exact arithmetic)."""
    names = list(tc.GRID_CASES)
    gt = [tc.grid_gt(n) for n in names]
    pred = [tc.grid_prediction(n) for n in names]
    scores = np.stack([p[0] for p in pred])
    locs = np.stack([p[1] for p in pred])
    expected = [tc.grid_expected(n) for n in names]
    ref_idx, ref_col = np.stack([e[0] for e in expected]), np.stack([e[1] for e in expected])
    anchors_np = tc.grid_anchors()
    idx32, col32 = tc.tal_np(gt, anchors_np, scores, locs, topk=tc.GRID_TOPK)
    idx64, col64 = tc.tal_np(gt, anchors_np, scores, locs, dtype=np.float64, topk=tc.GRID_TOPK)
    assert np.array_equal(idx32, ref_idx) and np.array_equal(idx64, ref_idx)
    assert np.allclose(col64, ref_col, rtol=1e-6, atol=0)
    t, idx = encode(gt, torch.from_numpy(anchors_np).cuda(), torch.from_numpy(scores).reshape(len(names), -1).cuda(),
                    torch.from_numpy(locs).reshape(len(names), -1).cuda(), dict(topk=tc.GRID_TOPK))
    assert np.array_equal(idx.cpu().numpy(), ref_idx), {n: np.nonzero(r >= 0)[0].tolist() for n, r in zip(names, idx.cpu().numpy())}
    check('grid', t, idx, gt, ref_idx, col64, float(np.abs(col32.astype(np.float64) - col64).max()))


@pytest.mark.parametrize('name', list(tc.GENERATED))
def test_generated_cases_equal_the_restatement(name):
    gt, anchors_np, scores_np, locs_np, kw, fig = tc.generated(name)
    anchors, scores, locs = (torch.from_numpy(x).cuda() for x in (anchors_np, scores_np, locs_np))
    ta = TaskAlignedAssigner(**kw)
    t, idx = encode(gt, anchors, scores, locs, kw, ta)
    check(name, t, idx, gt, fig['idx64'], fig['col64'], fig['col5_dev'])
    t2, idx2 = encode(gt, anchors, scores, locs, kw, ta)                       # two runs: identical bits
    assert torch.equal(idx, idx2) and np.array_equal(bits(t), bits(t2))
    # a PackedGroundTruth whose capacity exceeds its rows (garbage in the padding): the same bits as the list form
    total = sum(len(g) for g in gt)
    packed = PackedGroundTruth.from_list(tensors(gt), anchors.device, capacity=total + 37)
    packed.rows[total:] = torch.from_numpy(np.random.default_rng(5).uniform(1.0, 200.0, (37, 6)).astype(np.float32)).cuda()
    t3, idx3 = encode(packed, anchors, scores, locs, kw, ta)
    assert torch.equal(idx, idx3) and np.array_equal(bits(t), bits(t3))
    # without box_idx: the same target
    t4 = ta.encode_ground_truth(tensors(gt), anchors, (scores, locs), coder())
    assert np.array_equal(bits(t), bits(t4))


def test_one_thread_owns_three_candidates():
    """The sweep thread that owns the first box's three best anchors finds the third by re-reading its anchors (two keys stay in registers)."""
    gt, anchors_np, scores_np, locs_np, kw, fig = tc.one_thread_owns_three_candidates()
    anchors, scores, locs = (torch.from_numpy(x).cuda() for x in (anchors_np, scores_np, locs_np))
    t, idx = encode(gt, anchors, scores, locs, kw)
    assert (fig['idx64'][0, [5, 1029, 2053]] == 0).all()
    check('one_thread_owns_three_candidates', t, idx, gt, fig['idx64'], fig['col64'], fig['col5_dev'])


def test_match_task_aligned_is_row_0_of_the_batch_form():
    gt, anchors_np, scores_np, locs_np, kw, fig = tc.generated('mb2_g32')
    anchors = torch.from_numpy(anchors_np).cuda()
    A = len(anchors_np)
    scores, locs = torch.from_numpy(scores_np[0]).cuda().view(A, -1), torch.from_numpy(locs_np[0]).cuda().view(A, 4)
    g = torch.from_numpy(gt[0]).cuda()
    one = matcher.match_task_aligned(g[:, :4], g[:, 4], anchors, scores, locs, coder(), **kw)
    assert one.dtype == torch.int64 and one.shape == (A,)
    assert np.array_equal(one.cpu().numpy(), fig['idx64'][0])
    none = matcher.match_task_aligned(torch.zeros((0, 4), device='cuda'), torch.zeros((0,), device='cuda'), anchors, scores, locs, coder())
    assert (none == matcher.NOT_MATCHED).all()


def test_integral_box_coder_equals_the_assigner_on_the_integrated_locs():
    gt, anchors_np, scores_np, _, kw, _ = tc.generated('mb2_one_empty')
    anchors, scores = torch.from_numpy(anchors_np).cuda(), torch.from_numpy(scores_np).cuda()
    ibc = IntegralBoxCoder(tc.XY_SCALE, tc.WH_SCALE, reg_max=7, xy_limit=4.0, wh_limit=3.0)
    A = len(anchors_np)
    logits = torch.from_numpy(np.random.default_rng(23).standard_normal((len(gt), A * 4 * ibc.bins), dtype=np.float32) * 2).cuda().requires_grad_(True)
    t, idx = encode(gt, anchors, scores, logits, kw, box_coder=ibc)
    assert not t.requires_grad and logits.grad is None
    with torch.no_grad():
        locs = ibc.integrate(logits, A)
    t2, idx2 = encode(gt, anchors, scores, locs, kw)
    assert (idx >= 0).any() and torch.equal(idx, idx2) and np.array_equal(bits(t), bits(t2))


def test_python_layer_refuses_bad_predictions():
    anchors = torch.from_numpy(tc.grid_anchors()).cuda()
    gt = tensors([tc.grid_gt('box_on_one_cell')])
    scores, locs = torch.zeros((1, 42 * 3), device='cuda'), torch.zeros((1, 42 * 4), device='cuda')
    ta = TaskAlignedAssigner(3)
    with pytest.raises(ValueError):
        ta.encode_ground_truth(gt, anchors, (scores, locs[:, :-4]), coder())
    with pytest.raises(ValueError):
        ta.encode_ground_truth(gt, anchors, (scores[:, :-1], locs), coder())
    with pytest.raises(ValueError):
        ta.encode_ground_truth(gt, anchors, None, coder())
    with pytest.raises(ValueError):
        ta.encode_ground_truth(gt, anchors, (scores, locs), None)


def test_captured_graph_and_detection_init_in_a_child_process():
    """tests/tal_graph_worker.py, in a process of its own (see there): the call captured in a HIP graph and replayed on two batches equals
    the eager results; one training step (eager and with graph_hot_path=True) and one evaluation step through detection.init with
    target_assigner = {'name': 'TaskAlignedAssigner', 'topk': 13}, valid_sampler, QualityFocalLoss(use_iou=False) and the GIoU box term:
    the loss is the existing loss path's on the restatement's target."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, 'tests', 'tal_graph_worker.py')], cwd=repo, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    print(res)
    assert res['timeouts'] == 0
    assert all(np.isfinite(res[k]) for k in ('eager_loss', 'graphed_loss', 'eval_loss')), res
