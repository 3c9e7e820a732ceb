"""GPU: matcher.match_bipartite (ssdk_match_bipartite) and TargetAssigner(force_match='bipartite') (ssdk_encode_ground_truth_ex) against
the reference's own outputs (tests/golden/bipartite.npz) and, on randomised cases, against the numpy restatement that
tests/test_bipartite.py pins to those outputs.  Everything is exact."""
import numpy as np
import pytest
import torch

import bipartite_cases as bc
from single_shot_detection_amd import synthetic as syn
from single_shot_detection_amd.detection import matcher
from single_shot_detection_amd.detection.target_assigner import PackedGroundTruth, TargetAssigner

pytestmark = pytest.mark.gpu


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope='module')
def golden():
    return bc.load_golden()


def tensors(gt_list):
    return [torch.from_numpy(g) for g in gt_list]


# ---- the matrix form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(bc.MATRIX_CASES))
def test_match_bipartite_equals_the_reference(golden, name):
    w_np = bc.MATRIX_CASES[name]()
    ref = golden[f'matrix/{name}/anchor_idx']
    defined = golden[f'matrix/{name}/defined'] if name in bc.EXHAUSTED else np.ones(len(ref), bool)
    for inplace in (False, True):
        w = torch.from_numpy(w_np.copy()).cuda()
        box_idx, anchor_idx = matcher.match_bipartite(w, inplace=inplace)
        assert box_idx.dtype == anchor_idx.dtype == torch.int64 and box_idx.is_cuda and anchor_idx.is_cuda
        assert np.array_equal(box_idx.cpu().numpy(), golden[f'matrix/{name}/box_idx'])
        got = anchor_idx.cpu().numpy()
        assert np.array_equal(got[defined], ref[defined]), (name, inplace)
        assert (got[~defined] == -1).all(), (name, inplace)
        left = golden[f'matrix/{name}/inplace'] if inplace else w_np
        assert np.array_equal(bits(w), bits(left)), (name, inplace)


def test_match_bipartite_asserts_a_positive_entry_in_every_row():
    w = torch.tensor([[0.5, 0.2], [0.0, 0.0]], device='cuda')
    with pytest.raises(AssertionError):
        matcher.match_bipartite(w)
    w[1, 0] = float('nan')
    with pytest.raises(AssertionError):
        matcher.match_bipartite(w)
    with pytest.raises(ValueError):
        matcher.match_bipartite(torch.zeros((0, 4), device='cuda'))


def test_match_bipartite_random_matrices_equal_the_restatement():
    """Shapes around the 1 024-thread sweep and with negative entries (they lose to the zeros the loop writes)."""
    rng = np.random.default_rng(77)
    for g, a in ((1, 1), (2, 1025), (17, 64), (33, 2049), (70, 40)):
        w = (rng.random((g, a), dtype=np.float32) - np.float32(0.2)) * (rng.random((g, a)) < 0.5)
        w = np.round(w * 8) / np.float32(8)
        w[np.arange(g), rng.integers(0, a, g)] = 0.5
        w = np.ascontiguousarray(w, np.float32)
        ref_idx, ref_left = bc.match_bipartite_np(w)
        t = torch.from_numpy(w.copy()).cuda()
        _, anchor_idx = matcher.match_bipartite(t, inplace=True)
        assert np.array_equal(anchor_idx.cpu().numpy(), ref_idx), (g, a)
        assert np.array_equal(bits(t), bits(ref_left)), (g, a)


# ---- the fused form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(bc.FUSED_CASES))
def test_fused_bipartite_equals_the_reference(golden, name):
    gt, anchors_np, mt, ut = bc.fused_inputs(name)
    ref_idx = golden[f'fused/{name}/box_idx']
    ref_target = bc.target_from_box_idx(ref_idx, gt)
    anchors = torch.from_numpy(anchors_np).cuda()
    ta = TargetAssigner(mt, ut, force_match='bipartite')
    t, idx = ta.encode_ground_truth(tensors(gt), anchors, return_box_idx=True)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), ref_idx)
    assert np.array_equal(bits(t), bits(ref_target))
    total = sum(len(g) for g in gt)
    packed = PackedGroundTruth.from_list(tensors(gt), anchors.device, capacity=total + 37)
    packed.rows[total:] = torch.from_numpy(np.random.default_rng(5).uniform(1.0, 200.0, (37, 6)).astype(np.float32)).cuda()   # garbage padding
    t, idx = ta.encode_ground_truth(packed, anchors, return_box_idx=True)
    assert np.array_equal(idx.cpu().numpy(), ref_idx)
    assert np.array_equal(bits(t), bits(ref_target))


def test_modes_on_the_first_fused_case():
    gt, anchors_np, mt, ut = bc.fused_inputs('mb2_g32')
    anchors = torch.from_numpy(anchors_np).cuda()
    t_def, idx_def = TargetAssigner(mt, ut).encode_ground_truth(tensors(gt), anchors, return_box_idx=True)
    t_pp, idx_pp = TargetAssigner(mt, ut, force_match='per_prediction').encode_ground_truth(tensors(gt), anchors, return_box_idx=True)
    assert torch.equal(idx_def, idx_pp) and np.array_equal(bits(t_def), bits(t_pp))
    import oracle
    ref_t, ref_idx = oracle.encode_ground_truth(gt, anchors_np, mt, ut, return_box_idx=True)
    assert np.array_equal(idx_pp.cpu().numpy(), ref_idx) and np.array_equal(bits(t_pp), bits(ref_t))
    _, idx_b = TargetAssigner(mt, ut, force_match='bipartite').encode_ground_truth(tensors(gt), anchors, return_box_idx=True)
    assert (idx_b != idx_pp).any()
    corners = oracle.to_corners(anchors_np)
    idx_b = idx_b.cpu().numpy()
    for i, g in enumerate(gt):
        # an anchor is forced where it is positive although the threshold stage alone would not give it to that box
        nf = np.asarray(oracle.match_per_prediction(oracle.iou(np.ascontiguousarray(g[:, :4]), corners), mt, ut, False))
        forced_boxes = idx_b[i][idx_b[i] != nf]
        positives = np.bincount(idx_b[i][idx_b[i] >= 0], minlength=len(g))
        assert (positives >= 1).all(), i                                   # every box is trained on
        assert len(set(forced_boxes.tolist())) == len(forced_boxes), i     # at most one forced anchor per box
    # match_boxes: one image
    one = matcher.match_boxes(torch.from_numpy(gt[2][:, :4]).cuda(), anchors, mt, ut, force_match='bipartite')
    assert one.dtype == torch.int64 and np.array_equal(one.cpu().numpy(), idx_b[2])
    assert np.array_equal(matcher.match_boxes(torch.from_numpy(gt[2][:, :4]).cuda(), anchors, mt, ut).cpu().numpy(), ref_idx[2])


def _crowded(rng, size, g):
    """g boxes with duplicates and nested boxes: chains of collisions."""
    if g == 0:
        return np.zeros((0, 6), np.float32)
    base = syn.make_ground_truth(1, size, 21, seed=int(rng.integers(1 << 30)), fixed_g=g)[0]
    for k in range(g):
        kind, src = rng.integers(0, 4), int(rng.integers(0, g))
        if kind == 0:
            base[k, :4] = base[src, :4]                                                   # duplicate
        elif kind == 1:
            x1, y1, x2, y2 = base[src, :4]
            base[k, :4] = [x1 + (x2 - x1) * 0.02, y1 + (y2 - y1) * 0.02, x2 - (x2 - x1) * 0.02, y2 - (y2 - y1) * 0.02]   # nested
    return base.astype(np.float32)


def test_fused_bipartite_random_cases_equal_the_restatement():
    anchors_np = np.load(bc.GOLDEN + '/ssd_mb2_voc.npz')['anchors']
    anchors = torch.from_numpy(anchors_np).cuda()
    rng = np.random.default_rng(123)
    ta = TargetAssigner(0.5, 0.4, force_match='bipartite')
    collisions = 0
    for case in range(30):
        gt = [_crowded(rng, 300, int(rng.integers(0, 41))) for _ in range(int(rng.integers(1, 4)))]
        ref_idx = bc.encode_bipartite_np(gt, anchors_np, 0.5, 0.4)
        t, idx = ta.encode_ground_truth(tensors(gt), anchors, return_box_idx=True)
        assert np.array_equal(idx.cpu().numpy(), ref_idx), case
        assert np.array_equal(bits(t), bits(bc.target_from_box_idx(ref_idx, gt))), case
        import oracle
        collisions += sum(len(bc.lost_forced_anchor(oracle.iou(np.ascontiguousarray(g[:, :4]), oracle.to_corners(anchors_np)))) for g in gt if len(g))
    assert collisions > 30   # (the cases do what they are for)


def test_fused_bipartite_exhaustion_and_more_boxes_than_fit_in_lds():
    """Few anchors, many boxes: the stage stops when the anchors the remaining boxes overlap are all taken -- no box is forced onto
    anchor 0 (unlike match_bipartite).  And 1 100 boxes in one image: beyond the 1 024 whose keys the resolve kernel keeps in LDS."""
    anchors_np = np.load(bc.GOLDEN + '/ssd_mb2_voc.npz')['anchors']
    few = np.ascontiguousarray(anchors_np[1444:2044:25])    # 24 anchors spread over the 10 x 10 level
    gt = syn.make_ground_truth(2, 300, 21, seed=3, fixed_g=40)
    ref_idx = bc.encode_bipartite_np(gt, few, 0.5, 0.4)
    assert all((np.bincount(r[r >= 0], minlength=40) == 0).any() for r in ref_idx)        # boxes are left over
    _, idx = TargetAssigner(0.5, 0.4, force_match='bipartite').encode_ground_truth(tensors(gt), torch.from_numpy(few).cuda(), return_box_idx=True)
    assert np.array_equal(idx.cpu().numpy(), ref_idx)
    gt = syn.make_ground_truth(1, 300, 21, seed=6, fixed_g=1100) + syn.make_ground_truth(1, 300, 21, seed=7, fixed_g=9)
    ref_idx = bc.encode_bipartite_np(gt, anchors_np, 0.5, 0.4)
    t, idx = TargetAssigner(0.5, 0.4, force_match='bipartite').encode_ground_truth(tensors(gt), torch.from_numpy(anchors_np).cuda(), return_box_idx=True)
    assert np.array_equal(idx.cpu().numpy(), ref_idx)
    assert np.array_equal(bits(t), bits(bc.target_from_box_idx(ref_idx, gt)))


def test_captured_graph_and_detection_init_in_a_child_process():
    """tests/bipartite_graph_worker.py, in a process of its own (see there): encode_ground_truth in bipartite mode inside torch.cuda.graph
    on a PackedGroundTruth, replayed twice with update_ in between, equals the eager results; a config's target_assigner = {...,
    'force_match': 'bipartite'} reaches the TargetAssigner through detection.init (ssd_mb2_voc, batch 2): one train step, eager and with
    graph_hot_path=True, finite loss equal to the oracle's on the restatement's target, finite gradients."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, 'tests', 'bipartite_graph_worker.py')], cwd=repo, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert res['timeouts'] == 0
    assert np.isfinite(res['eager_loss']) and np.isfinite(res['graphed_loss']), res
