"""Child process of tests/test_bipartite_gpu.py: the checks of force_match='bipartite' that capture HIP graphs or build a whole detector
(encode_ground_truth inside torch.cuda.graph; detection.init eager and with graph_hot_path=True).  They run in a process of their own
so that what they leave behind -- captured graphs and their memory pools, per-stream workspaces, a detector's worth of cached
allocations -- never becomes the starting state of the test files that follow in the suite's process.  Every check asserts here; one
JSON line with the figures is printed at the end.  Usage: python tests/bipartite_graph_worker.py"""
import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bipartite_cases as bc                                                                                   # noqa: E402
import oracle                                                                                                  # noqa: E402
from single_shot_detection_amd import _lib, synthetic as syn                                                   # noqa: E402
from single_shot_detection_amd.detection.target_assigner import PackedGroundTruth, TargetAssigner             # noqa: E402


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tensors(gt_list):
    return [torch.from_numpy(g) for g in gt_list]


def fused_bipartite_in_a_captured_graph():
    """encode_ground_truth in bipartite mode inside torch.cuda.graph on a PackedGroundTruth of fixed capacity: two replays, update_ in
    between, equal the eager results."""
    gt_a, anchors_np, mt, ut = bc.fused_inputs('mb2_g32')
    gt_b = syn.make_ground_truth(4, 300, 21, seed=8, fixed_g=20)
    gt_b[1] = np.zeros((0, 6), np.float32)
    anchors = torch.from_numpy(anchors_np).cuda()
    ta = TargetAssigner(mt, ut, force_match='bipartite')
    eager = [ta.encode_ground_truth(tensors(g), anchors, return_box_idx=True) for g in (gt_a, gt_b)]
    packed = PackedGroundTruth.from_list(tensors(gt_a), anchors.device, capacity=4 * 32 + 5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ta.encode_ground_truth(packed, anchors, return_box_idx=True)      # warm-up: the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        t, idx = ta.encode_ground_truth(packed, anchors, return_box_idx=True)
    for gt, (ref_t, ref_idx) in zip((gt_a, gt_b), eager):
        packed.update_(tensors(gt))
        t.fill_(7.0)
        idx.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx, ref_idx) and np.array_equal(bits(t), bits(ref_t))


MB2 = {
    'base': {'name': 'torchvision_mobilenet_v2', 'pretrained': False},
    'detector': {'num_classes': 21, 'use_depthwise': True, 'features': {'name': 'Features', 'out_layers': (13, 18)},
                 'extras': {'layers': (('s', 512), ('s', 256), ('s', 256), ('s', 128))}},
    'anchor_generator': {'type': 'ssd', 'num_scales': 6, 'min_scale': 0.1, 'max_scale': 1.05,
                         'aspect_ratios': [[1.0, 2.0]] + [[1.0, 2.0, 3.0]] * 3 + [[1.0, 2.0]] * 2},
}


def detection_init_with_bipartite_force_match_trains(graph_hot_path):
    """A config's target_assigner = {..., 'force_match': 'bipartite'} reaches the TargetAssigner through detection.init (ssd_mb2_voc, batch
    2): one train step, the loss is the oracle's on the restatement's target; with graph_hot_path=True the step is captured as before."""
    from single_shot_detection_amd.detection import init as det_init
    torch.manual_seed(9)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, copy.deepcopy(MB2), {'xy_scale': 10.0, 'wh_scale': 5.0},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SOFTMAX'},
        {'classification_loss': {'name': 'CrossEntropyLoss'}, 'localization_loss': {'name': 'SmoothL1Loss'},
         'classification_weight': 1.0, 'localization_weight': 1.0},
        {'name': 'hard_negative_mining', 'negative_per_positive_ratio': 3, 'min_negative_per_image': 5},
        {'matched_threshold': 0.5, 'unmatched_threshold': 0.5, 'force_match': 'bipartite'}, graph_hot_path=graph_hot_path)
    wrapper.model.train()
    imgs = torch.from_numpy(np.random.default_rng(31).standard_normal((2, 3, 300, 300), dtype=np.float32))
    gt_np = syn.make_ground_truth(2, 300, 21, seed=1, fixed_g=32)
    loss, (scores, locs), _ = step_fn(0, 'train', (imgs, tensors(gt_np)), init_state())
    assert torch.isfinite(loss).all()
    assert bool(step_fn.hot_segments) == graph_hot_path
    anchors = np.load(bc.GOLDEN + '/ssd_mb2_voc.npz')['anchors']
    target = bc.target_from_box_idx(bc.encode_bipartite_np(gt_np, anchors, 0.5, 0.5), gt_np)
    s_np, l_np = scores.detach().cpu().numpy(), locs.detach().cpu().numpy()
    mask = oracle.hard_negative_mining(s_np, target, 3, 5)
    vals, _, _ = oracle.multibox_loss(s_np, l_np, anchors, target, mask, kind='ce', grads=False)
    assert abs(loss.item() - vals[0]) <= 1e-4 + 1e-5 * abs(vals[0]), (loss.item(), vals)
    loss.backward()
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in wrapper.model.parameters())
    return float(loss.detach()), float(vals[0])


def main():
    res = {}
    fused_bipartite_in_a_captured_graph()
    res['captured_graph'] = 'two replays equal the eager results'
    res['eager_loss'], res['eager_oracle_loss'] = detection_init_with_bipartite_force_match_trains(False)
    res['graphed_loss'], res['graphed_oracle_loss'] = detection_init_with_bipartite_force_match_trains(True)
    torch.cuda.synchronize()
    res['timeouts'] = _lib.streamk_timeouts()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
