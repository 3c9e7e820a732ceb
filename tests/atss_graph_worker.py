"""Child process of tests/test_atss_gpu.py: the checks of AtssTargetAssigner that capture HIP graphs or build a whole detector
(encode_ground_truth inside torch.cuda.graph; detection.init with target_assigner = {'name': 'AtssTargetAssigner', ...}, eager, with
graph_hot_path=True, and one evaluation step).  They run in a process of their own for the reasons tests/bipartite_graph_worker.py gives.
Every check asserts here; one JSON line with the figures is printed at the end.  Usage: python tests/atss_graph_worker.py"""
import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import atss_cases as ac                                                                                        # noqa: E402
import oracle                                                                                                  # noqa: E402
from bipartite_graph_worker import MB2                                                                         # noqa: E402
from single_shot_detection_amd import _lib, synthetic as syn                                                   # noqa: E402
from single_shot_detection_amd.detection.target_assigner import AtssTargetAssigner, PackedGroundTruth         # noqa: E402


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tensors(gt_list):
    return [torch.from_numpy(g) for g in gt_list]


def atss_in_a_captured_graph():
    """encode_ground_truth inside torch.cuda.graph on a PackedGroundTruth of fixed capacity: two replays, update_ in between, equal the
    eager results (and the restatement)."""
    gt_a, anchors_np, levels, topk, ref_a, _ = ac.generated('mb2_g32')
    gt_b, _, _, _, ref_b, _ = ac.generated('mb2_default_one_empty')
    anchors = torch.from_numpy(anchors_np).cuda()
    ta = AtssTargetAssigner(topk)
    eager = [ta.encode_ground_truth(tensors(g), anchors, return_box_idx=True, level_sizes=levels) for g in (gt_a, gt_b)]
    packed = PackedGroundTruth.from_list(tensors(gt_a), anchors.device, capacity=4 * 32 + 5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ta.encode_ground_truth(packed, anchors, return_box_idx=True, level_sizes=levels)      # warm-up: the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        t, idx = ta.encode_ground_truth(packed, anchors, return_box_idx=True, level_sizes=levels)
    for gt, (ref_t, ref_idx), ref_np in zip((gt_a, gt_b), eager, (ref_a, ref_b)):
        packed.update_(tensors(gt))
        t.fill_(7.0)
        idx.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx, ref_idx) and np.array_equal(bits(t), bits(ref_t))
        assert np.array_equal(idx.cpu().numpy(), ref_np)


def detection_init_with_the_atss_assigner(graph_hot_path, phase='train'):
    """target_assigner = {'name': 'AtssTargetAssigner', 'topk': 9} reaches the class through detection.init (ssd_mb2_voc, batch 2), which
    hands it the detector's level sizes: one step; the target of the eager line is the restatement's, the loss is the oracle's on it."""
    from single_shot_detection_amd.detection import init as det_init
    torch.manual_seed(9)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, copy.deepcopy(MB2), {'xy_scale': 10.0, 'wh_scale': 5.0},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SOFTMAX'},
        {'classification_loss': {'name': 'CrossEntropyLoss'}, 'localization_loss': {'name': 'SmoothL1Loss'},
         'classification_weight': 1.0, 'localization_weight': 1.0},
        {'name': 'hard_negative_mining', 'negative_per_positive_ratio': 3, 'min_negative_per_image': 5},
        {'name': 'AtssTargetAssigner', 'topk': 9}, graph_hot_path=graph_hot_path)
    imgs = torch.from_numpy(np.random.default_rng(31).standard_normal((2, 3, 300, 300), dtype=np.float32))
    gt_np = syn.make_ground_truth(2, 300, 21, seed=1, fixed_g=32)
    anchors = np.load(ac.GOLDEN + '/ssd_mb2_voc.npz')['anchors']
    levels = ac.config_level_sizes('ssd_mb2_voc')
    ref_idx, margin = ac.atss_np(gt_np, anchors, levels, 9)
    assert margin >= ac.MIN_MARGIN
    target = ac.target_from_box_idx(ref_idx, gt_np)

    seen = []
    encode = AtssTargetAssigner.encode_ground_truth

    def recording(self, *args, **kwargs):
        out = encode(self, *args, **kwargs)
        # (a copy: the loss encodes the boxes of the target in place; none while a segment is captured)
        seen.append((None if torch.cuda.is_current_stream_capturing() else out.clone(), kwargs.get('level_sizes')))
        return out
    AtssTargetAssigner.encode_ground_truth = recording
    try:
        if phase == 'train':
            wrapper.model.train()
            loss, (scores, locs), _ = step_fn(0, 'train', (imgs, tensors(gt_np)), init_state())
        else:
            wrapper.model.eval()
            with torch.no_grad():
                s0, l0, _ = wrapper.model(imgs.to(dev))       # (the evaluation step returns detections, not the raw prediction)
                loss, detections, _ = step_fn(0, 'eval', (imgs, tensors(gt_np)), init_state())
            scores, locs = s0, l0
            assert detections is not None
    finally:
        AtssTargetAssigner.encode_ground_truth = encode
    assert torch.isfinite(loss).all()
    assert bool(step_fn.hot_segments) == graph_hot_path
    assert seen and all(tuple(lv) == levels for _, lv in seen)
    if not graph_hot_path:      # (a captured segment's target lives in the graph's pool and is recycled by the backward pass)
        assert np.array_equal(bits(seen[-1][0]), bits(target))
    s_np, l_np = scores.detach().cpu().numpy(), locs.detach().cpu().numpy()
    mask = oracle.hard_negative_mining(s_np, target, 3, 5)
    vals, _, _ = oracle.multibox_loss(s_np, l_np, anchors, target, mask, kind='ce', grads=False)
    assert abs(loss.item() - vals[0]) <= 1e-4 + 1e-5 * abs(vals[0]), (loss.item(), vals)
    if phase == 'train':
        loss.backward()
        assert all(p.grad is None or torch.isfinite(p.grad).all() for p in wrapper.model.parameters())
    return float(loss.detach()), float(vals[0])


def main():
    res = {}
    atss_in_a_captured_graph()
    res['captured_graph'] = 'two replays equal the eager results'
    res['eager_loss'], res['eager_oracle_loss'] = detection_init_with_the_atss_assigner(False)
    res['graphed_loss'], res['graphed_oracle_loss'] = detection_init_with_the_atss_assigner(True)
    res['eval_loss'], res['eval_oracle_loss'] = detection_init_with_the_atss_assigner(False, phase='eval')
    torch.cuda.synchronize()
    res['timeouts'] = _lib.streamk_timeouts()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
