"""Child process of tests/test_tal_gpu.py: the checks of TaskAlignedAssigner that capture HIP graphs or build a whole detector
(encode_ground_truth inside torch.cuda.graph; detection.init with target_assigner = {'name': 'TaskAlignedAssigner', 'topk': 13},
valid_sampler, QualityFocalLoss(use_iou=False) and the GIoU box term: eager, with graph_hot_path=True, and one evaluation step).  They run
in a process of their own for the reasons tests/bipartite_graph_worker.py gives.  Every check asserts here; one JSON line with the figures
is printed at the end.  Usage: python tests/tal_graph_worker.py"""
import copy
import functools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tal_cases as tc                                                                                         # noqa: E402
from bipartite_graph_worker import MB2                                                                         # noqa: E402
from single_shot_detection_amd import _lib, synthetic as syn                                                   # noqa: E402
from single_shot_detection_amd.detection import sampler                                                        # noqa: E402
from single_shot_detection_amd.detection.box_coder import BoxCoder                                             # noqa: E402
from single_shot_detection_amd.detection.losses.multibox_loss import MultiboxLoss                              # noqa: E402
from single_shot_detection_amd.detection.target_assigner import PackedGroundTruth, TaskAlignedAssigner         # noqa: E402

LOSS = {'classification_loss': {'name': 'QualityFocalLoss', 'use_iou': False}, 'localization_loss': {'name': 'GeneralizedIoULoss'},
        'classification_weight': 1.0, 'localization_weight': 1.0}


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tensors(gt_list):
    return [torch.from_numpy(g) for g in gt_list]


def tal_in_a_captured_graph():
    """encode_ground_truth inside torch.cuda.graph on a PackedGroundTruth of fixed capacity and static prediction buffers: two replays on
    two batches (boxes AND predictions change in between) equal the eager results, whose decisions are the restatement's."""
    gt_a, anchors_np, s_a, l_a, kw, fig_a = tc.generated('mb2_g32')
    gt_b, _, s_b, l_b, kw_b, fig_b = tc.generated('mb2_one_empty')
    assert kw == kw_b and s_a.shape == s_b.shape
    anchors = torch.from_numpy(anchors_np).cuda()
    coder = BoxCoder(tc.XY_SCALE, tc.WH_SCALE)
    ta = TaskAlignedAssigner(**kw)
    batches = [(gt, torch.from_numpy(s).cuda(), torch.from_numpy(l).cuda()) for gt, s, l in ((gt_a, s_a, l_a), (gt_b, s_b, l_b))]
    eager = [ta.encode_ground_truth(tensors(gt), anchors, (s, l), coder, return_box_idx=True) for gt, s, l in batches]
    packed = PackedGroundTruth.from_list(tensors(gt_a), anchors.device, capacity=3 * 32 + 5)
    scores, locs = batches[0][1].clone(), batches[0][2].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ta.encode_ground_truth(packed, anchors, (scores, locs), coder, return_box_idx=True)      # warm-up: the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        t, idx = ta.encode_ground_truth(packed, anchors, (scores, locs), coder, return_box_idx=True)
    for (gt, s, l), (ref_t, ref_idx), fig in zip(batches, eager, (fig_a, fig_b)):
        packed.update_(tensors(gt))
        scores.copy_(s)
        locs.copy_(l)
        t.fill_(7.0)
        idx.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx, ref_idx) and np.array_equal(bits(t), bits(ref_t))
        assert np.array_equal(idx.cpu().numpy(), fig['idx64'])


def detection_init_with_the_task_aligned_assigner(graph_hot_path, phase='train'):
    """The intended configuration through detection.init (ssd_mb2_voc, batch 2), which hands the assigner the step's own prediction and the
    box coder: one step.  The restatement, evaluated on the prediction the step returns, must keep its margins; the step's loss is then
    the existing loss path's (MultiboxLoss on the same prediction) on the restatement's target."""
    from single_shot_detection_amd.detection import init as det_init
    torch.manual_seed(9)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, copy.deepcopy(MB2), {'xy_scale': tc.XY_SCALE, 'wh_scale': tc.WH_SCALE},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SIGMOID'},
        copy.deepcopy(LOSS), {'name': 'valid_sampler'}, {'name': 'TaskAlignedAssigner', 'topk': 13}, graph_hot_path=graph_hot_path)
    # A fresh detector's heads (std 0.01) predict nearly the same for every anchor, and equal predictions tie systematically between the
    # anchors of neighbouring cells: no decision would have a margin.  Heads of std 0.03 spread the logits and locs like a trained model's.
    with torch.no_grad():
        for head in wrapper.model.predictor.heads:
            for conv in (head['score'], head['loc']):
                conv.weight.normal_(0.0, 0.03)
    imgs = torch.from_numpy(np.random.default_rng(31).standard_normal((2, 3, 300, 300), dtype=np.float32))
    gt_np = syn.make_ground_truth(2, 300, 21, seed=1)
    anchors_np = np.load(tc.GOLDEN + '/ssd_mb2_voc.npz')['anchors']

    seen = []
    encode = TaskAlignedAssigner.encode_ground_truth

    def recording(self, ground_truth, anchors, prediction, box_coder, **kwargs):
        out = encode(self, ground_truth, anchors, prediction, box_coder, **kwargs)
        # (a copy: none while a segment is captured -- its target lives in the graph's pool)
        seen.append((None if torch.cuda.is_current_stream_capturing() else out.clone(), box_coder))
        return out
    TaskAlignedAssigner.encode_ground_truth = recording
    try:
        if phase == 'train':
            wrapper.model.train()
            loss, (scores, locs), _ = step_fn(0, 'train', (imgs, tensors(gt_np)), init_state())
        else:
            # The evaluation step (phase 'eval': eager encode, loss, postprocess) under no_grad, the norms still on batch statistics: with
            # the running statistics of a model that never trained (mean 0, variance 1) the predictions nearly tie between cells (a rank gap
            # of 5e-8 was measured; why exactly was not looked into): no decision would have a margin.
            wrapper.model.train()
            with torch.no_grad():
                s0, l0, _ = wrapper.model(imgs.to(dev))       # (the evaluation step returns detections, not the raw prediction)
                loss, detections, _ = step_fn(0, 'eval', (imgs, tensors(gt_np)), init_state())
            scores, locs = s0, l0
            assert detections is not None
    finally:
        TaskAlignedAssigner.encode_ground_truth = encode
    assert torch.isfinite(loss).all()
    assert bool(step_fn.hot_segments) == graph_hot_path
    assert seen and all(isinstance(bc, BoxCoder) and bc.xy_scale == tc.XY_SCALE for _, bc in seen)
    B, A = 2, len(anchors_np)
    s_np, l_np = scores.detach().cpu().numpy().reshape(B, A, -1), locs.detach().cpu().numpy().reshape(B, A, 4)
    assert s_np.shape[2] == 21
    fig = tc.margins(gt_np, anchors_np, s_np, l_np, topk=13)
    print('margins', phase, 'graphed' if graph_hot_path else 'eager', {k: float(f'{v:.3g}') for k, v in fig.items() if np.isscalar(v)},
          'positives', int((fig['idx64'] >= 0).sum()), flush=True)
    tc.assert_margins(fig)
    assert (fig['idx64'] >= 0).any()
    target = torch.from_numpy(tc.target_np(fig['idx64'], fig['col64'], gt_np).astype(np.float32)).to(dev)
    if not graph_hot_path and phase == 'train':      # (a captured segment's target lives in the graph's pool and is recycled by the backward pass)
        got = seen[-1][0]
        assert np.array_equal(bits(got[..., :5]), bits(target[..., :5]))
        assert float((got[..., 5] - target[..., 5]).abs().max()) <= 4.0 * fig['col5_dev']
    criterion = MultiboxLoss(sampler=functools.partial(sampler.valid_sampler), box_coder=BoxCoder(tc.XY_SCALE, tc.WH_SCALE), **copy.deepcopy(LOSS))
    with torch.no_grad():
        ref = float(criterion((scores.detach(), locs.detach()), torch.from_numpy(anchors_np).to(dev), target.clone())[0])
    assert abs(loss.item() - ref) <= 1e-4 + 1e-5 * abs(ref), (loss.item(), ref)
    if phase == 'train':
        loss.backward()
        assert all(p.grad is None or torch.isfinite(p.grad).all() for p in wrapper.model.parameters())
    return float(loss.detach()), ref


def main():
    res = {}
    tal_in_a_captured_graph()
    res['captured_graph'] = 'two replays equal the eager results'
    res['eager_loss'], res['eager_ref_loss'] = detection_init_with_the_task_aligned_assigner(False)
    res['graphed_loss'], res['graphed_ref_loss'] = detection_init_with_the_task_aligned_assigner(True)
    res['eval_loss'], res['eval_ref_loss'] = detection_init_with_the_task_aligned_assigner(False, phase='eval')
    torch.cuda.synchronize()
    res['timeouts'] = _lib.streamk_timeouts()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
