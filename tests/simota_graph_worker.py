"""Child process of tests/test_simota_gpu.py: the checks of SimOtaAssigner that capture HIP graphs or build a whole detector
(encode_ground_truth inside torch.cuda.graph; detection.init with target_assigner = {'name': 'SimOtaAssigner'}, valid_sampler,
QualityFocalLoss and IoULoss: eager and with graph_hot_path=True).  They run in a fresh process of their own for the reasons
tests/bipartite_graph_worker.py gives.  Every check asserts here; one JSON line with the figures is printed at the end.
Usage: python tests/simota_graph_worker.py"""
import copy
import functools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simota_cases as sc                                                                                      # noqa: E402
from bipartite_graph_worker import MB2                                                                         # noqa: E402
from single_shot_detection_amd import _lib, synthetic as syn                                                   # noqa: E402
from single_shot_detection_amd.detection import sampler                                                        # noqa: E402
from single_shot_detection_amd.detection.box_coder import BoxCoder                                             # noqa: E402
from single_shot_detection_amd.detection.losses.multibox_loss import MultiboxLoss                              # noqa: E402
from single_shot_detection_amd.detection.target_assigner import PackedGroundTruth, SimOtaAssigner              # noqa: E402

LOSS = {'classification_loss': {'name': 'QualityFocalLoss'}, 'localization_loss': {'name': 'IoULoss'},
        'classification_weight': 1.0, 'localization_weight': 1.0}


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tensors(gt_list):
    return [torch.from_numpy(g) for g in gt_list]


def simota_in_a_captured_graph():
    """encode_ground_truth inside torch.cuda.graph on a PackedGroundTruth of fixed capacity and static prediction buffers: two replays on
    two batches (boxes AND predictions change in between) equal the eager results, whose decisions are the restatement's."""
    gt_a, anchors_np, s_a, l_a, sizes, strides, kw, fig_a = sc.generated('mb2_g32')
    gt_b, _, s_b, l_b, _, _, kw_b, fig_b = sc.generated('mb2_one_empty')
    assert kw == kw_b and s_a.shape == s_b.shape
    anchors = torch.from_numpy(anchors_np).cuda()
    coder = BoxCoder(sc.XY_SCALE, sc.WH_SCALE)
    sa = SimOtaAssigner(**kw)
    lv = dict(level_sizes=sizes, level_strides=strides, return_box_idx=True, return_dynamic_k=True)
    batches = [(gt, torch.from_numpy(s).cuda(), torch.from_numpy(l).cuda()) for gt, s, l in ((gt_a, s_a, l_a), (gt_b, s_b, l_b))]
    eager = [sa.encode_ground_truth(tensors(gt), anchors, (s, l), coder, **lv) for gt, s, l in batches]
    packed = PackedGroundTruth.from_list(tensors(gt_a), anchors.device, capacity=3 * 32 + 5)
    scores, locs = batches[0][1].clone(), batches[0][2].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sa.encode_ground_truth(packed, anchors, (scores, locs), coder, **lv)      # warm-up: the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        t, idx, k = sa.encode_ground_truth(packed, anchors, (scores, locs), coder, **lv)
    for (gt, s, l), (ref_t, ref_idx, ref_k), fig in zip(batches, eager, (fig_a, fig_b)):
        packed.update_(tensors(gt))
        scores.copy_(s)
        locs.copy_(l)
        t.fill_(7.0)
        idx.fill_(7)
        k.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        n = ref_k.numel()
        assert torch.equal(idx, ref_idx) and np.array_equal(bits(t), bits(ref_t)) and torch.equal(k[:n], ref_k) and (k[n:] == 0).all()
        assert np.array_equal(idx.cpu().numpy(), fig['idx64']) and np.array_equal(ref_k.cpu().numpy(), np.concatenate(fig['k64']))


def detection_init_with_the_simota_assigner(graph_hot_path):
    """The intended configuration through detection.init (ssd_mb2_voc, batch 2), which hands the assigner the step's own prediction, the
    box coder and the detector's level sizes and strides: one training step.  The restatement, evaluated on the prediction the step
    returns, must keep its margins; the step's loss is then the existing loss path's (MultiboxLoss on the same prediction) on the
    restatement's target."""
    from single_shot_detection_amd.detection import init as det_init
    torch.manual_seed(9)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, copy.deepcopy(MB2), {'xy_scale': sc.XY_SCALE, 'wh_scale': sc.WH_SCALE},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SIGMOID'},
        copy.deepcopy(LOSS), {'name': 'valid_sampler'}, {'name': 'SimOtaAssigner'}, graph_hot_path=graph_hot_path)
    # A fresh detector's heads (std 0.01) predict nearly the same for every anchor, and equal predictions tie systematically between the
    # anchors of neighbouring cells: no decision would have a margin.  Heads of std 0.03 spread the logits and locs like a trained model's.
    with torch.no_grad():
        for head in wrapper.model.predictor.heads:
            for conv in (head['score'], head['loc']):
                conv.weight.normal_(0.0, 0.03)
    imgs = torch.from_numpy(np.random.default_rng(31).standard_normal((2, 3, 300, 300), dtype=np.float32))
    gt_np = syn.make_ground_truth(2, 300, 21, seed=1)
    anchors_np = np.load(sc.GOLDEN + '/ssd_mb2_voc.npz')['anchors']
    sizes, strides = sc.config_levels('ssd_mb2_voc')

    seen = []
    encode = SimOtaAssigner.encode_ground_truth

    def recording(self, ground_truth, anchors, prediction, box_coder, **kwargs):
        out = encode(self, ground_truth, anchors, prediction, box_coder, **kwargs)
        # (a copy: none while a segment is captured -- its target lives in the graph's pool)
        seen.append((None if torch.cuda.is_current_stream_capturing() else out.clone(), box_coder, kwargs))
        return out
    SimOtaAssigner.encode_ground_truth = recording
    try:
        wrapper.model.train()
        loss, (scores, locs), _ = step_fn(0, 'train', (imgs, tensors(gt_np)), init_state())
    finally:
        SimOtaAssigner.encode_ground_truth = encode
    assert torch.isfinite(loss).all()
    assert bool(step_fn.hot_segments) == graph_hot_path
    assert seen and all(isinstance(bc, BoxCoder) and bc.xy_scale == sc.XY_SCALE for _, bc, _ in seen)
    # the detector's own level table is the config's: sizes exactly, strides image size / map size
    assert all(tuple(kw['level_sizes']) == tuple(sizes) for _, _, kw in seen)
    assert all(np.allclose(np.asarray(kw['level_strides']), np.asarray(strides)[:, None].repeat(2, 1), rtol=0, atol=0) for _, _, kw in seen)
    B, A = 2, len(anchors_np)
    s_np, l_np = scores.detach().cpu().numpy().reshape(B, A, -1), locs.detach().cpu().numpy().reshape(B, A, 4)
    assert s_np.shape[2] == 21
    fig = sc.margins(gt_np, anchors_np, s_np, l_np, sizes, strides)
    print('margins', 'graphed' if graph_hot_path else 'eager', {k: float(f'{v:.3g}') for k, v in fig.items() if np.isscalar(v)},
          'positives', int((fig['idx64'] >= 0).sum()), flush=True)
    sc.assert_margins(fig)
    assert (fig['idx64'] >= 0).any()
    target = torch.from_numpy(sc.target_np(fig['idx64'], gt_np)).to(dev)
    if not graph_hot_path:      # (a captured segment's target lives in the graph's pool and is recycled by the backward pass)
        assert np.array_equal(bits(seen[-1][0]), bits(target))
    criterion = MultiboxLoss(sampler=functools.partial(sampler.valid_sampler), box_coder=BoxCoder(sc.XY_SCALE, sc.WH_SCALE), **copy.deepcopy(LOSS))
    with torch.no_grad():
        ref = float(criterion((scores.detach(), locs.detach()), torch.from_numpy(anchors_np).to(dev), target.clone())[0])
    assert abs(loss.item() - ref) <= 1e-4 + 1e-5 * abs(ref), (loss.item(), ref)
    loss.backward()
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in wrapper.model.parameters())
    return float(loss.detach()), ref


def main():
    res = {}
    simota_in_a_captured_graph()
    res['captured_graph'] = 'two replays equal the eager results'
    res['eager_loss'], res['eager_ref_loss'] = detection_init_with_the_simota_assigner(False)
    res['graphed_loss'], res['graphed_ref_loss'] = detection_init_with_the_simota_assigner(True)
    torch.cuda.synchronize()
    res['timeouts'] = _lib.streamk_timeouts()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
