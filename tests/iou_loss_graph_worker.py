"""Child process of tests/test_iou_loss_gpu.py: the checks of the IoU-based box terms that capture HIP graphs or build a whole detector
(ssdk_multibox_loss_fwd / _bwd_ex with a new box kind inside torch.cuda.graph; detection.init on ssd_mb2_voc, batch 2, with
TaskAlignedAssigner, valid_sampler, QualityFocalLoss(use_iou=False) and CompleteIoULoss: eager and with graph_hot_path=True).  They run in a
process of their own for the reasons tests/bipartite_graph_worker.py gives.  Every check asserts here; one JSON line with the figures is
printed at the end.  Usage: python tests/iou_loss_graph_worker.py"""
import copy
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iou_loss_cases as ic                                                                                    # noqa: E402
import quality_loss_cases as qc                                                                                # noqa: E402
from bipartite_graph_worker import MB2                                                                         # noqa: E402
from single_shot_detection_amd import _lib, ops, synthetic as syn                                              # noqa: E402
from single_shot_detection_amd.detection import sampler                                                        # noqa: E402
from single_shot_detection_amd.detection.target_assigner import TaskAlignedAssigner                            # noqa: E402

LOSS = {'classification_loss': {'name': 'QualityFocalLoss', 'use_iou': False}, 'localization_loss': {'name': 'CompleteIoULoss'},
        'classification_weight': 1.0, 'localization_weight': 1.0}


def loss_calls_in_a_captured_graph(cls_kind, box):
    """Forward and backward through the C ABI with sampled = NULL, captured once and replayed on two batches: out3, dscores, dlocs, the
    row mask (and the target, which these kinds leave alone) equal the eager calls bit for bit."""
    lib = _lib.lib()
    case = qc.case('b3_c20')
    B, A, C = case['B'], case['A'], case['C']
    batches = [(case['scores'], case['locs'], case['target']),
               (case['scores'].roll(1, 0).flip(1).contiguous(), case['locs'].roll(1, 0).contiguous(), case['target'].roll(1, 0).contiguous())]
    dev = torch.device('cuda:0')
    anchors = case['anchors'].cuda()
    params = _lib.LossParams(cls_kind, ic.LOC_KIND[box], 2.0, 0.75, 0, 0.0, 1.0, 1.0, qc.XY_SCALE, qc.WH_SCALE, qc.EPS, 1.0, 0.0, None, 0)
    ws = sampler.loss_workspace(B, A, C, dev)
    scores, locs = torch.empty((B, A * C), device=dev), torch.empty((B, A * 4), device=dev)
    target = torch.empty((B, A, 6), device=dev)
    out3, grad = torch.empty((3,), device=dev), torch.tensor([1.5], device=dev)
    dscores, dlocs = torch.empty_like(scores), torch.empty_like(locs)
    row_mask = torch.empty((B, A), dtype=torch.uint8, device=dev)

    def calls():
        _lib.check(lib.ssdk_multibox_loss_fwd(ctypes.byref(params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target), None,
                                              B, A, C, 0, _lib.ptr(out3), _lib.ptr(ws), ws.numel(), _lib.current_stream()), 'fwd')
        _lib.check(lib.ssdk_multibox_loss_bwd_ex(ctypes.byref(params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target), None,
                                                 _lib.ptr(grad), 1, B, A, C, _lib.ptr(dscores), _lib.ptr(dlocs), _lib.ptr(row_mask), _lib.ptr(ws),
                                                 ws.numel(), _lib.current_stream()), 'bwd')

    def load(batch):
        for dst, src in zip((scores, locs, target), batch):
            dst.copy_(src.view(dst.shape))
        for t in (out3, dscores, dlocs):
            t.fill_(7.0)
        row_mask.fill_(7)

    eager = []
    for batch in batches:
        load(batch)
        calls()
        torch.cuda.synchronize()
        eager.append([t.clone() for t in (out3, dscores, dlocs, target, row_mask)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls()
    for batch, ref in zip(batches, eager):
        load(batch)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((out3, dscores, dlocs, target, row_mask), ref):
            assert torch.equal(got, want)
        assert torch.isfinite(out3).all() and out3[2] > 0 and torch.equal(target.cpu(), batch[2])
        assert torch.equal(row_mask.cpu().bool(), batch[2][..., 4] != -1)


def detection_init_with_tal_and_ciou(graph_hot_path, state_dict=None):
    """TaskAlignedAssigner + valid_sampler + QualityFocalLoss(use_iou=False) + CompleteIoULoss through detection.init (ssd_mb2_voc, batch 2):
    one training step; the loss is the restatement's on the target the assigner produced (eager line)."""
    from single_shot_detection_amd.detection import init as det_init
    torch.manual_seed(9)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, copy.deepcopy(MB2), {'xy_scale': qc.XY_SCALE, 'wh_scale': qc.WH_SCALE},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SIGMOID'},
        copy.deepcopy(LOSS), {'name': 'valid_sampler'}, {'name': 'TaskAlignedAssigner', 'topk': 13}, graph_hot_path=graph_hot_path)
    if state_dict is None:
        with torch.no_grad():   # (as tests/tal_graph_worker.py: heads of std 0.03 spread the predictions like a trained model's)
            for head in wrapper.model.predictor.heads:
                for conv in (head['score'], head['loc']):
                    conv.weight.normal_(0.0, 0.03)
    else:
        wrapper.model.load_state_dict(state_dict)
    state_dict = copy.deepcopy(wrapper.model.state_dict())
    imgs = torch.from_numpy(np.random.default_rng(31).standard_normal((2, 3, 300, 300), dtype=np.float32))
    gt_np = syn.make_ground_truth(2, 300, 21, seed=1)
    anchors = torch.from_numpy(np.load(qc.GOLDEN + '/ssd_mb2_voc.npz')['anchors'])

    seen = []
    encode = TaskAlignedAssigner.encode_ground_truth

    def recording(self, *args, **kwargs):
        out = encode(self, *args, **kwargs)
        # (a copy: none while a segment is captured -- its target lives in the graph's pool)
        seen.append(None if torch.cuda.is_current_stream_capturing() else out.clone())
        return out
    TaskAlignedAssigner.encode_ground_truth = recording
    try:
        wrapper.model.train()
        loss, (scores, locs), _ = step_fn(0, 'train', (imgs, [torch.from_numpy(g) for g in gt_np]), init_state())
    finally:
        TaskAlignedAssigner.encode_ground_truth = encode
    assert torch.isfinite(loss).all()
    assert bool(step_fn.hot_segments) == graph_hot_path
    ref = None
    if not graph_hot_path:
        target = seen[-1].cpu()
        assert (target[..., 4] > 0).any()
        out = ic.dense_restatement(scores.detach().cpu().double(), locs.detach().cpu().double(), anchors, target, None, 'qfl', 'ciou', use_iou=False)
        ref = float(out[0])
        assert abs(loss.item() - ref) <= 1e-4 + 1e-5 * abs(ref), (loss.item(), ref)
        assert float(out[2]) > 0
    loss.backward()
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in wrapper.model.parameters())
    return float(loss.detach()), ref, state_dict


def main():
    res = {}
    loss_calls_in_a_captured_graph(5, 'ciou')    # Quality Focal + CIoU
    loss_calls_in_a_captured_graph(6, 'eiou')    # Varifocal + EIoU
    loss_calls_in_a_captured_graph(1, 'diou')    # SigmoidFocalLoss on the dense path + DIoU
    loss_calls_in_a_captured_graph(5, 'iou')
    res['captured_graph'] = 'two replays equal the eager results'
    flags = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        with ops.deterministic():
            res['eager_loss'], res['restatement_loss'], state = detection_init_with_tal_and_ciou(False)
            res['graphed_loss'], _, _ = detection_init_with_tal_and_ciou(True, state)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = flags
    assert res['eager_loss'] == res['graphed_loss'], res
    torch.cuda.synchronize()
    res['timeouts'] = _lib.streamk_timeouts()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
