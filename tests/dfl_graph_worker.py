"""Child process of tests/test_dfl_gpu.py: the checks of the integral box head that capture HIP graphs or build a whole detector
(ssdk_integral_fwd / _bwd inside torch.cuda.graph; detection.init with the full Generalized Focal Loss configuration -- ATSS, valid_sampler,
QualityFocalLoss, GeneralizedIoULoss, IntegralBoxCoder + DistributionFocalLoss, heads built with reg_max -- eager and with
graph_hot_path=True).  They run in a process of their own for the reasons tests/bipartite_graph_worker.py gives.  Every check asserts here;
one JSON line with the figures is printed at the end.
Usage: python tests/dfl_graph_worker.py"""
import copy
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_cases as dc                                                                                         # noqa: E402
import quality_loss_cases as qc                                                                                # noqa: E402
from bipartite_graph_worker import MB2                                                                         # noqa: E402
from single_shot_detection_amd import _lib, ops, synthetic as syn                                              # noqa: E402
from single_shot_detection_amd.detection.target_assigner import AtssTargetAssigner                             # noqa: E402

REG_MAX = 16


def integral_calls_in_a_captured_graph(bins):
    """Forward and backward through the C ABI, captured once and replayed on two batches: locs, out, dlogits equal the eager calls bit for
    bit."""
    lib = _lib.lib()
    case = qc.case('b3_c20')
    B, A = case['B'], case['A']
    z0 = dc.logits_for('b3_c20', bins).view(B, A, 4, bins)
    rng = np.random.default_rng(4)
    dl0 = torch.from_numpy(rng.standard_normal((B, A, 4)).astype(np.float32))
    batches = [(z0, case['target'], dl0), (z0.roll(1, 0).flip(1).contiguous(), case['target'].roll(1, 0).contiguous(), dl0.flip(0).contiguous())]
    dev = torch.device('cuda:0')
    anchors = case['anchors'].cuda()
    params = _lib.IntegralParams(bins, dc.XY_LIMIT, dc.WH_LIMIT, qc.XY_SCALE, qc.WH_SCALE, qc.EPS, 0.25)
    ws = torch.empty((lib.ssdk_integral_workspace_bytes(B, A),), dtype=torch.uint8, device=dev)
    z, target, dlocs = torch.empty((B, A, 4, bins), device=dev), torch.empty((B, A, 6), device=dev), torch.empty((B, A, 4), device=dev)
    locs, out2, dz = torch.empty((B, A, 4), device=dev), torch.empty((2,), device=dev), torch.empty_like(z)
    grad = torch.tensor([1.5], device=dev)

    def calls():
        _lib.check(lib.ssdk_integral_fwd(ctypes.byref(params), _lib.ptr(z), _lib.ptr(anchors), _lib.ptr(target), B, A, _lib.ptr(locs), _lib.ptr(out2),
                                         _lib.ptr(ws), ws.numel(), _lib.current_stream()), 'fwd')
        _lib.check(lib.ssdk_integral_bwd(ctypes.byref(params), _lib.ptr(z), _lib.ptr(dlocs), target[..., 4].data_ptr(), 6, _lib.ptr(grad), B, A,
                                         _lib.ptr(dz), _lib.ptr(ws), ws.numel(), _lib.current_stream()), 'bwd')

    def load(batch):
        for dst, src in zip((z, target, dlocs), batch):
            dst.copy_(src)
        for t in (locs, out2, dz):
            t.fill_(7.0)

    eager = []
    for batch in batches:
        load(batch)
        calls()
        torch.cuda.synchronize()
        eager.append([t.clone() for t in (locs, out2, dz)])
    assert not torch.equal(eager[0][2], eager[1][2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls()
    for batch, ref in zip(batches, eager):
        load(batch)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((locs, out2, dz), ref):
            assert torch.equal(got, want)
        assert torch.isfinite(out2).all() and out2[1] > 0


def detection_init_with_the_gfl_config(graph_hot_path, state_dict=None):
    """ATSS + valid_sampler + QualityFocalLoss + GeneralizedIoULoss + IntegralBoxCoder / DistributionFocalLoss through detection.init
    (ssd_mb2_voc, batch 2, heads built with reg_max): one training step; the loss is the restatement's on the target the assigner produced
    (eager line)."""
    from single_shot_detection_amd.detection import init as det_init
    torch.manual_seed(9)
    dev = torch.device('cuda:0')
    model = copy.deepcopy(MB2)
    model['detector']['heads'] = {'reg_max': REG_MAX}
    wrapper, init_state, step_fn = det_init.init(
        dev, model, {'name': 'IntegralBoxCoder', 'xy_scale': 10.0, 'wh_scale': 5.0, 'reg_max': REG_MAX},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SIGMOID'},
        {'classification_loss': {'name': 'QualityFocalLoss'}, 'localization_loss': {'name': 'GeneralizedIoULoss'},
         'distribution_loss': {'name': 'DistributionFocalLoss'}, 'distribution_weight': 0.25,
         'classification_weight': 1.0, 'localization_weight': 1.0},
        {'name': 'valid_sampler'}, {'name': 'AtssTargetAssigner', 'topk': 9}, graph_hot_path=graph_hot_path)
    if state_dict is not None:
        wrapper.model.load_state_dict(state_dict)
    state_dict = copy.deepcopy(wrapper.model.state_dict())
    assert state_dict['predictor.heads.0.loc.weight'].shape[0] % (4 * (REG_MAX + 1)) == 0
    imgs = torch.from_numpy(np.random.default_rng(31).standard_normal((2, 3, 300, 300), dtype=np.float32))
    gt_np = syn.make_ground_truth(2, 300, 21, seed=1, fixed_g=32)
    anchors = torch.from_numpy(np.load(qc.GOLDEN + '/ssd_mb2_voc.npz')['anchors'])

    seen = []
    encode = AtssTargetAssigner.encode_ground_truth

    def recording(self, *args, **kwargs):
        out = encode(self, *args, **kwargs)
        # (a copy: none while a segment is captured -- its target lives in the graph's pool)
        seen.append(None if torch.cuda.is_current_stream_capturing() else out.clone())
        return out
    AtssTargetAssigner.encode_ground_truth = recording
    try:
        wrapper.model.train()
        loss, (scores, logits), _ = step_fn(0, 'train', (imgs, [torch.from_numpy(g) for g in gt_np]), init_state())
    finally:
        AtssTargetAssigner.encode_ground_truth = encode
    assert torch.isfinite(loss).all()
    assert bool(step_fn.hot_segments) == graph_hot_path
    A = anchors.shape[0]
    assert tuple(logits.shape) == (2, A * 4 * (REG_MAX + 1))
    ref = dfl = None
    if not graph_hot_path:
        target = seen[-1].cpu()
        assert (target[..., 4] > 0).any()
        out = dc.restatement(scores.detach().cpu().double(), logits.detach().cpu().double(), anchors, target, None, 'qfl', REG_MAX + 1, loc='giou')
        ref, dfl = float(out[0]), float(out[3])
        assert abs(loss.item() - ref) <= 1e-4 + 1e-5 * abs(ref), (loss.item(), ref)
    loss.backward()
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in wrapper.model.parameters())
    if not graph_hot_path:   # both head families received a gradient (a level without a positive has an all-zero loc gradient: summed over levels)
        for kind in ('score', 'loc'):
            grads = [p.grad for n, p in wrapper.model.named_parameters() if f'.{kind}.weight' in n and '.heads.' in n]
            assert len(grads) == 6 and all(g is not None for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0, kind
    if not graph_hot_path:   # evaluation through the same wrapper: the postprocessor integrates the logits first
        wrapper.model.eval()
        with torch.no_grad():
            _, pred, _ = step_fn(1, 'eval', (imgs, [torch.from_numpy(g) for g in gt_np]), init_state())
        assert len(pred) == 2 and all(p.shape[1] == 6 and torch.isfinite(p).all() for p in pred)
    return float(loss.detach()), ref, dfl, state_dict


def main():
    res = {}
    integral_calls_in_a_captured_graph(17)
    integral_calls_in_a_captured_graph(8)
    res['captured_graph'] = 'two replays equal the eager results'
    flags = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        with ops.deterministic():
            res['eager_loss'], res['restatement_loss'], res['dfl'], state = detection_init_with_the_gfl_config(False)
            res['graphed_loss'], _, _, _ = detection_init_with_the_gfl_config(True, state)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = flags
    assert res['eager_loss'] == res['graphed_loss'], res
    torch.cuda.synchronize()
    res['timeouts'] = _lib.streamk_timeouts()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
