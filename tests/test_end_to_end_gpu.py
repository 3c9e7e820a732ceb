"""GPU: the mirrored API driven end to end through ``detection.init`` (the seam of detection/init.py:19-137):
build -> step_fn('train') -> backward -> step_fn('eval'), SSD-300 VGG16 configuration with a random-init backbone.
The backbone is out of scope (stock PyTorch-ROCm); everything behind its taps is checked against torch fp32 CPU
modules with the same weights plus the oracle."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle
from single_shot_detection_amd import synthetic as syn
from single_shot_detection_amd.detection import init as det_init

pytestmark = pytest.mark.gpu

MODEL = {
    'base': {'name': 'torchvision_vgg16_bn', 'pretrained': False},
    'detector': {'num_classes': 21, 'use_depthwise': False,
                 'features': {'name': 'Features', 'out_layers': (32, 42), 'last_feature_layer': 42},
                 'extras': {'layers': (('s', 512), ('s', 256), ('s', 256), ('s', 256))}},
    'anchor_generator': {'type': 'ssd', 'num_scales': 6, 'min_scale': 0.15, 'max_scale': 1.05,
                         'aspect_ratios': [[1.0, 2.0]] + [[1.0, 2.0, 3.0]] * 3 + [[1.0, 2.0]] * 2},
}


def _ref_block(blk, x):
    x = F.conv2d(x, blk.conv.weight.detach().cpu().contiguous(), None, stride=blk.conv.stride, padding=blk.conv.padding)
    bn = blk.bn
    x = F.batch_norm(x, None, None, bn.weight.detach().cpu(), bn.bias.detach().cpu(), training=True, eps=bn.eps)
    return torch.relu(x)


def test_ssd300_step_fn_train_and_eval():
    torch.manual_seed(3)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, MODEL, {'xy_scale': 10.0, 'wh_scale': 5.0},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SOFTMAX'},
        {'classification_loss': {'name': 'CrossEntropyLoss'}, 'localization_loss': {'name': 'SmoothL1Loss'},
         'classification_weight': 1.0, 'localization_weight': 1.0},
        {'name': 'hard_negative_mining', 'negative_per_positive_ratio': 3, 'min_negative_per_image': 5},
        {'matched_threshold': 0.5, 'unmatched_threshold': 0.5})
    detector = wrapper.model
    detector.train()
    B = 2
    imgs = torch.from_numpy(np.random.default_rng(23).standard_normal((B, 3, 300, 300), dtype=np.float32))
    gt_np = syn.make_ground_truth(B, 300, 21, seed=1)
    gt = [torch.from_numpy(g) for g in gt_np]

    # capture the backbone taps of THIS forward (train-mode BN): the reference below starts from them
    taps = {}
    hooks = [detector.predictor.features.base[i].register_forward_hook(lambda m, a, o, i=i: taps.__setitem__(i, o.detach())) for i in (32, 42)]
    state = init_state()
    loss, prediction, state = step_fn(0, 'train', (imgs, gt), state)
    for h in hooks:
        h.remove()
    scores, locs = prediction
    assert scores.shape == (B, 8108 * 21) and locs.shape == (B, 8108 * 4)      # A = 8108
    assert np.isfinite(loss.item()) and abs(state['loss'] - loss.item()) < 1e-4

    # ---- reference from the taps: extras + heads with torch fp32 CPU ops, then the oracle -------------------------
    x = taps[42].float().cpu().contiguous()
    sources = [taps[32].float().cpu().contiguous(), x]
    for layer in detector.predictor.extras:
        for blk in layer:
            x = _ref_block(blk, x)
        sources.append(x)
    ref_s, ref_l = [], []
    for src, head in zip(sources, detector.predictor.heads):
        ref_s.append(F.conv2d(src, head['score'].weight.detach().cpu().contiguous(), head['score'].bias.detach().cpu(), padding=1).permute(0, 2, 3, 1).reshape(B, -1))
        ref_l.append(F.conv2d(src, head['loc'].weight.detach().cpu().contiguous(), head['loc'].bias.detach().cpu(), padding=1).permute(0, 2, 3, 1).reshape(B, -1))
    # The two levels fed by the backbone taps are ONE convolution away from the reference's inputs: held to the fp32 bound of a K = 9 * 512
    # sum (2e-6 * sqrt(K), as tests/test_heads_gpu.py).  The four tail levels sit behind up to eight train-mode BatchNorms whose
    # statistics are taken over B * H * W = 2 * (9^2 .. 1^2) rows: a last-bit difference in a convolution sum is divided by sqrt(var + eps)
    # of as few as two values per channel (the 1 x 1 level), layer after layer -- rtol 1e-3 / atol 2e-3 is what that chain is held to here;
    # block by block the same arithmetic is pinned to 2e-5 by tests/test_blocks_golden_gpu.py (reference-generated goldens).
    n0 = [h * h * 4 * 21 for h in (37,)][0] + 18 * 18 * 6 * 21
    l0 = 37 * 37 * 4 * 4 + 18 * 18 * 6 * 4
    got_s, got_l = scores.cpu().numpy(), locs.cpu().numpy()
    tight = 2e-6 * np.sqrt(9 * 512)
    np.testing.assert_allclose(got_s[:, :n0], torch.cat(ref_s, 1).numpy()[:, :n0], rtol=1e-5, atol=tight * float(np.abs(torch.cat(ref_s, 1).numpy()[:, :n0]).max() + 1))
    np.testing.assert_allclose(got_l[:, :l0], torch.cat(ref_l, 1).numpy()[:, :l0], rtol=1e-5, atol=tight * float(np.abs(torch.cat(ref_l, 1).numpy()[:, :l0]).max() + 1))
    ref_s, ref_l = torch.cat(ref_s, 1).numpy(), torch.cat(ref_l, 1).numpy()
    np.testing.assert_allclose(got_s, ref_s, rtol=1e-3, atol=2e-3)
    np.testing.assert_allclose(got_l, ref_l, rtol=1e-3, atol=2e-3)

    cfg = syn.CONFIGS['ssd_300_vgg16_voc']
    anchors = oracle.anchors(cfg['anchor'], 300, cfg['levels'])
    target = oracle.encode_ground_truth(gt_np, anchors, 0.5, 0.5)
    s_np, l_np = scores.cpu().numpy(), locs.cpu().numpy()
    mask = oracle.hard_negative_mining(s_np, target, 3, 5)
    vals, _, _ = oracle.multibox_loss(s_np, l_np, anchors, target, mask, kind='ce', grads=False)
    assert abs(loss.item() - vals[0]) <= 1e-4 + 1e-5 * abs(vals[0]), (loss.item(), vals)

    loss.backward()
    grads = [p.grad for p in detector.parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)

    # ---- eval phase: list of [K,6] detections, checked against the oracle on the same logits ---------------------
    detector.eval()
    with torch.no_grad():
        # (freshly initialised score heads give 21 near-equal probabilities per anchor: thousands of candidates whose ORDER is decided by
        # the last ulp of an exp(), and greedy NMS follows the order -- no checker can pin that.  Spread the logits like a trained head's.)
        for h in detector.predictor.heads:
            h['score'].weight.mul_(60.0)
        loss_e, dets, state = step_fn(1, 'eval', (imgs, gt), state)
        s_e, l_e, pri = detector(imgs.to(dev))
    assert np.array_equal(pri.cpu().numpy().view(np.uint32), anchors.view(np.uint32))
    ref = oracle.postprocess(s_e.cpu().numpy(), l_e.cpu().numpy(), anchors, softmax=True, nms_thr=0.45)
    assert len(dets) == B and all(d.shape[1] == 6 for d in dets)
    # row by row (class ids exact, scores 1e-5 relative, boxes 1e-4), a row may differ only on a selection boundary: the strict checker of
    # tests/test_postprocess_gpu.py
    from test_postprocess_gpu import Boundaries, compare
    compare(dets, ref, boundaries=Boundaries(s_e.cpu().numpy(), 21, True))

    # predict_single surface (detector_wrapper.py:49-65) without a preprocess pipeline
    wrapper.preprocess = None
    res = wrapper.predict_single(imgs[0])
    assert res.dim() == 2 and res.shape[1] == 6


RETINA = {
    'base': {'name': 'torchvision_resnet50', 'pretrained': False},
    'detector': {'num_classes': 80, 'use_depthwise': False,
                 'features': {'name': 'FeaturePyramid', 'out_layers': (5, 6, 7), 'pyramid_layers': 5, 'pyramid_channels': 256,
                              'initializer': {'name': 'normal_', 'args': {'mean': 0, 'std': 0.03}}},
                 'predictor': {'num_layers': 4, 'num_channels': 256, 'kernel_size': 3,
                               'activation': {'name': 'ReLU', 'args': {'inplace': True}},
                               'initializer': {'name': 'normal_', 'args': {'mean': 0, 'std': 0.01}}},
                 'heads': {'initializer': {'name': 'normal_', 'args': {'mean': 0, 'std': 0.01}}, 'score_head_bias_init': -4.6}},
    'anchor_generator': {'type': 'retina_net', 'min_level': 3, 'max_level': 7, 'aspect_ratios': [1.0, 2.0, 0.5], 'scale': 4.0,
                         'scales_per_level': 3},
}


def test_retina500_step_fn_train_and_eval():
    """samples/retina_rn50_500_coco.py wiring: FPN neck + shared-conv tower + focal loss (naive sampler, the reference's
    reduction='mean' constructor quirk) + SIGMOID postprocess; A = 47 961."""
    torch.manual_seed(5)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, RETINA, {'xy_scale': 10.0, 'wh_scale': 5.0},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .5}, 'score_converter': 'SIGMOID'},
        {'classification_loss': {'name': 'SigmoidFocalLoss', 'gamma': 2.0, 'alpha': 0.25}, 'localization_loss': {'name': 'SmoothL1Loss'},
         'classification_weight': 1.0, 'localization_weight': 1.0},
        {'name': 'naive_sampler'}, {'matched_threshold': 0.5, 'unmatched_threshold': 0.4})
    detector = wrapper.model
    detector.train()
    B = 2
    imgs = torch.from_numpy(np.random.default_rng(23).standard_normal((B, 3, 500, 500), dtype=np.float32))
    gt_np = syn.make_ground_truth(B, 500, 80, seed=1, background=False)
    gt = [torch.from_numpy(g) for g in gt_np]
    state = init_state()
    loss, prediction, state = step_fn(0, 'train', (imgs, gt), state)
    scores, locs = prediction
    assert scores.shape == (B, 47961 * 80) and locs.shape == (B, 47961 * 4)
    cfg = syn.CONFIGS['retina_rn50_500_coco']
    anchors = oracle.anchors(cfg['anchor'], 500, cfg['levels'])
    target = oracle.encode_ground_truth(gt_np, anchors, 0.5, 0.4)
    s_np, l_np = scores.cpu().numpy(), locs.cpu().numpy()
    mask = oracle.naive_sampler(s_np, target)
    vals, _, _ = oracle.multibox_loss(s_np, l_np, anchors, target, mask, kind='focal', reduce_mean=True, grads=False)
    assert abs(loss.item() - vals[0]) <= 1e-4 + 1e-5 * abs(vals[0]), (loss.item(), vals)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in detector.parameters() if p.requires_grad)

    detector.eval()
    with torch.no_grad():
        _, dets, state = step_fn(1, 'eval', (imgs, gt), state)
        s_e, l_e, pri = detector(imgs.to(dev))
    assert np.array_equal(pri.cpu().numpy().view(np.uint32), anchors.view(np.uint32))
    ref = oracle.postprocess(s_e.cpu().numpy(), l_e.cpu().numpy(), anchors, softmax=False, nms_thr=0.5)
    for d, r in zip(dets, ref):
        assert d.shape[1] == 6 and abs(d.shape[0] - r.shape[0]) <= 1
        n = min(d.shape[0], r.shape[0])
        if n:
            np.testing.assert_allclose(np.sort(d.cpu().numpy()[:n, 5]), np.sort(r[:n, 5]), rtol=1e-4, atol=1e-6)


M2DET = {
    'base': {'name': 'torchvision_vgg16_bn', 'pretrained': False},
    'detector': {'num_classes': 81,
                 'features': {'name': 'MultilevelFeaturePyramid', 'out_layers': (32, 42), 'last_feature_layer': 42, 'num_scales': 6,
                              'num_tums': 8, 'base_reduced_channels': [512, 256]}},
    'anchor_generator': {'type': 'ssd', 'num_scales': 6, 'min_scale': 0.07, 'max_scale': 1.05,
                         'aspect_ratios': [[1.0, 2.0]] + [[1.0, 2.0, 3.0]] * 3 + [[1.0, 2.0]] * 2},
}


def test_m2det512_step_fn_train():
    """samples/m2det_512_vgg16_coco.py wiring: MLFPN neck (8 TUMs x 6 scales + SFAM) -> 1024-channel heads; A = 24 528."""
    torch.manual_seed(7)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, M2DET, {'xy_scale': 10.0, 'wh_scale': 5.0},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SOFTMAX'},
        {'classification_loss': {'name': 'CrossEntropyLoss'}, 'localization_loss': {'name': 'SmoothL1Loss'},
         'classification_weight': 1.0, 'localization_weight': 1.0},
        {'name': 'hard_negative_mining', 'negative_per_positive_ratio': 3, 'min_negative_per_image': 5},
        {'matched_threshold': 0.5, 'unmatched_threshold': 0.5})
    detector = wrapper.model
    detector.train()
    B = 2
    imgs = torch.from_numpy(np.random.default_rng(29).standard_normal((B, 3, 512, 512), dtype=np.float32))
    gt_np = syn.make_ground_truth(B, 512, 81, seed=2)
    gt = [torch.from_numpy(g) for g in gt_np]
    loss, (scores, locs), state = step_fn(0, 'train', (imgs, gt), init_state())
    assert scores.shape == (B, 24528 * 81) and locs.shape == (B, 24528 * 4)
    cfg = syn.CONFIGS['m2det_512_vgg16_coco']
    anchors = oracle.anchors(cfg['anchor'], 512, cfg['levels'])
    target = oracle.encode_ground_truth(gt_np, anchors, 0.5, 0.5)
    s_np, l_np = scores.detach().cpu().numpy(), locs.detach().cpu().numpy()
    mask = oracle.hard_negative_mining(s_np, target, 3, 5)
    vals, _, _ = oracle.multibox_loss(s_np, l_np, anchors, target, mask, kind='ce', grads=False)
    assert abs(loss.item() - vals[0]) <= 1e-4 + 1e-5 * abs(vals[0]), (loss.item(), vals)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in detector.parameters() if p.requires_grad)
    detector.eval()
    with torch.no_grad():
        _, dets, _ = step_fn(1, 'eval', (imgs, gt), state)
    assert len(dets) == B and all(d.shape[1] == 6 for d in dets)


MB2 = {
    'base': {'name': 'torchvision_mobilenet_v2', 'pretrained': False},
    'detector': {'num_classes': 21, 'use_depthwise': True, 'features': {'name': 'Features', 'out_layers': (13, 18)},
                 'extras': {'layers': (('s', 512), ('s', 256), ('s', 256), ('s', 128))}},
    'anchor_generator': {'type': 'ssd', 'num_scales': 6, 'min_scale': 0.1, 'max_scale': 1.05,
                         'aspect_ratios': [[1.0, 2.0]] + [[1.0, 2.0, 3.0]] * 3 + [[1.0, 2.0]] * 2},
}


def test_ssd_mb2_step_fn_train_and_eval():
    """samples/ssd_mb2_voc.py (BASELINE config 0) through detection.init: depthwise extras on libssdk, A = 2 268."""
    torch.manual_seed(9)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, MB2, {'xy_scale': 10.0, 'wh_scale': 5.0},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SOFTMAX'},
        {'classification_loss': {'name': 'CrossEntropyLoss'}, 'localization_loss': {'name': 'SmoothL1Loss'},
         'classification_weight': 1.0, 'localization_weight': 1.0},
        {'name': 'hard_negative_mining', 'negative_per_positive_ratio': 3, 'min_negative_per_image': 5},
        {'matched_threshold': 0.5, 'unmatched_threshold': 0.5})
    detector = wrapper.model
    detector.train()
    B = 2
    imgs = torch.from_numpy(np.random.default_rng(31).standard_normal((B, 3, 300, 300), dtype=np.float32))
    gt_np = syn.make_ground_truth(B, 300, 21, seed=4)
    gt = [torch.from_numpy(g) for g in gt_np]
    loss, (scores, locs), state = step_fn(0, 'train', (imgs, gt), init_state())
    assert scores.shape == (B, 2268 * 21) and locs.shape == (B, 2268 * 4)
    cfg = syn.CONFIGS['ssd_mb2_voc']
    anchors = oracle.anchors(cfg['anchor'], 300, cfg['levels'])
    target = oracle.encode_ground_truth(gt_np, anchors, 0.5, 0.5)
    s_np, l_np = scores.detach().cpu().numpy(), locs.detach().cpu().numpy()
    mask = oracle.hard_negative_mining(s_np, target, 3, 5)
    vals, _, _ = oracle.multibox_loss(s_np, l_np, anchors, target, mask, kind='ce', grads=False)
    assert abs(loss.item() - vals[0]) <= 1e-4 + 1e-5 * abs(vals[0]), (loss.item(), vals)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in detector.parameters() if p.requires_grad)
    detector.eval()
    with torch.no_grad():
        _, dets, _ = step_fn(1, 'eval', (imgs, gt), state)
        s_e, l_e, pri = detector(imgs.to(dev))
    assert np.array_equal(pri.cpu().numpy().view(np.uint32), anchors.view(np.uint32))
    ref = oracle.postprocess(s_e.cpu().numpy(), l_e.cpu().numpy(), anchors, softmax=True, nms_thr=0.45)
    for d, r in zip(dets, ref):
        assert d.shape[1] == 6 and abs(d.shape[0] - r.shape[0]) <= 1


SSD512 = {
    'base': {'name': 'torchvision_vgg16_bn', 'pretrained': False},
    'detector': {'num_classes': 81, 'use_depthwise': False,
                 'features': {'name': 'Features', 'out_layers': (32, 42), 'last_feature_layer': 42},
                 'extras': {'layers': (('s', 512), ('s', 256), ('s', 256), ('s', 256), ('s', 256))}},
    'anchor_generator': {'type': 'ssd', 'num_scales': 7, 'min_scale': 0.1, 'max_scale': 1.05,
                         'aspect_ratios': [[1.0, 2.0]] + [[1.0, 2.0, 3.0]] * 4 + [[1.0, 2.0]] * 2},
}


def test_ssd512_step_fn_train():
    """samples/ssd_512_vgg16_coco.py through detection.init: seven levels, A = 24 564."""
    torch.manual_seed(13)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, SSD512, {'xy_scale': 10.0, 'wh_scale': 5.0},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SOFTMAX'},
        {'classification_loss': {'name': 'CrossEntropyLoss'}, 'localization_loss': {'name': 'SmoothL1Loss'},
         'classification_weight': 1.0, 'localization_weight': 1.0},
        {'name': 'hard_negative_mining', 'negative_per_positive_ratio': 3, 'min_negative_per_image': 5},
        {'matched_threshold': 0.5, 'unmatched_threshold': 0.5})
    detector = wrapper.model
    detector.train()
    B = 2
    imgs = torch.from_numpy(np.random.default_rng(37).standard_normal((B, 3, 512, 512), dtype=np.float32))
    gt_np = syn.make_ground_truth(B, 512, 81, seed=6)
    gt = [torch.from_numpy(g) for g in gt_np]
    loss, (scores, locs), state = step_fn(0, 'train', (imgs, gt), init_state())
    assert scores.shape == (B, 24564 * 81) and locs.shape == (B, 24564 * 4)
    cfg = syn.CONFIGS['ssd_512_vgg16_coco']
    anchors = oracle.anchors(cfg['anchor'], 512, cfg['levels'])
    target = oracle.encode_ground_truth(gt_np, anchors, 0.5, 0.5)
    s_np, l_np = scores.detach().cpu().numpy(), locs.detach().cpu().numpy()
    mask = oracle.hard_negative_mining(s_np, target, 3, 5)
    vals, _, _ = oracle.multibox_loss(s_np, l_np, anchors, target, mask, kind='ce', grads=False)
    assert abs(loss.item() - vals[0]) <= 1e-4 + 1e-5 * abs(vals[0]), (loss.item(), vals)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in detector.parameters() if p.requires_grad)


def test_detection_init_distributed_two_ranks(tmp_path):
    """detection.init(distributed=True) with two ranks (detection/init.py:80-86): DistributedDataParallel around the predictor, the
    hot-path BatchNorms on libssdk with their statistics all-reduced, the backbone's as SyncBatchNorm.  Both ranks use this box's one
    GPU and gloo; tests/ddp_worker.py holds the per-rank body and its cross-rank checks (equal averaged gradients from different
    images, equal running statistics)."""
    import os
    import sys
    from single_shot_detection_amd import launch
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ddp_worker.py')
    rc = launch.launch(2, [sys.executable, worker, str(tmp_path)])
    assert rc == 0
    assert all(os.path.exists(os.path.join(str(tmp_path), f'ok{r}.npy')) for r in range(2))


def test_rccl_world_of_one(tmp_path):
    """One REAL RCCL execution (backend 'nccl'), at world size 1, in a fresh child process: init_process_group('nccl', device_id=...),
    the ReduceOp.AVG probe, the 36 MB head-gradient bucket forced through dist.all_reduce with its zero-copy views, a packed fp64
    SyncBatchNorm buffer, destroy_process_group -- everything of the N > 1 exchange short of a second GPU (tests/rccl_worker.py)."""
    import json
    import os
    import sys
    from single_shot_detection_amd import launch
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rccl_worker.py')
    out = os.path.join(str(tmp_path), 'rccl.json')
    rc = launch.launch(1, [sys.executable, worker, out])
    assert rc == 0
    res = json.load(open(out))
    assert res['backend'] == 'nccl' and res['world'] == 1 and res['ipc_legacy_env'] == '0'
    assert res['avg_supported'] is True              # RCCL has ReduceOp.AVG: the average costs no extra pass
    assert res['bucket_bytes'] == 36046848 and res['views_alias_bucket'] and res['views_alias_after'] and res['copied_last'] == 0
    assert res['max_abs_change'] == 0.0 and res['finite'] and res['sums_ok'] and res['streamk_timeouts'] == 0


def test_graphed_eval_replays_match_the_eager_step():
    """single_shot_detection_amd.graphs: the evaluation step (pyramid tail + heads forward + postprocess) captured in a HIP graph and
    replayed on new inputs gives what the eagerly enqueued step gives.  Batch 2 of SSD-300: the head GEMM runs in its stream-K form,
    whose flags must survive being replayed with the same launch arguments (they are reset by their consumer)."""
    import bench
    from single_shot_detection_amd.graphs import GraphedCallable
    from test_postprocess_gpu import Boundaries, compare
    dev = torch.device('cuda:0')
    hp = bench.HotPath('ssd_300_vgg16_voc', 2, dev)
    hp.heads.eval()
    if hp.extras is not None:
        hp.extras.eval()

    def step(*taps):
        hp.inputs = list(taps)
        return hp.eval_step()

    first = [t.detach().clone() for t in hp.inputs]
    graphed = GraphedCallable(step, first)
    assert graphed.scratch_allocated_in_capture == 0   # every workspace was made by the warm-up calls, none inside the graph's pool
    gen = torch.Generator(device=dev).manual_seed(77)
    for trial in range(3):   # the captured inputs again, then two new sets (the second replay would meet the first one's flags)
        taps = first if trial == 0 else [torch.randn(t.shape, device=dev, generator=gen).contiguous(memory_format=torch.channels_last) for t in first]
        rows, counts = graphed(*taps)
        rows, counts = rows.clone(), counts.clone()
        ref_rows, ref_counts = step(*taps)
        n, m = counts.cpu().numpy(), ref_counts.cpu().numpy()
        assert np.abs(n - m).max() <= 1
        with torch.no_grad():   # (the logits behind both results, up to the head GEMM's summation order: they name the selection boundaries)
            hp.inputs = list(taps)
            logits = hp.forward_heads()[0].cpu().numpy()
        compare([rows[i, :n[i]] for i in range(len(n))], [ref_rows[i, :m[i]].cpu().numpy() for i in range(len(m))],
                boundaries=Boundaries(logits, hp.C, True))


@pytest.mark.parametrize('cfg_name,batch', [('ssd_mb2_voc', 2), ('ssd_300_vgg16_voc', 2), ('retina_rn50_500_coco', 2)])
def test_graphed_training_steps_match_eager_ones(cfg_name, batch):
    """The whole training step (pyramid tail + heads forward, match, sampler, loss, backward, fused SGD) captured in a HIP graph with the
    ground truth in a PackedGroundTruth: every replay moves the parameters like the eagerly enqueued step does.  (Found with this
    check: a hipMemsetAsync node that stopped zeroing the loss counters from the second replay on -- the library zero-fills with kernels.)"""
    import bench
    from single_shot_detection_amd.detection.target_assigner import PackedGroundTruth
    from single_shot_detection_amd.graphs import GraphedCallable
    dev = torch.device('cuda:0')
    eager, graphed = bench.HotPath(cfg_name, batch, dev), bench.HotPath(cfg_name, batch, dev)
    graphed.gt = PackedGroundTruth.from_list(graphed.gt, dev, capacity=sum(len(g) for g in graphed.gt) + 7)   # (padding rows are skipped)

    def params(hp):
        return [p for g in hp.opt.param_groups for p in g['params']]

    step = GraphedCallable(graphed.train_step, [], warmup=3)
    assert step.scratch_allocated_in_capture == 0   # (nor is the stream-K workspace's zero-fill a node of the graph)
    for _ in range(3):
        eager.train_step()
    start = [q.detach().clone() for q in params(eager)]
    for k in range(4):
        loss_e = eager.train_step()
        loss_g = step()
        torch.cuda.synchronize()
        assert abs(float(loss_e.detach()) - float(loss_g.detach())) <= 2e-4 * abs(float(loss_e.detach())) + 1e-6, (k, float(loss_e.detach()), float(loss_g.detach()))
        for p, q, q0 in zip(params(graphed), params(eager), start):
            # 0.2 % of the parameter's size, plus 5 % of how far these steps have moved it: the default mode's atomics (legacy heads,
            # split-K tail) retire in another order in a replay, and a parameter of size 2e-4 (a bias that started at 0) is all update --
            # seen once at 1.3 % of it; a dead or stale graph node is off by the whole update.  Bit-for-bit: the deterministic-mode test.
            scale = float(q.detach().abs().max()) + 1e-12
            moved = float((q.detach() - q0).abs().max())
            assert float((p.detach() - q.detach()).abs().max()) <= 2e-3 * scale + 5e-2 * moved, k


def _hot_path_state(hp):
    """Every tensor a training step reads and writes besides its inputs: parameters, BatchNorm buffers, SGD momentum."""
    mods = [m for m in (hp.heads, hp.extras, hp.tower, hp.neck) if m is not None]
    out = [p for p in hp.params]
    out += [b for m in mods for n, b in m.named_buffers() if not n.startswith('base.')]
    out += [hp.opt.state[p]['momentum_buffer'] for p in hp.params]
    return out


def _copy_state(src, dst):
    with torch.no_grad():
        for a, b in zip(_hot_path_state(src), _hot_path_state(dst)):
            b.copy_(a)   # (in place: the captured graph reads these very buffers)


@pytest.mark.parametrize('cfg_name,batch', [('m2det_512_vgg16_coco', 2), ('retina_rn50_500_coco', 2)])
def test_graphed_training_step_is_within_the_eager_steps_own_spread(cfg_name, batch):
    """m2det_512_vgg16_coco's step is not a reproducible function of its state in fp32: the MLFPN neck is ~130 conv -> BatchNorm layers
    deep with statistics over as few as 8 rows, the order of the split-K / scatter atomics differs from run to run, and that rounding
    noise grows ~4x per TUM (tools/determinism_fwd.py: 1e-7 after the first TUM, 1e-4 after the eighth; gradients of the first layers
    differ by several % between two EAGER runs from the same state -- round 2's "graph replay disagrees with eager on m2det" was this,
    plus a miscounted step).  So a replay is held to the eager step's own run-to-run spread: from ONE state (copied in place into the
    captured step's buffers) an eager step A, a second eager step B and a replay G; G - A must not be larger than a few times B - A
    plus a small share of the step itself (per tensor 10 % of its update, in aggregate 5 %, the loss 0.5 %; with 5 / 2.5 / 0.2 % the
    M2Det case failed once in about a dozen runs on the GPU boxes -- the check is statistical by nature): two eager steps enqueued
    back to back by the same process tend to retire their atomics alike (round 4 saw a pair 0.005 % apart on a tensor where the replay,
    whose kernels start at other times, was 1.4 % away), a dead or stale graph node moves a tensor by its whole update.  (Round 3
    needed 10 % / 5 %: its eager steps also multiplied the data gradients with weight layouts of an OLD step --
    ops.prepare_weight_transposes trusted the parameters' version counters, which a fused optimizer step does not bump -- while the
    captured step re-laid them out every replay.)  The strict form of this check is test_deterministic_mode_steps_are_bit_identical:
    under ops.deterministic() eager, eager and replay agree bit for bit on this network.  Two rounds, so that the
    second replay also meets what the first one left behind."""
    import bench
    from single_shot_detection_amd.detection.target_assigner import PackedGroundTruth
    from single_shot_detection_amd.graphs import GraphedCallable
    dev = torch.device('cuda:0')
    a, b, g = (bench.HotPath(cfg_name, batch, dev) for _ in range(3))
    g.gt = PackedGroundTruth.from_list(g.gt, dev, capacity=sum(len(t) for t in g.gt) + 7)
    for _ in range(2):
        a.train_step()
    b.train_step()
    step = GraphedCallable(g.train_step, [], warmup=3)
    assert step.scratch_allocated_in_capture == 0
    for rnd in range(2):
        _copy_state(a, b)
        _copy_state(a, g)
        before = [t.detach().clone() for t in _hot_path_state(a)]
        loss_a, loss_b, loss_g = a.train_step(), b.train_step(), step()
        torch.cuda.synchronize()
        la, lb, lg = float(loss_a.detach()), float(loss_b.detach()), float(loss_g.detach())
        # (the spread of ONE eager pair can be anything from 0 -- the atomics happened to fall in the same order -- to several %: every
        # bound below also allows a fixed share of the step's own size, far below what a dead or stale node would cost)
        assert abs(lg - la) <= 3 * abs(lb - la) + 5e-3 * abs(la), (rnd, la, lb, lg)
        num = den = upd2 = 0.0
        worst = (-1.0, -1)
        for i, (ta, tb, tg, t0) in enumerate(zip(_hot_path_state(a), _hot_path_state(b), _hot_path_state(g), before)):
            ta, tb, tg = ta.detach(), tb.detach(), tg.detach()
            upd = float((ta.double() - t0.double()).norm())
            dg, db = float((tg.double() - ta.double()).norm()), float((tb.double() - ta.double()).norm())
            num, den, upd2 = num + dg * dg, den + db * db, upd2 + upd * upd
            if upd > 0:
                assert dg <= 8 * db + 0.10 * upd, (rnd, i, tuple(ta.shape), dg, db, upd)   # per tensor: within the spread (+ 10 % of its update)
                worst = max(worst, (dg / upd, i))
        assert num <= 6.0 * den + 0.05 ** 2 * upd2 + 1e-12, (rnd, num, den, upd2, worst)   # in aggregate: one more sample of the same spread


def test_bench_n2_path_on_one_gpu_over_gloo():
    """`python bench.py --gpus 2` end to end (self-launched ranks, two-phase backward, zero-copy gradient buckets, synchronised BatchNorm
    statistics): both ranks share this box's GPU and the collectives run over gloo (SSDK_BENCH_ONE_GPU / SSDK_BENCH_BACKEND) -- the timing
    means nothing, the N > 1 code path is what is exercised; on a multi-GPU node the same command runs one rank per GPU over RCCL."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SSDK_BENCH_ONE_GPU='1', SSDK_BENCH_BACKEND='gloo')
    out = subprocess.run([sys.executable, os.path.join(repo, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1', '--full',
                          '--no-cpu-baseline', '--sync-bn', '--eval-steps', '1'], env=env, cwd=repo, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['rccl_ranks'] == 2 and line['collective_backend'] == 'gloo'
    assert line['config']['parallelism'] == 'dp2' and line['config']['sync_bn'] is True and line['config']['global_batch'] == 64
    assert line['scaling'] == 'weak' and line['value'] > 0 and line['grad_bucket_bytes']['heads'] == 36046848
    assert line['streamk_timeouts'] == 0   # two ranks time-slicing one card: every stream-K partner still arrived
    # the exchange detection.init(distributed=True) runs: heads' ring first and from a hook (under the tail's backward), zero-copy
    assert line['exchange']['start_order'] == [0, 1] and 0 in line['exchange']['started_early'] and line['exchange']['heads_copied'] == 0
    # ... and the line explains itself: per bucket the ring's start -> join time and how long the join stalled (device events)
    ex = line['exchange']
    assert len(ex['buckets']) == 2 and ex['buckets'][0]['bytes'] == 36046848 and ex['recovered_steps'] == 0
    assert all(t is not None and t >= 0.0 for t in ex['exposed_ms']) and all(t is not None and t > 0.0 for t in ex['ring_ms'])
    assert all(e <= r + 1e-3 for e, r in zip(ex['exposed_ms'], ex['ring_ms']))


def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: the line holds the headline fields of exactly K timed steps and
    none of the --full legs; DIR holds the last step's outputs as float32 .npy files, arrays above bench.DUMP_SAMPLE elements as a sample.
    Two runs with the same arguments write the same outputs to rounding: the last step starts from the state before the first one (over
    tens of SGD steps the default mode's rounding differences otherwise grow well beyond rounding)."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for r in range(2):
        dump = tmp_path / f'out{r}'
        out = subprocess.run([sys.executable, os.path.join(repo, 'bench.py'), '--gpus', '1', '--steps', '40', '--warmup', '5', '--batch', '2',
                              '--dump-outputs', str(dump)], cwd=repo, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        runs.append((json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1]), dump))
    line, dump = runs[0]
    assert line['unit'] == 'images/sec' and line['higher_is_better'] is True and line['dtype'] == 'f32' and line['steps'] == 40
    assert line['value'] > 0 and abs(line['ms_per_step'] - 2 * 1e3 / line['value']) < 1e-6 * line['ms_per_step']
    assert line['streamk_timeouts'] == 0 and line['roofline']['achieved'] > 0
    assert not {'cpu_baseline', 'per_config', 'roofline_hbm', 'nms_boxes_per_sec', 'deterministic'} & set(line)
    names = {'loss', 'class_loss', 'loc_loss', 'scores', 'locs', 'input_grad_0', 'input_grad_1', 'params', 'param_grads'}
    assert {f[:-4] for f in os.listdir(dump)} == names
    arrays = {n: np.load(dump / f'{n}.npy') for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
    assert arrays['loss'].shape == () and arrays['loss'] > 0
    assert arrays['scores'].shape == (1 << 20,) and arrays['locs'].ndim == 2 and arrays['locs'].shape[0] == 2
    assert arrays['input_grad_0'].shape == (1 << 20,) and arrays['input_grad_1'].shape == (2, 512, 18, 18)   # 2 x 512 x 37 x 37 is sampled
    assert np.abs(arrays['input_grad_0']).max() > 0 and np.abs(arrays['input_grad_1']).max() > 0
    assert arrays['params'].shape == arrays['param_grads'].shape == (1 << 20,) and np.abs(arrays['param_grads']).max() > 0
    for n, a in arrays.items():
        b = np.load(runs[1][1] / f'{n}.npy')
        assert b.shape == a.shape and np.abs(b.astype(np.float64) - a).max() <= 1e-5 * np.abs(a).max(), n


def test_hot_path_scopes_its_process_wide_switches():
    """bench.HotPath defers the pyramid tail's weight gradients inside train_step only (ops.deferred_weight_gradients): constructing one
    and stepping it leaves torch.autograd.grad with respect to a Conv2dBn weight working for everything else in the process, and the
    heads' fast mode where it was."""
    import bench
    from single_shot_detection_amd import _lib, ops
    from single_shot_detection_amd.bf.modules.conv import Conv2dBn
    dev = torch.device('cuda:0')
    hp = bench.HotPath('ssd_300_vgg16_voc', 2, dev)
    assert ops.defer_weight_gradients(False) is False      # (constructing it switched nothing on)
    hp.train_step()
    assert ops.defer_weight_gradients(False) is False and _lib.fast_mode is None
    assert all(p.grad is not None for p in hp.extras.parameters())   # (the deferred flush ran inside the step)
    blk = Conv2dBn(32, 32, kernel_size=3, padding=1, bias=False).to(dev).to(memory_format=torch.channels_last).train()
    x = torch.randn((2, 32, 6, 6), device=dev).contiguous(memory_format=torch.channels_last)
    (gw,) = torch.autograd.grad(blk(x).square().sum(), [blk.conv.weight])
    assert gw is not None and float(gw.abs().sum()) > 0.0
    with ops.deferred_weight_gradients():
        assert ops._defer_wgrad is True
        try:
            with ops.deferred_weight_gradients(False):
                raise RuntimeError('x')
        except RuntimeError:
            pass
        assert ops._defer_wgrad is True                     # (restored although the inner block raised)
    assert ops._defer_wgrad is False


@pytest.mark.parametrize('cfg_name,batch', [('ssd_300_vgg16_voc', 4), ('ssd_mb2_voc', 2), ('retina_rn50_500_coco', 2), ('m2det_512_vgg16_coco', 2)])
def test_deterministic_mode_steps_are_bit_identical(cfg_name, batch):
    """ops.set_deterministic (the reference runs cudnn.deterministic = True, bf/training/env.py:74-76): from ONE state, two eager training
    steps on two HotPaths and two replays of the captured step give the same bits -- loss, every parameter, BatchNorm buffer and momentum
    buffer -- over three consecutive steps (the state is copied once, then the three runs evolve on their own).  Off, the same network
    (m2det) differs by several % in its neck gradients between two eager runs (profiles/r03_determinism_grads.txt)."""
    import bench
    from single_shot_detection_amd import ops
    from single_shot_detection_amd.detection.target_assigner import PackedGroundTruth
    from single_shot_detection_amd.graphs import GraphedCallable
    dev = torch.device('cuda:0')
    with ops.deterministic():
        a, b, g = (bench.HotPath(cfg_name, batch, dev) for _ in range(3))
        g.gt = PackedGroundTruth.from_list(g.gt, dev, capacity=sum(len(t) for t in g.gt) + 7)
        a.train_step()
        b.train_step()
        step = GraphedCallable(g.train_step, [], warmup=2)
        assert step.scratch_allocated_in_capture == 0
        _copy_state(a, b)
        _copy_state(a, g)
        for k in range(3):
            loss_a, loss_b, loss_g = a.train_step(), b.train_step(), step()
            torch.cuda.synchronize()
            la, lb, lg = (float(t.detach()) for t in (loss_a, loss_b, loss_g))
            assert np.isfinite(la) and la == lb == lg, (k, la, lb, lg)
            for i, (ta, tb, tg) in enumerate(zip(_hot_path_state(a), _hot_path_state(b), _hot_path_state(g))):
                assert torch.equal(ta.detach(), tb.detach()), (k, i, tuple(ta.shape), float((ta.detach() - tb.detach()).abs().max()))
                assert torch.equal(ta.detach(), tg.detach()), (k, i, tuple(ta.shape), float((ta.detach() - tg.detach()).abs().max()))
            # ... and the gradients themselves (a parameter update could hide a difference below its rounding)
            for i, (p, q) in enumerate(zip(a.params, b.params)):
                assert torch.equal(p.grad, q.grad), (k, i, tuple(p.shape))


@pytest.mark.parametrize('cfg_name,batch', [('ssd_300_vgg16_voc', 4), ('m2det_512_vgg16_coco', 2)])
def test_deterministic_mode_computes_the_same_step(cfg_name, batch):
    """The deterministic forms are other decompositions of the same sums (dense instead of sparse data / weight gradients, no K split):
    one step from the same state gives the default mode's loss and gradients up to fp32 summation order."""
    import bench
    from single_shot_detection_amd import ops
    dev = torch.device('cuda:0')
    a, b = bench.HotPath(cfg_name, batch, dev), bench.HotPath(cfg_name, batch, dev)
    a.train_step()
    b.train_step()   # (the momentum buffers exist from the first step on)
    _copy_state(a, b)
    loss_a = float(a.train_step().detach())
    with ops.deterministic():
        loss_b = float(b.train_step().detach())
    assert abs(loss_a - loss_b) <= 1e-5 * abs(loss_a) + 1e-6, (loss_a, loss_b)
    if cfg_name.startswith('m2det'):
        return   # (its gradients are chaotic in the last bits of the forward pass: tools/determinism_fwd.py; the loss is what is compared)
    for i, (p, q) in enumerate(zip(a.params, b.params)):
        scale = float(p.grad.abs().max()) + 1e-12
        assert float((p.grad - q.grad).abs().max()) <= 1e-4 * scale, (i, tuple(p.shape), float((p.grad - q.grad).abs().max()), scale)


def test_training_step_hands_the_loss_row_mask_to_the_heads():
    """MultiboxLoss's backward under hard-negative mining writes which anchors carry a gradient (ssdk_multibox_loss_bwd_ex) and the heads'
    backward of the same pass takes it (ssdk_heads_bwd_ex: no scan of dscores): one hint per training step, and the step's gradients are
    those of the same step with the hand-over switched off."""
    import bench
    from single_shot_detection_amd.detection.modules import heads as heads_mod
    dev = torch.device('cuda:0')
    a, b = bench.HotPath('ssd_300_vgg16_voc', 4, dev), bench.HotPath('ssd_300_vgg16_voc', 4, dev)
    a.train_step()
    b.train_step()
    _copy_state(a, b)
    taken = heads_mod.row_hints_taken
    a.train_step()
    assert heads_mod.row_hints_taken == taken + 1
    orig = heads_mod.RowHint
    try:
        heads_mod.RowHint = lambda *args: None     # (the producer announces nothing: the heads scan)
        b.train_step()
    finally:
        heads_mod.RowHint = orig
    assert heads_mod.row_hints_taken == taken + 1
    for i, (p, q) in enumerate(zip(a.params, b.params)):
        scale = float(q.grad.abs().max()) + 1e-12
        assert float((p.grad - q.grad).abs().max()) <= 1e-4 * scale, (i, tuple(p.shape))


def test_split_heads_step_captures_into_a_hip_graph():
    """Regression guard for the abort of round 4 (hipStreamEndCapture crashed while capturing the split-heads step: a reference cycle kept
    earlier steps' default-stream AccumulateGrad nodes alive): two eager split steps, two warm-up steps on the capture stream, capture,
    one replay, in a child process (a crash there is a failed test, not a dead test run); the replayed step -- the fifth from the
    initial state -- has the loss of the fifth single-stream eager step from the same state."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, 'tests', 'capture_split_worker.py')], cwd=repo, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert res['timeouts'] == 0
    # the split only re-orders launches: eager split steps follow the single-stream ones, and the replay is step 5
    assert all(abs(a - b) <= 2e-4 * abs(b) for a, b in zip(res['eager'], res['ref'][:2])), res
    assert abs(res['replay'] - res['ref'][4]) <= 2e-4 * abs(res['ref'][4]), res


@pytest.mark.parametrize('model_name', ['ssd300', 'mb2'])
def test_step_fn_with_graphed_hot_path_equals_the_eager_step_fn(model_name, request):
    """detection.init(graph_hot_path=True): the libssdk part of the training step (pyramid tail + heads, target assignment, sampler + loss,
    their backward) replayed from two HIP graphs behind an eager PyTorch backbone (detection/init.py:108-135).  Under ops.deterministic()
    three steps with different images and ground truth give the same bits as the eager step_fn from the same state: losses, the running
    means step_fn keeps, and every parameter after SGD -- the backbone's too (its gradients come through the segment's input gradients)."""
    import copy
    from single_shot_detection_amd import ops
    dev = torch.device('cuda:0')
    if model_name == 'ssd300':
        model, size, B, ncls = MODEL, 300, 2, 21
    else:
        model = MB2
        size, B, ncls = 300, 2, 21
    args = ({'xy_scale': 10.0, 'wh_scale': 5.0},
            {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SOFTMAX'},
            {'classification_loss': {'name': 'CrossEntropyLoss'}, 'localization_loss': {'name': 'SmoothL1Loss'},
             'classification_weight': 1.0, 'localization_weight': 1.0},
            {'name': 'hard_negative_mining', 'negative_per_positive_ratio': 3, 'min_negative_per_image': 5},
            {'matched_threshold': 0.5, 'unmatched_threshold': 0.5})
    # (the backbone is stock PyTorch-ROCm: its convolutions must pick the same algorithm in both models for a bit-for-bit comparison --
    # what the reference asks of cuDNN on every GPU run, bf/training/env.py:74-76)
    prev_flags = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    request.addfinalizer(lambda: (setattr(torch.backends.cudnn, 'deterministic', prev_flags[0]), setattr(torch.backends.cudnn, 'benchmark', prev_flags[1])))
    with ops.deterministic():
        torch.manual_seed(11)
        w_e, init_e, step_e = det_init.init(dev, copy.deepcopy(model), *copy.deepcopy(args))
        w_g, init_g, step_g = det_init.init(dev, copy.deepcopy(model), *copy.deepcopy(args), graph_hot_path=True)
        w_g.model.load_state_dict(w_e.model.state_dict())
        with torch.no_grad():   # same taps from both backbones?  (checked first: everything below depends on it)
            probe = torch.randn((B, 3, size, size), device=dev)
            for _ in range(2):
                te, tg = w_e.model.predictor.features(probe), w_g.model.predictor.features(probe)
            assert all(torch.equal(a, b) for a, b in zip(te[0], tg[0])), 'the two PyTorch backbones do not agree bit for bit on this box'
        opt_e = torch.optim.SGD(w_e.model.parameters(), lr=1e-3, momentum=0.9)
        opt_g = torch.optim.SGD(w_g.model.parameters(), lr=1e-3, momentum=0.9)
        w_e.model.train()
        w_g.model.train()
        st_e, st_g = init_e(), init_g()
        rng = np.random.default_rng(31)
        for k in range(3):
            imgs = torch.from_numpy(rng.standard_normal((B, 3, size, size), dtype=np.float32))
            gt = [torch.from_numpy(g) for g in syn.make_ground_truth(B, size, ncls, seed=40 + k)]
            opt_e.zero_grad(set_to_none=True)
            opt_g.zero_grad(set_to_none=True)
            loss_e, pred_e, st_e = step_e(k, 'train', (imgs, gt), st_e)
            loss_g, pred_g, st_g = step_g(k, 'train', (imgs, gt), st_g)
            assert torch.equal(pred_e[0], pred_g[0]) and torch.equal(pred_e[1], pred_g[1]), (k, float((pred_e[0] - pred_g[0]).abs().max()), float((pred_e[1] - pred_g[1]).abs().max()))
            assert float(loss_e.detach()) == float(loss_g.detach()), (k, float(loss_e.detach()), float(loss_g.detach()))
            assert st_e == st_g, (k, st_e, st_g)
            loss_e.backward()
            loss_g.backward()
            for (n, p), q in zip(w_e.model.named_parameters(), w_g.model.parameters()):
                assert (p.grad is None) == (q.grad is None), n
                if p.grad is not None:
                    assert torch.equal(p.grad, q.grad), (k, n, float((p.grad - q.grad).abs().max()))
            opt_e.step()
            opt_g.step()
        for (n, p), q in zip(w_e.model.named_parameters(), w_g.model.parameters()):
            assert torch.equal(p, q), n
        # the eval phase of the same step_fn stays eager
        w_g.model.eval()
        with torch.no_grad():
            _, dets, _ = step_g(0, 'eval', (imgs, gt), init_g())
        assert len(dets) == B
