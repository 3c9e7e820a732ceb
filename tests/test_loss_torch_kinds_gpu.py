"""GPU: the torch loss options of MultiboxLoss on the fused kernels (csrc/loss.hip) -- CrossEntropyLoss label_smoothing / weight, L1Loss,
MSELoss, HuberLoss, SmoothL1Loss beta=0 -- against the reference's goldens (tests/golden/losses_torch.npz), against a torch-CPU
restatement at full size, in deterministic mode, through the C ABI's refusals, and under detection.init(graph_hot_path=True)."""
import copy
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import oracle
from single_shot_detection_amd import _lib, ops, synthetic as syn
from single_shot_detection_amd.detection import sampler
from single_shot_detection_amd.detection.box_coder import BoxCoder
from single_shot_detection_amd.detection.losses.multibox_loss import MultiboxLoss
from conftest import GOLDEN, dense_from_rows, load_golden
from loss_torch_cases import CASES, encode_target, torch_multibox_loss, with_weight

pytestmark = pytest.mark.gpu

HNM = functools.partial(sampler.hard_negative_mining, negative_per_positive_ratio=3, min_negative_per_image=5)


def _sampler(name):
    return HNM if name == 'hnm' else sampler.naive_sampler


@pytest.mark.parametrize('tag', sorted(CASES))
def test_torch_kinds_vs_reference_golden(tag):
    g = np.load(os.path.join(GOLDEN, 'losses_torch.npz'))
    smp, cl, ll = CASES[tag]
    anchors_np = load_golden('ssd_mb2_voc')['anchors']
    B, A, C = 2, anchors_np.shape[0], 21
    crit = MultiboxLoss(sampler=_sampler(smp), box_coder=BoxCoder(10.0, 5.0), classification_loss=with_weight(cl, torch.from_numpy(g['class_weight'])),
                        localization_loss=ll)
    s_t = torch.from_numpy(syn.make_logits(B, A, C, seed=2)).cuda().requires_grad_(True)
    l_t = torch.from_numpy(syn.make_locs(B, A, seed=3, scale=0.5)).cuda().requires_grad_(True)
    target = torch.from_numpy(g['target'].copy()).cuda()
    loss, class_loss, loc_loss = crit((s_t, l_t), torch.from_numpy(anchors_np).cuda(), target)
    loss.backward()
    ref_mask = np.unpackbits(g[tag + '_sampled_bits'], axis=1)[:, :A].astype(bool)
    mask = crit.last_sampled_mask.cpu().numpy().astype(bool)
    assert np.array_equal(mask, ref_mask)
    np.testing.assert_allclose([loss.item(), class_loss.item(), loc_loss.item()], g[tag + '_values'], rtol=1e-5)
    np.testing.assert_allclose(s_t.grad.view(B, A, C).cpu().numpy(), dense_from_rows(g[tag + '_dscores_rows'], g[tag + '_dscores_vals'], (B, A, C)),
                               rtol=3e-4, atol=3e-7)
    np.testing.assert_allclose(l_t.grad.view(B, A, 4).cpu().numpy(), dense_from_rows(g[tag + '_dlocs_rows'], g[tag + '_dlocs_vals'], (B, A, 4)),
                               rtol=3e-4, atol=3e-7)
    # the in-place target mutation of multibox_loss.py:81-82, as the reference leaves it (tolerance of test_loss_gpu's encoded target)
    got = target.cpu().numpy()
    np.testing.assert_allclose(got[..., :4], g['target_encoded'][..., :4], rtol=1e-6, atol=2e-5)
    assert np.array_equal(got[..., 4:], g['target_encoded'][..., 4:])


FULL = {   # config, batch, sampler, classification_loss, localization_loss
    'ssd300_smooth_weight_l1': ('ssd_300_vgg16_voc', 32, 'hnm', {'name': 'CrossEntropyLoss', 'label_smoothing': 0.1, 'weight': 'class_weight'},
                                {'name': 'L1Loss'}),
    'ssd300_weight_huber': ('ssd_300_vgg16_voc', 32, 'hnm', {'name': 'CrossEntropyLoss', 'weight': 'class_weight'}, {'name': 'HuberLoss', 'delta': 0.3}),
    'retina500_smooth_mse': ('retina_rn50_500_coco', 8, 'naive', {'name': 'CrossEntropyLoss', 'label_smoothing': 0.05}, {'name': 'MSELoss'}),
    'retina500_beta0': ('retina_rn50_500_coco', 8, 'hnm', {'name': 'CrossEntropyLoss'}, {'name': 'SmoothL1Loss', 'beta': 0.0}),
}


@pytest.mark.parametrize('case', sorted(FULL))
def test_full_size_vs_torch_restatement(case):
    """SSD-300 (81 classes, batch 32) and RetinaNet-500 (as a softmax detector of 81 classes) against multibox_loss.py:59-94 restated
    on torch's own loss modules on CPU, on the GPU sampler's mask (checked against the oracle's hard-negative mining)."""
    name, batch, smp, cl, ll = FULL[case]
    cfg = syn.CONFIGS[name]
    anchors_np = load_golden(name)['anchors']
    A, C = anchors_np.shape[0], 81
    gt = syn.make_ground_truth(batch, cfg['size'], C, seed=21, background=True)
    target_np = oracle.encode_ground_truth(gt, anchors_np, cfg['matched'], cfg['unmatched'])
    logits = syn.make_logits(batch, A, C, seed=22, trained_like=True)
    locs = syn.make_locs(batch, A, seed=23, scale=0.5)
    weight = torch.from_numpy(np.random.default_rng(5).uniform(0.25, 2.0, C).astype(np.float32))
    cl = with_weight(cl, weight)
    crit = MultiboxLoss(sampler=_sampler(smp), box_coder=BoxCoder(10.0, 5.0), classification_loss=cl, localization_loss=ll,
                        classification_weight=0.7, localization_weight=1.3)
    s_t = torch.from_numpy(logits).cuda().requires_grad_(True)
    l_t = torch.from_numpy(locs).cuda().requires_grad_(True)
    target = torch.from_numpy(target_np.copy()).cuda()
    loss, class_loss, loc_loss = crit((s_t, l_t), torch.from_numpy(anchors_np).cuda(), target)
    (2.0 * class_loss + 0.5 * loc_loss).backward()       # non-unit upstream gradients
    mask = crit.last_sampled_mask.cpu().numpy().astype(bool)
    if smp == 'hnm':
        ref_mask = oracle.hard_negative_mining(logits, target_np, 3, 5)
        assert (mask != ref_mask).sum() <= 8
    enc = encode_target(torch.from_numpy(target_np), torch.from_numpy(anchors_np))
    np.testing.assert_allclose(target.cpu().numpy(), enc.numpy(), rtol=1e-6, atol=2e-5)
    s_c = torch.from_numpy(logits).requires_grad_(True)
    l_c = torch.from_numpy(locs).requires_grad_(True)
    # (on the target as the kernel encoded it: an ulp of the encode must not flip the sign of an L1 gradient)
    ref = torch_multibox_loss(s_c, l_c, target.cpu(), torch.from_numpy(mask), cl, ll, 0.7, 1.3)
    (2.0 * ref[1] + 0.5 * ref[2]).backward()
    np.testing.assert_allclose([loss.item(), class_loss.item(), loc_loss.item()], [float(v) for v in ref], rtol=1e-5)
    np.testing.assert_allclose(s_t.grad.cpu().numpy(), s_c.grad.numpy(), rtol=3e-4, atol=3e-7)
    np.testing.assert_allclose(l_t.grad.cpu().numpy(), l_c.grad.numpy(), rtol=3e-4, atol=3e-7)


def test_deterministic_mode_is_bit_identical_for_a_new_kind():
    cfg = syn.CONFIGS['ssd_300_vgg16_voc']
    anchors = torch.from_numpy(load_golden('ssd_300_vgg16_voc')['anchors']).cuda()
    A, C, B = anchors.shape[0], 81, 16
    gt = syn.make_ground_truth(B, cfg['size'], C, seed=4, background=True)
    target_np = oracle.encode_ground_truth(gt, anchors.cpu().numpy(), cfg['matched'], cfg['unmatched'])
    logits = torch.from_numpy(syn.make_logits(B, A, C, seed=6, trained_like=True)).cuda()
    locs = torch.from_numpy(syn.make_locs(B, A, seed=7, scale=0.5)).cuda()
    weight = torch.linspace(0.5, 1.5, C)
    crit = MultiboxLoss(sampler=HNM, box_coder=BoxCoder(10.0, 5.0),
                        classification_loss={'name': 'CrossEntropyLoss', 'label_smoothing': 0.1, 'weight': weight},
                        localization_loss={'name': 'HuberLoss', 'delta': 0.5})
    runs = []
    with ops.deterministic():
        for _ in range(2):
            s = logits.clone().requires_grad_(True)
            l = locs.clone().requires_grad_(True)
            out = crit((s, l), anchors, torch.from_numpy(target_np.copy()).cuda())
            out[0].backward()
            runs.append([t.detach().clone() for t in out] + [s.grad.clone(), l.grad.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_c_abi_refuses_bad_new_fields():
    """ssdk_multibox_loss_fwd / _bwd refuse the new fields outside their range or kind, before any launch."""
    lib = _lib.lib()
    B, A, C = 1, 64, 5
    dev = torch.device('cuda:0')
    scores = torch.zeros((B, A * C), device=dev)
    locs = torch.zeros((B, A * 4), device=dev)
    anchors = torch.ones((A, 4), device=dev)
    target = torch.zeros((B, A, 6), device=dev)
    sampled = torch.ones((B, A), dtype=torch.uint8, device=dev)
    out3 = torch.empty((3,), device=dev)
    grad = torch.ones((2,), device=dev)
    ds, dl = torch.empty_like(scores), torch.empty_like(locs)
    w = torch.ones((C,), device=dev)
    from single_shot_detection_amd.detection import sampler as smp
    ws = smp.loss_workspace(B, A, C, dev)

    def params(cls_kind=0, loc_kind=0, beta=1.0, ls=0.0, weight=None):
        return _lib.LossParams(cls_kind, loc_kind, 2.0, 0.25, 0, 0.0, 1.0, 1.0, 10.0, 5.0, 1e-8, beta, ls, weight)

    bad = [params(loc_kind=5), params(loc_kind=4, beta=0.0), params(loc_kind=0, beta=-1.0), params(ls=1.5), params(ls=-0.1),
           params(cls_kind=1, ls=0.1), params(cls_kind=3, weight=w.data_ptr())]
    for p in bad:
        rc = lib.ssdk_multibox_loss_fwd(ctypes.byref(p), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target),
                                        _lib.ptr(sampled), B, A, C, 0, _lib.ptr(out3), _lib.ptr(ws), ws.numel(), _lib.current_stream())
        assert rc == -1, (p.cls_kind, p.loc_kind, p.smooth_l1_beta, p.ce_label_smoothing)
        rc = lib.ssdk_multibox_loss_bwd(ctypes.byref(p), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target),
                                        _lib.ptr(sampled), _lib.ptr(grad), B, A, C, _lib.ptr(ds), _lib.ptr(dl), _lib.ptr(ws), ws.numel(),
                                        _lib.current_stream())
        assert rc == -1
    torch.cuda.synchronize()


MB2 = {
    'base': {'name': 'torchvision_mobilenet_v2', 'pretrained': False},
    'detector': {'num_classes': 21, 'use_depthwise': True, 'features': {'name': 'Features', 'out_layers': (13, 18)},
                 'extras': {'layers': (('s', 512), ('s', 256), ('s', 256), ('s', 128))}},
    'anchor_generator': {'type': 'ssd', 'num_scales': 6, 'min_scale': 0.1, 'max_scale': 1.05,
                         'aspect_ratios': [[1.0, 2.0]] + [[1.0, 2.0, 3.0]] * 3 + [[1.0, 2.0]] * 2},
}


def test_graphed_hot_path_with_label_smoothing_and_l1_equals_the_eager_step_fn(request):
    """detection.init(graph_hot_path=True) with CrossEntropyLoss(label_smoothing, weight) + L1Loss: under ops.deterministic() three steps
    give the bits of the eager step_fn from the same state -- losses, running means and every parameter after SGD (the class weights are
    read from the loss object's device copy at the address the captured graphs hold)."""
    from single_shot_detection_amd.detection import init as det_init
    dev = torch.device('cuda:0')
    size, B, ncls = 300, 2, 21
    args = ({'xy_scale': 10.0, 'wh_scale': 5.0},
            {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SOFTMAX'},
            {'classification_loss': {'name': 'CrossEntropyLoss', 'label_smoothing': 0.1, 'weight': torch.linspace(0.5, 1.5, ncls)},
             'localization_loss': {'name': 'L1Loss'}, 'classification_weight': 1.0, 'localization_weight': 1.0},
            {'name': 'hard_negative_mining', 'negative_per_positive_ratio': 3, 'min_negative_per_image': 5},
            {'matched_threshold': 0.5, 'unmatched_threshold': 0.5})
    prev_flags = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    request.addfinalizer(lambda: (setattr(torch.backends.cudnn, 'deterministic', prev_flags[0]), setattr(torch.backends.cudnn, 'benchmark', prev_flags[1])))
    with ops.deterministic():
        torch.manual_seed(11)
        w_e, init_e, step_e = det_init.init(dev, copy.deepcopy(MB2), *copy.deepcopy(args))
        w_g, init_g, step_g = det_init.init(dev, copy.deepcopy(MB2), *copy.deepcopy(args), graph_hot_path=True)
        w_g.model.load_state_dict(w_e.model.state_dict())
        with torch.no_grad():
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
            assert torch.equal(pred_e[0], pred_g[0]) and torch.equal(pred_e[1], pred_g[1]), k
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
