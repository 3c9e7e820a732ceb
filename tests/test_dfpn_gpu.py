"""GPU: DepthwiseFeaturePyramid (Tiny-DSOD D-FPN, bf/modules/features.py:123-212) on libssdk -- against the REFERENCE's own class
(tests/golden/dfpn_small.npz, tools/gen_golden_dfpn.py), against the same graph on stock torch CPU ops, kernel by kernel, in deterministic
mode, under a dispatch recorder (no stock kernel on the hot path), for the stock-module variants, through detection.init, with synchronised
BatchNorm over two ranks and replayed from a HIP graph."""
import copy
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dfpn_cases
from blocks_cases import _StubBase
from conftest import GOLDEN
from single_shot_detection_amd import ops
from single_shot_detection_amd.bf.modules import conv, features

pytestmark = pytest.mark.gpu

BAR = 2e-5   # the reference-golden bar of test_blocks_golden_gpu.py: outputs, the input gradient, BatchNorm buffers
# Parameter gradients: 5e-5 on the same scale-relative form.  The first downsample level's norms sit under six levels of the pyramid and
# the up path back (stub6: four training-mode norms over as few as 12 values per channel between them and the outputs); one gamma element of
# the 3 x 2 level came out at 1.2 x the 2e-5 bar on the MI355X, every other element of every gradient below it.
BAR_GRAD = 5e-5


def _close(got, want, bar=1e-4, err_msg='', scale=None):
    """test_conv_bn_gpu._close: |got - want| <= bar * (|want| + max|want|) for every element."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (err_msg, got.shape, want.shape)
    if scale is None:
        scale = float(np.abs(want).max()) if want.size else 0.0
    err = np.abs(got - want)
    tol = bar * (np.abs(want) + scale) + 1e-12
    bad = err > tol
    assert not bad.any(), (err_msg, int(bad.sum()), float((err / tol).max()), scale)


# ---- the same graph on stock torch ops (CPU reference of features.py:177-209) -----------------------------------------------------

def _cbr(blk, x):   # Conv2dBn (bf/modules/conv.py:30-36)
    x = blk.bn(blk.conv(x))
    return blk.activation(x) if 'activation' in blk._modules else x


def _dwbr(blk, x):   # DepthwiseConv2dBn (bf/modules/conv.py:72-85)
    for name in ('depthwise_conv', 'depthwise_bn', 'depthwise_activation', 'pointwise_conv', 'pointwise_bn', 'pointwise_activation'):
        if name in blk._modules:
            x = blk._modules[name](x)
    return x


def _ref_neck(m, sources):
    feats = [lat(s) for s, lat in zip(sources, m.pyramid_lateral)]
    for down in m.downsample:
        f = feats[-1]
        pad = [0, 1 if f.shape[3] > 2 else 0, 0, 1 if f.shape[2] > 2 else 0]
        feats.append(torch.cat([_cbr(down[0][1], F.max_pool2d(F.pad(f, pad), 2)), _dwbr(down[1], f)], dim=1))
    out = [feats[-1]]
    for i in reversed(range(len(feats) - 1)):
        out.append(_cbr(m.up_conv[i], F.interpolate(out[-1], size=feats[i].shape[2:], mode=m.interpolation_mode)) + feats[i])
    return list(reversed(out))


def _taps(base, x):
    srcs, cur = [], x
    for i, layer in enumerate(base):
        cur = layer(cur)
        srcs.append(cur)
    return srcs


class _Taps(nn.Module):
    """Two backbone taps of the given channels at the given sizes of a 300 x 300 image (1 x 1 strided stand-ins)."""

    def __init__(self, c0, c1, s0, s1):
        super().__init__()
        self.features = nn.Sequential(nn.Conv2d(3, c0, 1, stride=s0), nn.Conv2d(c0, c1, 1, stride=s1))


def _randomize(m, rng):
    with torch.no_grad():
        for n, p in m.named_parameters():
            v = rng.standard_normal(tuple(p.shape), dtype=np.float32)
            if p.dim() > 1:
                p.copy_(torch.from_numpy(v * np.float32(np.sqrt(2.0 / np.prod(p.shape[1:])))))
            elif n.endswith('bn.weight'):
                p.copy_(torch.from_numpy(np.abs(v) * 0.5 + 0.5))
            else:
                p.copy_(torch.from_numpy(v * 0.1))


def _neck_params(m):
    return [(n, p) for n, p in sorted(m.named_parameters()) if not n.startswith('base.')]


def _compare_with_cpu(m_gpu, m_cpu, src_np, rng, bar=1e-4):
    """neck on libssdk vs _ref_neck on the CPU: outputs, tap gradients, parameter gradients, BatchNorm buffers."""
    sg = [torch.from_numpy(s).cuda().requires_grad_(True) for s in src_np]
    sr = [torch.from_numpy(s).requires_grad_(True) for s in src_np]
    outs_g, last = m_gpu.neck(sg)
    outs_r = _ref_neck(m_cpu, sr)
    assert last is outs_g[-1] and [o.shape for o in outs_g] == [o.shape for o in outs_r]
    for i, (a, b) in enumerate(zip(outs_g, outs_r)):
        _close(a.detach().cpu().numpy(), b.detach().numpy(), bar, f'y{i}')
    gs = [torch.from_numpy(rng.standard_normal(tuple(o.shape), dtype=np.float32)) for o in outs_r]
    torch.autograd.backward(outs_r, gs)
    torch.autograd.backward(outs_g, [g.cuda() for g in gs])
    for i, (a, b) in enumerate(zip(sg, sr)):
        _close(a.grad.cpu().numpy(), b.grad.numpy(), bar, f'dsrc{i}')
    for (n1, p1), (n2, p2) in zip(_neck_params(m_gpu), _neck_params(m_cpu)):
        assert n1 == n2
        _close(p1.grad.cpu().numpy(), p2.grad.numpy(), bar, n1)
    for (n1, b1), (n2, b2) in zip(sorted(m_gpu.named_buffers()), sorted(m_cpu.named_buffers())):
        np.testing.assert_allclose(b1.cpu().numpy(), b2.numpy(), rtol=1e-4, atol=1e-5, err_msg=n1)


# ---- 1. the reference's own class (golden) ---------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def golden_dfpn():
    return np.load(os.path.join(GOLDEN, 'dfpn_small.npz'))


@pytest.mark.parametrize('case', sorted(dfpn_cases.CASES))
def test_dfpn_vs_reference_golden(case, golden_dfpn):
    got = dfpn_cases.run_case(case, features.DepthwiseFeaturePyramid, torch.device('cuda'))
    want_keys = sorted(k for k in golden_dfpn.files if k.startswith(case + '/'))
    assert sorted(got) == want_keys, sorted(set(want_keys) ^ set(got))[:10]
    # a bias whose gradient is analytically ZERO (one_tap has no activation: the depthwise norm's beta shifts the pointwise convolution's
    # output by a per-channel constant that the next training-mode norm subtracts) holds rounding noise on both sides: its scale is that of
    # the mode's largest parameter gradient (test_conv_bn_gpu.test_m2det_neck_vs_torch's rule)
    gw_max = {mode: max(float(np.abs(golden_dfpn[k]).max()) for k in want_keys if f'/{mode}/dp/' in k and not k.endswith(('__shape', '__sum_l2')))
              for mode in ('eval', 'train')}
    for key in want_keys:
        ref, val = golden_dfpn[key], got[key]
        if key.endswith(('__shape', 'state_names', 'state_shapes', 'num_batches_tracked')):
            assert np.array_equal(ref, val), (key, ref, val)
        elif key.endswith('__sum_l2'):
            l2, bar = float(ref[1]), BAR_GRAD if '/dp/' in key else BAR
            assert abs(val[1] - ref[1]) <= bar * l2 + 1e-12, (key, val, ref)
            assert abs(val[0] - ref[0]) <= 10 * bar * l2 + 1e-12, (key, val, ref)
        else:
            mode = key.split('/')[1]
            zero_grad_bias = '/dp/' in key and key.endswith('bias') and float(np.abs(ref).max()) < 1e-3 * gw_max[mode]
            _close(val, ref, BAR_GRAD if '/dp/' in key else BAR, key, scale=gw_max[mode] if zero_grad_bias else None)


# ---- 2. SSD-MobileNetV2 geometry against stock torch on the CPU --------------------------------------------------------------------

def test_dfpn_mb2_geometry_vs_torch_cpu():
    """taps 96 @ 19 x 19 and 1280 @ 10 x 10 (mobilenet_v2 layers 13, 18 at 300 x 300), C = 128, batch 4, train mode: levels 19, 10, 5, 3, 2, 1."""
    rng = np.random.default_rng(17)
    torch.manual_seed(0)
    m = features.DepthwiseFeaturePyramid(_Taps(96, 1280, 16, 2), (0, 1), pyramid_layers=6, pyramid_channels=128)
    _randomize(m, rng)
    ref = copy.deepcopy(m).train()
    m = m.cuda().train()
    src = [rng.standard_normal((4, 96, 19, 19), dtype=np.float32), rng.standard_normal((4, 1280, 10, 10), dtype=np.float32)]
    _compare_with_cpu(m, ref, src, rng)


# ---- 3. the kernels against torch on the CPU ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W', [(10, 10), (5, 5), (3, 3), (2, 2), (10, 8), (5, 4), (3, 2), (2, 3), (9, 7), (19, 15)])
@pytest.mark.parametrize('kind', ['ties', 'normal'])
def test_maxpool2x2_bit_exact_vs_torch_cpu(H, W, kind):
    rng = np.random.default_rng(H * 100 + W)
    B, C = 2, 8
    if kind == 'ties':   # small integers: ties everywhere; a NaN; all-negative odd-edge windows (the pad's 0.0 wins)
        x = rng.integers(-2, 3, (B, C, H, W)).astype(np.float32)
        if H % 2:
            x[:, :, -1, :] = -rng.integers(1, 4, (B, C, W)).astype(np.float32)
        if W % 2:
            x[:, :, :, -1] = -rng.integers(1, 4, (B, C, H)).astype(np.float32)
        x[0, 1, 0, 0] = np.nan
        x[1, 3, H - 1, W - 1] = np.nan
    else:
        x = rng.standard_normal((B, C, H, W), dtype=np.float32)
    pb, pr = int(H > 2), int(W > 2)
    xr = torch.from_numpy(x).requires_grad_(True)
    xg = torch.from_numpy(x).cuda().requires_grad_(True)
    yr = F.max_pool2d(F.pad(xr, [0, pr, 0, pb]), 2)
    yg = ops.maxpool2x2(xg, pb, pr)
    assert np.array_equal(yg.detach().cpu().numpy(), yr.detach().numpy(), equal_nan=True)
    g = torch.from_numpy(rng.standard_normal(tuple(yr.shape), dtype=np.float32))
    yr.backward(g)
    yg.backward(g.cuda())
    assert np.array_equal(xg.grad.cpu().numpy(), xr.grad.numpy())


@pytest.mark.parametrize('hf,wf,hc,wc', [(2, 2, 1, 1), (3, 3, 2, 2), (5, 5, 3, 3), (10, 10, 5, 5), (19, 19, 10, 10), (38, 38, 19, 19),
                                         (15, 15, 8, 8), (38, 30, 19, 15), (19, 15, 10, 8), (5, 4, 3, 2), (3, 2, 2, 1), (2, 1, 1, 1)])
def test_depthwise_upsample_conv_vs_torch_cpu(hf, wf, hc, wc):
    rng = np.random.default_rng(hf * 1000 + wf * 10 + hc)
    B, C = 3, 16
    x = rng.standard_normal((B, C, hc, wc), dtype=np.float32)
    w = rng.standard_normal((C, 1, 3, 3), dtype=np.float32) * np.float32(0.3)
    bias = rng.standard_normal((C,), dtype=np.float32) if hf == 10 else None
    xr, wr = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    xg, wg = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(w).cuda().requires_grad_(True)
    br = None if bias is None else torch.from_numpy(bias).requires_grad_(True)
    bg = None if bias is None else torch.from_numpy(bias).cuda().requires_grad_(True)
    yr = F.conv2d(F.interpolate(xr, size=(hf, wf), mode='nearest'), wr, br, padding=1, groups=C)
    yg = ops.depthwise_upsample_conv2d(xg, wg, bg, (hf, wf))
    _close(yg.detach().cpu().numpy(), yr.detach().numpy(), err_msg='y')
    g = torch.from_numpy(rng.standard_normal(tuple(yr.shape), dtype=np.float32))
    yr.backward(g)
    yg.backward(g.cuda())
    _close(xg.grad.cpu().numpy(), xr.grad.numpy(), err_msg='dx')
    _close(wg.grad.cpu().numpy(), wr.grad.numpy(), err_msg='dw')
    if bias is not None:
        _close(bg.grad.cpu().numpy(), br.grad.numpy(), err_msg='db')


@pytest.mark.parametrize('chans', [(16, 16), (8, 4, 12), (64, 64)])
def test_concat_channels_bit_exact(chans):
    rng = np.random.default_rng(sum(chans))
    xs = [rng.standard_normal((2, c, 5, 7), dtype=np.float32) for c in chans]
    xr = [torch.from_numpy(x).requires_grad_(True) for x in xs]
    xg = [torch.from_numpy(x).cuda().requires_grad_(True) for x in xs]
    yr, yg = torch.cat(xr, dim=1), ops.concat_channels(xg)
    assert torch.equal(yg.detach().cpu(), yr.detach())
    g = torch.from_numpy(rng.standard_normal(tuple(yr.shape), dtype=np.float32))
    yr.backward(g)
    yg.backward(g.cuda())
    for a, b in zip(xg, xr):
        assert torch.equal(a.grad.cpu(), b.grad)


# ---- 4. deterministic mode ---------------------------------------------------------------------------------------------------------

def _stub6_taps(seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s, dtype=np.float32) for s in ((2, 16, 38, 30), (2, 24, 19, 15), (2, 40, 10, 8))]


def test_deterministic_mode_runs_are_bit_identical():
    base = dfpn_cases.build(features.DepthwiseFeaturePyramid, 'stub6').cuda().train()
    src = _stub6_taps(3)
    gs = None
    runs = []
    with ops.deterministic():
        for _ in range(2):
            m = copy.deepcopy(base)
            xs = [torch.from_numpy(s).cuda().requires_grad_(True) for s in src]
            outs, _ = m.neck(xs)
            if gs is None:
                rng = np.random.default_rng(4)
                gs = [torch.from_numpy(rng.standard_normal(tuple(o.shape), dtype=np.float32)).cuda() for o in outs]
            torch.autograd.backward(outs, gs)
            runs.append([o.detach().clone() for o in outs] + [x.grad for x in xs] + [p.grad for _, p in _neck_params(m)]
                        + [b for _, b in sorted(m.named_buffers())])
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i


# ---- 5. no stock kernel on the libssdk path ----------------------------------------------------------------------------------------

FWD_BANNED = ('aten.cat', 'aten.constant_pad_nd', 'aten.max_pool2d', 'aten.upsample_nearest2d', 'aten.convolution', 'aten._convolution',
              'aten.cudnn_convolution', 'aten.miopen_convolution', 'aten.miopen_depthwise_convolution', 'aten.native_batch_norm',
              'aten._native_batch_norm', 'aten.miopen_batch_norm', 'aten.batch_norm', 'aten.add.Tensor', 'aten.add_.Tensor')
BWD_BANNED = ('aten.max_pool2d_with_indices_backward', 'aten.upsample_nearest2d_backward', 'aten.convolution_backward',
              'aten.native_batch_norm_backward', 'aten.miopen_batch_norm_backward')


def _recorder():
    from torch.utils._python_dispatch import TorchDispatchMode

    class _Rec(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))
    return _Rec()


def test_no_stock_kernel_in_forward_or_backward():
    m = dfpn_cases.build(features.DepthwiseFeaturePyramid, 'stub6').cuda().train()
    xs = [torch.from_numpy(s).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for s in _stub6_taps(5)]
    rec = _recorder()
    with rec:
        outs, _ = m.neck(xs)
    bad = [n for n in rec.names if n.startswith(FWD_BANNED)]
    assert not bad, bad
    assert rec.names, 'the recorder saw nothing'
    gs = [torch.ones_like(o) for o in outs]
    rec = _recorder()
    with rec:
        torch.autograd.backward(outs, gs)
    bad = [n for n in rec.names if n.startswith(BWD_BANNED)]
    assert not bad, bad
    assert all(x.grad is not None for x in xs)


# ---- 6. variants on the stock modules ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kw', [dict(activation={'name': 'ReLU6', 'args': {'inplace': True}}), dict(interpolation_mode='bilinear'),
                                dict(pyramid_channels=12)])
def test_stock_variants_warn_once_and_match_torch(kw, caplog):
    args = dict(out_layers=(1, 3, 4), pyramid_layers=5, pyramid_channels=16)
    args.update(kw)
    rng = np.random.default_rng(23)
    torch.manual_seed(0)
    m = features.DepthwiseFeaturePyramid(_StubBase(), **args)
    _randomize(m, rng)
    ref = copy.deepcopy(m).train()
    m = m.cuda().train()
    conv._warned.discard(('DepthwiseFeaturePyramid', m._stock_reason))
    x = rng.standard_normal((2, 3, 64, 48), dtype=np.float32)
    with caplog.at_level(logging.WARNING):
        for _ in range(2):
            outs_g, _ = m(torch.from_numpy(x).cuda())
    assert sum('DepthwiseFeaturePyramid' in r.getMessage() for r in caplog.records) == 1
    xg = torch.from_numpy(x).cuda().requires_grad_(True)
    xr = torch.from_numpy(x).requires_grad_(True)
    outs_g, _ = m(xg)
    outs_r = _ref_neck(ref, [s for i, s in enumerate(_taps(ref.base, xr)) if i in args['out_layers']])
    for i, (a, b) in enumerate(zip(outs_g, outs_r)):
        _close(a.detach().cpu().numpy(), b.detach().numpy(), err_msg=f'y{i}')
    gs = [torch.from_numpy(rng.standard_normal(tuple(o.shape), dtype=np.float32)) for o in outs_r]
    torch.autograd.backward(outs_r, gs)
    torch.autograd.backward(outs_g, [g.cuda() for g in gs])
    _close(xg.grad.cpu().numpy(), xr.grad.numpy(), err_msg='dx')


# ---- 7. end to end through detection.init ------------------------------------------------------------------------------------------

MB2_DFPN = {
    'base': {'name': 'torchvision_mobilenet_v2', 'pretrained': False},
    'detector': {'num_classes': 21, 'use_depthwise': True,
                 'features': {'name': 'DepthwiseFeaturePyramid', 'out_layers': (13, 18), 'pyramid_layers': 6, 'pyramid_channels': 128}},
    'anchor_generator': {'type': 'ssd', 'num_scales': 6, 'min_scale': 0.1, 'max_scale': 1.05,
                         'aspect_ratios': [[1.0, 2.0]] + [[1.0, 2.0, 3.0]] * 3 + [[1.0, 2.0]] * 2},
}


def test_dfpn_ssd_mb2_step_fn_train_and_eval():
    """A config naming DepthwiseFeaturePyramid trains and evaluates through detection.init: levels 19, 10, 5, 3, 2, 1, A = 2 268."""
    import oracle
    from single_shot_detection_amd import synthetic as syn
    from single_shot_detection_amd.detection import init as det_init
    torch.manual_seed(9)
    dev = torch.device('cuda:0')
    wrapper, init_state, step_fn = det_init.init(
        dev, MB2_DFPN, {'xy_scale': 10.0, 'wh_scale': 5.0},
        {'score_threshold': .01, 'max_total': 200, 'nms': {'max_per_class': 100, 'overlap_threshold': .45}, 'score_converter': 'SOFTMAX'},
        {'classification_loss': {'name': 'CrossEntropyLoss'}, 'localization_loss': {'name': 'SmoothL1Loss'},
         'classification_weight': 1.0, 'localization_weight': 1.0},
        {'name': 'hard_negative_mining', 'negative_per_positive_ratio': 3, 'min_negative_per_image': 5},
        {'matched_threshold': 0.5, 'unmatched_threshold': 0.5})
    detector = wrapper.model
    assert isinstance(detector.predictor.features, features.DepthwiseFeaturePyramid)
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


# ---- 8. synchronised BatchNorm over two ranks --------------------------------------------------------------------------------------

def _sync_dfpn(state):
    torch.manual_seed(0)
    m = features.DepthwiseFeaturePyramid(_Taps(16, 24, 25, 2), (0, 1), pyramid_layers=4, pyramid_channels=16)
    m.load_state_dict(state)
    return m


def _dfpn_sync_rank(rank, world, port, out_dir):
    import torch.distributed as dist
    from single_shot_detection_amd.distributed import convert_sync_batchnorm
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    d = np.load(os.path.join(out_dir, 'in.npz'))
    m = _sync_dfpn({k: torch.from_numpy(v) for k, v in np.load(os.path.join(out_dir, 'state.npz')).items()})
    m = convert_sync_batchnorm(m).cuda().train()
    half = slice(rank * 2, rank * 2 + 2)
    xs = [torch.from_numpy(d[f'x{i}'][half]).cuda().requires_grad_(True) for i in range(2)]
    outs, _ = m.neck(xs)
    torch.autograd.backward(outs, [torch.from_numpy(d[f'g{i}'][half]).cuda() for i in range(len(outs))])
    out = {f'y{i}': y.detach().cpu().numpy() for i, y in enumerate(outs)}
    out.update({f'dx{i}': x.grad.cpu().numpy() for i, x in enumerate(xs)})
    out.update({'p_' + n: p.grad.cpu().numpy() for n, p in _neck_params(m)})
    out.update({'b_' + n: b.cpu().numpy() for n, b in m.named_buffers()})
    np.savez(os.path.join(out_dir, f'out{rank}.npz'), **out)
    dist.destroy_process_group()


def test_sync_batchnorm_two_ranks_equal_one_process_on_the_whole_batch(tmp_path):
    """Two ranks on this one GPU (gloo), half the batch each, every DFPN norm synchronised == one process on the whole batch with torch's
    own modules on the CPU: outputs, tap gradients and running statistics; parameter gradients sum over the ranks."""
    import socket
    import torch.multiprocessing as mp
    rng = np.random.default_rng(41)
    torch.manual_seed(0)
    m = features.DepthwiseFeaturePyramid(_Taps(16, 24, 25, 2), (0, 1), pyramid_layers=4, pyramid_channels=16)
    _randomize(m, rng)
    np.savez(tmp_path / 'state.npz', **{k: v.numpy() for k, v in m.state_dict().items()})
    data = {'x0': rng.standard_normal((4, 16, 12, 10), dtype=np.float32), 'x1': rng.standard_normal((4, 24, 6, 5), dtype=np.float32)}
    for i, (h, w) in enumerate(((12, 10), (6, 5), (3, 3), (2, 2))):
        data[f'g{i}'] = rng.standard_normal((4, 16, h, w), dtype=np.float32)
    np.savez(tmp_path / 'in.npz', **data)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dfpn_sync_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    ref = m.train()
    xs = [torch.from_numpy(data[f'x{i}']).requires_grad_(True) for i in range(2)]
    outs = _ref_neck(ref, xs)
    torch.autograd.backward(outs, [torch.from_numpy(data[f'g{i}']) for i in range(len(outs))])
    res = [np.load(tmp_path / f'out{r}.npz') for r in range(2)]
    for i, y in enumerate(outs):
        _close(np.concatenate([res[0][f'y{i}'], res[1][f'y{i}']], 0), y.detach().numpy(), err_msg=f'y{i}')
    for i, x in enumerate(xs):
        _close(np.concatenate([res[0][f'dx{i}'], res[1][f'dx{i}']], 0), x.grad.numpy(), err_msg=f'dx{i}')
    for n, p in _neck_params(ref):
        _close(res[0]['p_' + n] + res[1]['p_' + n], p.grad.numpy(), err_msg=n)
    for n, b in ref.named_buffers():
        for r in range(2):
            np.testing.assert_allclose(res[r]['b_' + n], b.numpy(), rtol=1e-4, atol=1e-5, err_msg=n)


# ---- 9. HIP-graph capture ----------------------------------------------------------------------------------------------------------

def test_graphed_forward_backward_equals_eager():
    from single_shot_detection_amd.graphs import GraphedCallable
    m = dfpn_cases.build(features.DepthwiseFeaturePyramid, 'stub6').cuda().train()
    params = [p for _, p in _neck_params(m)]
    rng = np.random.default_rng(8)
    shapes = [(2, 32, h, w) for h, w in ((38, 30), (19, 15), (10, 8), (5, 4), (3, 2), (2, 1))]
    gs = [torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda() for s in shapes]

    def step(*srcs):
        xs = [s.detach().requires_grad_(True) for s in srcs]
        outs, _ = m.neck(xs)
        grads = torch.autograd.grad(outs, xs + params, gs)
        return [o.detach() for o in outs] + list(grads)

    first = [torch.from_numpy(s).cuda().contiguous(memory_format=torch.channels_last) for s in _stub6_taps(11)]
    graphed = GraphedCallable(step, first)
    assert graphed.scratch_allocated_in_capture == 0
    for seed in (12, 13):
        srcs = [torch.from_numpy(s).cuda().contiguous(memory_format=torch.channels_last) for s in _stub6_taps(seed)]
        got = [t.clone() for t in graphed(*srcs)]
        want = step(*srcs)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            _close(a.cpu().numpy(), b.cpu().numpy(), err_msg=str(i))
