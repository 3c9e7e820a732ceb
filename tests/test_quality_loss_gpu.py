"""GPU: QualityFocalLoss / VarifocalLoss and valid_sampler on the dense all-anchor kernels (csrc/loss.hip: loss_dense_fwd_kernel /
loss_dense_bwd_kernel) against the fp64 torch-CPU restatement of tests/quality_loss_cases.py: values and both gradients, with the project's
tolerances for this family (tests/test_loss_torch_kinds_gpu.py, tests/test_loss_gpu.py)."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import quality_loss_cases as qc
from single_shot_detection_amd import _lib
from single_shot_detection_amd.bf.modules import losses
from single_shot_detection_amd.detection import sampler
from single_shot_detection_amd.detection.box_coder import BoxCoder
from single_shot_detection_amd.detection.losses.multibox_loss import MultiboxLoss

pytestmark = pytest.mark.gpu

HNM = functools.partial(sampler.hard_negative_mining, negative_per_positive_ratio=3, min_negative_per_image=5)
CLS = {'qfl': 'QualityFocalLoss', 'vfl': 'VarifocalLoss', 'focal': 'SigmoidFocalLoss'}
LOC = {'giou': 'GeneralizedIoULoss', 'smooth_l1': 'SmoothL1Loss'}
VALUES = dict(rtol=1e-5, atol=1e-4)
DSCORES = dict(rtol=3e-4, atol=3e-7)
DLOCS = {'smooth_l1': dict(rtol=1e-5, atol=1e-8), 'giou': dict(rtol=3e-4, atol=3e-7)}


def not_ignored(predictions, target_classes):
    """A custom callable with valid_sampler's rule: MultiboxLoss does not recognise it, so its mask goes to the kernels."""
    return target_classes != -1


SAMPLERS = {'valid': sampler.valid_sampler, 'valid_partial': functools.partial(sampler.valid_sampler), 'hnm': HNM,
            'naive': sampler.naive_sampler, 'custom': not_ignored}


def run(case, kind, loc, smp, **cl_kw):
    """One forward + backward of MultiboxLoss on the GPU: values [3], dscores, dlocs, the target as the loss left it, the sampled mask."""
    crit = MultiboxLoss(sampler=SAMPLERS[smp], box_coder=BoxCoder(qc.XY_SCALE, qc.WH_SCALE), classification_loss={'name': CLS[kind], **cl_kw},
                        localization_loss={'name': LOC[loc]})
    s, l, anchors, target = qc.fresh(case)
    loss, class_loss, loc_loss = crit((s, l), anchors, target)
    (2.0 * class_loss + 0.5 * loc_loss).backward()       # non-unit upstream gradients
    return dict(values=np.array([loss.item(), class_loss.item(), loc_loss.item()]), dscores=s.grad.cpu().numpy(), dlocs=l.grad.cpu().numpy(),
                target=target.cpu(), mask=crit.last_sampled_mask.cpu().bool(), out3=torch.stack([loss, class_loss, loc_loss]).detach().cpu(),
                ds_t=s.grad.cpu(), dl_t=l.grad.cpu())


def reference(case, got, kind, loc, smp, **kw):
    """The fp64 restatement for a GPU run: on the run's own mask (None for valid_sampler: the rule itself), and for SmoothL1 against the
    target as the kernel encoded it (as tests/test_loss_torch_kinds_gpu.py does), which is compared with the fp64 encode on its own."""
    mask = None if smp.startswith('valid') else got['mask']
    encoded = got['target'] if loc == 'smooth_l1' else None
    reduction = 'mean' if kind == 'focal' else 'sum'     # (SigmoidFocalLoss takes **kwargs: filter_kwargs drops MultiboxLoss's 'sum')
    return qc.reference_run(case, mask, kind, loc=loc, encoded=encoded, reduction=reduction, **kw)


def compare(got, ref, loc, what='', kink=None):
    """kink: rows [B, A] whose GIoU gradient is one-sided (tests/quality_loss_cases.py: the positive exactly on its box): under the GIoU
    term their dlocs are only required to be finite."""
    vals, ds, dl = ref
    if loc == 'giou' and kink is not None and kink.any():
        k = kink.numpy().repeat(4, axis=1)
        assert np.isfinite(got['dlocs'][k]).all()
        got = dict(got, dlocs=np.where(k, 0.0, got['dlocs']))
        dl = np.where(k, 0.0, dl)
    print(what, 'values', got['values'], vals, 'max |ddscores|', np.abs(got['dscores'] - ds).max(), 'max |ddlocs|', np.abs(got['dlocs'] - dl).max())
    np.testing.assert_allclose(got['values'], vals, **VALUES)
    np.testing.assert_allclose(got['dscores'], ds, **DSCORES)
    np.testing.assert_allclose(got['dlocs'], dl, **DLOCS[loc])


def check(name, kind, loc, smp, **kw):
    case = qc.case(name)
    got = run(case, kind, loc, smp, **kw)
    if smp.startswith('valid') or smp == 'custom':
        assert torch.equal(got['mask'], case['target'][..., 4] != -1)
    compare(got, reference(case, got, kind, loc, smp, **kw), loc, f'{name} {kind} {loc} {smp}', case['giou_kink'])
    if loc == 'smooth_l1':    # the in-place encode of multibox_loss.py:81-82 happened, and q was taken before it
        enc = qc.encode_target(case['target'].double(), case['anchors'].double())
        np.testing.assert_allclose(got['target'].numpy(), enc.numpy(), rtol=1e-6, atol=2e-5)
        assert torch.equal(got['target'][..., 4:], case['target'][..., 4:])
    else:
        assert torch.equal(got['target'], case['target'])
    return got


@pytest.mark.parametrize('loc', ['giou', 'smooth_l1'])
@pytest.mark.parametrize('kind', ['qfl', 'vfl'])
def test_valid_sampler_b3_c20(kind, loc):
    """B = 3, C = 20, an ignore band, one image without boxes, one box of mixup weight 0.6; positives off their box (q = 0), one on it."""
    case = qc.case('b3_c20')
    cls = case['target'][..., 4]
    assert (cls == -1).any() and (cls[1] <= 0).all() and (case['target'][..., 5][cls > 0] == 0.6).any()
    check('b3_c20', kind, loc, 'valid')


@pytest.mark.parametrize('name', ['b3_c3', 'b3_c1', 'b1_c81_a257', 'b2_c81_a257', 'b1_c3_a5', 'no_positive'])
@pytest.mark.parametrize('kind', ['qfl', 'vfl'])
def test_valid_sampler_shapes(kind, name):
    """C = 3 / C = 1 (a 16-byte vector straddles or covers rows), 257 anchors (a full tile plus one row; at B = 2 a tile crosses the image
    boundary), 5 anchors of 3 classes (less than one vector per thread, a scalar tail), and a batch without a positive (divider 1)."""
    case = qc.case(name)
    if name == 'no_positive':
        assert not case['positive'].any()
    check(name, kind, 'giou', 'valid_partial' if name == 'b3_c3' else 'valid')
    if name in ('b1_c81_a257', 'b1_c3_a5'):
        check(name, kind, 'smooth_l1', 'valid')


@pytest.mark.parametrize('smp', ['hnm', 'naive', 'custom'])
@pytest.mark.parametrize('kind', ['qfl', 'vfl'])
def test_through_a_mask(kind, smp):
    for name in ('b3_c20', 'b2_c81_a257', 'no_positive'):
        got = check(name, kind, 'giou', smp)
        if smp == 'custom':      # the same rows as the NULL path: the two agree within the tolerances
            null = run(qc.case(name), kind, 'giou', 'valid')
            compare(got, (null['values'], null['dscores'], null['dlocs']), 'giou', f'{name} custom vs NULL')
    check('b3_c20', kind, 'smooth_l1', smp)


@pytest.mark.parametrize('name', ['b3_c20', 'b3_c3', 'b2_c81_a257', 'no_positive'])
def test_sigmoid_focal_dense_path_against_the_existing_kernels(name):
    """SigmoidFocalLoss: valid_sampler (sampled = NULL, the dense kernels) and the same rule as a custom callable (a mask, the kernels it
    always had) agree within the tolerances, and both with the restatement."""
    dense = check(name, 'focal', 'giou', 'valid')
    masked = check(name, 'focal', 'giou', 'custom')
    compare(dense, (masked['values'], masked['dscores'], masked['dlocs']), 'giou', f'{name} focal dense vs masked')
    check(name, 'focal', 'smooth_l1', 'valid')


@pytest.mark.parametrize('kind', ['qfl', 'vfl'])
def test_use_iou_false_takes_the_given_target(kind):
    check('b3_c20', kind, 'giou', 'valid', use_iou=False)
    check('b3_c20', kind, 'smooth_l1', 'hnm', use_iou=False)


def test_other_exponents():
    check('b3_c20', 'qfl', 'giou', 'valid', beta=1.5)
    check('b3_c20', 'qfl', 'giou', 'valid', beta=1.0)
    check('b3_c20', 'vfl', 'giou', 'valid', alpha=0.5, gamma=1.5)


@pytest.mark.parametrize('kind,loc,smp', [('qfl', 'giou', 'valid'), ('vfl', 'smooth_l1', 'valid'), ('qfl', 'smooth_l1', 'hnm')])
def test_two_runs_give_identical_bits(kind, loc, smp):
    a, b = (run(qc.case('b3_c20'), kind, loc, smp) for _ in range(2))
    for k in ('out3', 'ds_t', 'dl_t', 'target'):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('reduction', ['sum', 'mean'])
@pytest.mark.parametrize('rows,C', [(1000, 20), (7, 3), (1000, 3), (7, 20)])
@pytest.mark.parametrize('kind', ['qfl', 'vfl'])
def test_standalone_modules(kind, rows, C, reduction):
    rng = np.random.default_rng(rows * 31 + C)
    x_np = (rng.standard_normal((rows, C)) * 2.0).astype(np.float32)
    y_np = np.zeros((rows, C), np.float32)
    hot = rng.random(rows) < 0.4
    y_np[np.nonzero(hot)[0], rng.integers(0, C, int(hot.sum()))] = rng.uniform(0.05, 1.0, int(hot.sum())).astype(np.float32)
    module = (losses.QualityFocalLoss(beta=2.0, reduction=reduction) if kind == 'qfl' else losses.VarifocalLoss(reduction=reduction))
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    out = module(x, torch.from_numpy(y_np).cuda())
    (3.0 * out).backward()
    xr = torch.from_numpy(x_np).double().requires_grad_(True)
    elem = (qc.quality_focal if kind == 'qfl' else qc.varifocal)(xr, torch.from_numpy(y_np).double())
    ref = elem.sum() / (rows if reduction == 'mean' else 1)
    (3.0 * ref).backward()
    np.testing.assert_allclose(out.item(), float(ref), **VALUES)
    np.testing.assert_allclose(x.grad.cpu().numpy(), xr.grad.numpy(), **DSCORES)
    with pytest.raises(NotImplementedError):
        type(module)(reduction='none')(x, torch.from_numpy(y_np).cuda())


def test_retina_500_atss_qfl_giou():
    """RetinaNet-500 geometry (47 961 anchors, 80 classes), B = 2, ATSS targets, the README's configuration."""
    case = qc.case('retina_b2_c80_atss')
    assert case['A'] == 47961 and not (case['target'][..., 4] == -1).any()
    check('retina_b2_c80_atss', 'qfl', 'giou', 'valid')


def test_c_abi_refusals():
    """By return code, before any launch: a NULL mask for a kind that has no dense path, quality_from_iou for an older kind, beta < 1,
    Varifocal's alpha and gamma out of range; and the accepted NULL."""
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
    ws = sampler.loss_workspace(B, A, C, dev)

    def params(cls_kind, gamma=2.0, alpha=0.25, quality=0):
        return _lib.LossParams(cls_kind, 1, gamma, alpha, 0, 0.0, 1.0, 1.0, 10.0, 5.0, 1e-8, 1.0, 0.0, None, quality)

    def both(p, mask):
        f = lib.ssdk_multibox_loss_fwd(ctypes.byref(p), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target), _lib.ptr(mask), B, A,
                                       C, 0, _lib.ptr(out3), _lib.ptr(ws), ws.numel(), _lib.current_stream())
        b = lib.ssdk_multibox_loss_bwd(ctypes.byref(p), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target), _lib.ptr(mask),
                                       _lib.ptr(grad), B, A, C, _lib.ptr(ds), _lib.ptr(dl), _lib.ptr(ws), ws.numel(), _lib.current_stream())
        return f, b

    for kind in (0, 2, 3, 4):
        assert both(params(kind), None) == (-1, -1), kind                      # NULL mask: SSDK_CLS_CROSS_ENTROPY and the other older kinds
    assert both(params(1, quality=1), sampled) == (-1, -1)                     # quality_from_iou with SSDK_CLS_SIGMOID_FOCAL
    assert both(params(0, quality=1), sampled) == (-1, -1)
    assert both(params(5, gamma=0.5), sampled) == (-1, -1)                     # beta = 0.5
    assert both(params(6, gamma=-1.0, alpha=0.75), sampled) == (-1, -1)
    assert both(params(6, alpha=1.5), sampled) == (-1, -1)
    assert both(params(7), sampled) == (-1, -1)
    for kind, alpha in ((1, 0.25), (5, 0.25), (6, 0.75)):
        assert both(params(kind, alpha=alpha, quality=int(kind != 1)), None) == (0, 0), kind
    assert lib.ssdk_valid_sampler(None, 6, B, A, _lib.ptr(sampled), _lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert torch.isfinite(out3).all() and (ds == 0).sum() == 0                 # (x = 0, y = 0: every element has a gradient)


def test_valid_sampler_function():
    case = qc.case('b3_c20')
    t = case['target'].cuda()
    got = sampler.valid_sampler(None, t[..., 4])
    assert got.dtype == torch.bool and torch.equal(got.cpu(), case['target'][..., 4] != -1)
    assert torch.equal(sampler.valid_sampler(None, t[..., 4].long()).cpu(), got.cpu())


def test_valid_sampler_with_a_softmax_kind_hands_over_its_mask():
    """CrossEntropyLoss has no dense path: under valid_sampler it gets the mask of ssdk_valid_sampler on the kernels it always had, bit for
    bit what the same rule gives as a custom callable."""
    case = qc.case('b3_c20')
    B, A, C = case['B'], case['A'], 21
    scores = torch.from_numpy(np.random.default_rng(3).standard_normal((B, A * C), dtype=np.float32))
    runs = []
    for smp in ('valid', 'custom'):
        crit = MultiboxLoss(sampler=SAMPLERS[smp], box_coder=BoxCoder(qc.XY_SCALE, qc.WH_SCALE), classification_loss={'name': 'CrossEntropyLoss'},
                            localization_loss={'name': 'SmoothL1Loss'})
        s = scores.clone().cuda().requires_grad_(True)
        _, l, anchors, target = qc.fresh(case)
        out = crit((s, l), anchors, target)
        out[0].backward()
        runs.append([o.detach() for o in out] + [s.grad, l.grad, crit.last_sampled_mask])
    assert torch.isfinite(runs[0][0]) and runs[0][5].bool().sum() == (case['target'][..., 4] != -1).sum()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_captured_graph_and_detection_init_in_a_child_process():
    """tests/quality_loss_graph_worker.py, in a process of its own (see there): forward and backward captured in a HIP graph and replayed on
    two batches equal the eager results bit for bit; a training step through detection.init with the README's configuration, eager and
    with graph_hot_path=True, gives the same loss, which is the restatement's on the assigner's target."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, 'tests', 'quality_loss_graph_worker.py')], cwd=repo, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert res['timeouts'] == 0
    assert res['eager_loss'] == res['graphed_loss'] and np.isfinite(res['eager_loss']), res
