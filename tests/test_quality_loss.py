"""CPU: the restatement of Quality Focal Loss / Varifocal Loss (tests/quality_loss_cases.py) against the hand values and closed forms of
include/ssdk.h, and the Python surface of the feature (constructors by name, MultiboxLoss's mapping, valid_sampler by name)."""
import functools
import math

import pytest
import torch

import quality_loss_cases as qc
from single_shot_detection_amd.bf.modules import losses
from single_shot_detection_amd.detection import sampler
from single_shot_detection_amd.detection.box_coder import BoxCoder
from single_shot_detection_amd.detection.losses import multibox_loss as mbl
from single_shot_detection_amd.utils import get_ctor


def _value_and_grad(fn, x, y):
    xt = torch.tensor([x], dtype=torch.float64, requires_grad=True)
    v = fn(xt, torch.tensor([y], dtype=torch.float64))
    v.sum().backward()
    return float(v.detach()), float(xt.grad)


@pytest.mark.parametrize('fn,y,value,grad', [
    (qc.quality_focal, 0.5, 0.0, 0.0),
    (qc.quality_focal, 1.0, 0.1732868, -0.2982868),
    (qc.varifocal, 0.5, 0.3465736, 0.0),
    (qc.varifocal, 0.0, 0.1299651, 0.2237151),
])
def test_hand_values_at_x_0(fn, y, value, grad):
    """x = 0: s = 1/2, bce(0, y) = ln 2.  QFL(beta 2): (y - 1/2)^2 ln 2, gradient 2 |y - 1/2| sgn(1/2 - y) ln 2 / 4 + (y - 1/2)^2 (1/2 - y);
    VFL(alpha 3/4, gamma 2): y ln 2 with gradient y (1/2 - y), or 3/16 ln 2 with gradient 3/16 (ln 2 + 1/2)."""
    v, g = _value_and_grad(fn, 0.0, y)
    assert abs(v - value) < 5e-8 and abs(g - grad) < 5e-8
    closed = {qc.quality_focal: qc.quality_focal_grad, qc.varifocal: qc.varifocal_grad}[fn]
    assert abs(float(closed(torch.zeros(1, dtype=torch.float64), torch.tensor([y], dtype=torch.float64))) - grad) < 5e-8


def test_hand_values_in_closed_form():
    ln2 = math.log(2.0)
    assert abs(0.25 * ln2 - 0.1732868) < 5e-8 and abs(-(0.25 * ln2 + 0.125) - -0.2982868) < 5e-8
    assert abs(0.5 * ln2 - 0.3465736) < 5e-8 and abs(0.1875 * ln2 - 0.1299651) < 5e-8 and abs(0.1875 * (ln2 + 0.5) - 0.2237151) < 5e-8


def test_plain_iou_of_two_unit_offset_squares():
    q = qc.plain_iou(torch.tensor([[0.0, 0.0, 2.0, 2.0]], dtype=torch.float64), torch.tensor([[1.0, 1.0, 3.0, 3.0]], dtype=torch.float64))
    assert abs(float(q) - 1.0 / 7.0) < 1e-15
    z = qc.plain_iou(torch.tensor([[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0]]), torch.tensor([[0.0, 0.0, 0.0, 0.0], [2.0, 2.0, 3.0, 3.0]]))
    assert z.tolist() == [0.0, 0.0]                          # an empty union (0 / 0), and disjoint boxes


@pytest.mark.parametrize('kind', ['qfl_beta2', 'qfl_beta1.5', 'qfl_beta1', 'vfl', 'vfl_gamma1.5'])
def test_autograd_equals_the_closed_forms(kind):
    rng = torch.Generator().manual_seed(7)
    x = (torch.randn(1000, generator=rng, dtype=torch.float64) * 4.0).requires_grad_(True)
    y = torch.rand(1000, generator=rng, dtype=torch.float64)
    if kind.startswith('vfl'):
        y = torch.where(torch.rand(1000, generator=rng) < 0.5, torch.zeros_like(y), y)    # both branches
        gamma = 1.5 if kind.endswith('1.5') else 2.0
        value, closed = qc.varifocal(x, y, 0.75, gamma), qc.varifocal_grad(x.detach(), y, 0.75, gamma)
    else:
        beta = float(kind[len('qfl_beta'):])
        value, closed = qc.quality_focal(x, y, beta), qc.quality_focal_grad(x.detach(), y, beta)
    value.sum().backward()
    torch.testing.assert_close(x.grad, closed, rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize('name,extra', [('QualityFocalLoss', {'beta': 1.5}), ('VarifocalLoss', {'alpha': 0.5, 'gamma': 1.0})])
def test_constructed_by_name_keeps_reduction_sum(name, extra):
    """multibox_loss.py:23-26's constructor dance: reduction='sum' survives filter_kwargs because the signature names it."""
    m = get_ctor(losses, name)(reduction='sum', ignore_index=-1, name=name, **extra)
    assert m.reduction == 'sum' and m.MULTICLASS and m.use_iou is True
    for k, v in extra.items():
        assert getattr(m, k) == v
    assert get_ctor(losses, name)(name=name).reduction == 'mean'
    assert get_ctor(losses, name)(name=name, use_iou=False).use_iou is False


def test_parameter_refusals():
    with pytest.raises(ValueError):
        losses.QualityFocalLoss(beta=0.5)
    with pytest.raises(ValueError):
        losses.VarifocalLoss(alpha=1.5)
    with pytest.raises(ValueError):
        losses.VarifocalLoss(alpha=-0.1)
    with pytest.raises(ValueError):
        losses.VarifocalLoss(gamma=-1.0)
    with pytest.raises(ValueError):
        losses.QualityFocalLoss(reduction='total')
    losses.QualityFocalLoss(beta=1.0)
    losses.VarifocalLoss(alpha=0.0, gamma=0.0)


@pytest.mark.parametrize('cl,kind,gamma,alpha,q', [
    ({'name': 'QualityFocalLoss'}, 5, 2.0, None, 1),
    ({'name': 'QualityFocalLoss', 'beta': 1.5, 'use_iou': False}, 5, 1.5, None, 0),
    ({'name': 'VarifocalLoss'}, 6, 2.0, 0.75, 1),
    ({'name': 'VarifocalLoss', 'alpha': 0.5, 'gamma': 1.0, 'use_iou': False}, 6, 1.0, 0.5, 0),
])
def test_multibox_loss_maps_the_kinds(cl, kind, gamma, alpha, q):
    crit = mbl.MultiboxLoss(sampler=sampler.valid_sampler, box_coder=BoxCoder(10.0, 5.0), classification_loss=cl,
                            localization_loss={'name': 'GeneralizedIoULoss'})
    p = crit.loss_params()
    assert (p.cls_kind, p.loc_kind, p.quality_from_iou, p.reduce_mean) == (kind, mbl.SSDK_LOC_GIOU, q, 0)
    assert p.focal_gamma == gamma and (alpha is None or p.focal_alpha == alpha)
    assert crit.multiclass
    # the older kinds leave the appended field 0
    ce = mbl.MultiboxLoss(sampler=sampler.naive_sampler, box_coder=BoxCoder(10.0, 5.0), classification_loss={'name': 'SigmoidFocalLoss'},
                          localization_loss={'name': 'SmoothL1Loss'})
    assert ce.loss_params().quality_from_iou == 0


def test_loss_params_binding_is_the_header_struct_with_the_appended_field():
    """ssdk_loss_params ends in quality_from_iou (ABI 125).  The binding keeps the older fields in LossParams._fields_ and the new one in a
    subclass that ctypes lays out behind them; LossParams(...) constructs that full struct, so the library reads the field inside it."""
    import ctypes
    import os
    import re
    from conftest import REPO
    from single_shot_detection_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'ssdk.h')).read(), flags=re.S)
    body = header[header.index('typedef struct ssdk_loss_params'):header.index('} ssdk_loss_params;')]
    declared = re.findall(r'(\w+)\s*[;,]', body)
    old = _lib.LossParams(0, 0, 2.0, 0.25, 0, 0.0, 1.0, 1.0, 10.0, 5.0, 1e-8, 1.0)     # positional, the twelve fields of ABI 123
    names = [f[0] for klass in type(old).__mro__[::-1] if '_fields_' in vars(klass) for f in klass._fields_]
    assert names == declared and names[-1] == 'quality_from_iou'
    assert old.quality_from_iou == 0 and old.class_weight is None
    # 13 four-byte fields, padding to 56, the pointer, the int at 64, the struct padded to the pointer's alignment
    assert type(old).quality_from_iou.offset == 64 and type(old).class_weight.offset == 56 and ctypes.sizeof(old) == 72
    new = _lib.LossParams(5, 1, 2.0, 0.25, 0, 0.0, 1.0, 1.0, 10.0, 5.0, 1e-8, 1.0, 0.0, None, 1)
    assert new.quality_from_iou == 1 and ctypes.sizeof(new) == 72 and isinstance(new, _lib.LossParams)


def test_valid_sampler_is_resolved_by_name():
    """detection/init.py:68-70: getattr on the sampler module, the config's keywords filtered by the function's own names, a partial."""
    sampler_args = {'name': 'valid_sampler', 'negative_per_positive_ratio': 3}
    fn = getattr(sampler, sampler_args['name'])
    kwargs = {k: v for k, v in sampler_args.items() if k in fn.__code__.co_varnames and not k.startswith('_')}
    assert kwargs == {}
    wrapped = functools.partial(fn, **kwargs)
    base, kw = mbl._unwrap_sampler(wrapped)
    assert base is sampler.valid_sampler and kw == {}
