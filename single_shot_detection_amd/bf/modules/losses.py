"""Loss modules -- mirror of bf/modules/losses.py for the classes the hot path can select by name.

Inside MultiboxLoss the arithmetic is fused into ssdk_multibox_loss_fwd / _bwd (csrc/loss.hip) and these classes only carry the
constructor surface (so that ``get_ctor``/``filter_kwargs`` behave exactly like the reference's, including the dropped ``reduction``
keyword for classes whose ``__init__`` takes ``**kwargs`` -- SURVEY.md §8a L1) and the attributes MultiboxLoss inspects
(``MULTICLASS``, ``SOFT_TARGET``, ``IOU_LOSS``, ``reduction``).

On their own (``forward(prediction, target)``, losses.py:42-114) they run the SAME kernels on the [rows, classes] slice they are given:
the rows become the anchors of a one-image batch in which every row is sampled, the target rows -- which MultiboxLoss builds with at most
one non-zero entry, multibox_loss.py:62-74 -- go back to the (class, score) columns the kernel reads, and ``reduce_mean = 2`` asks for
the plain sums instead of MultiboxLoss's division by the positives.  Limits, each refused loudly: CUDA tensors, ``reduction`` 'sum' or
'mean' ('none' has no per-row output in the fused kernel), dense targets with at most one non-zero entry per row, SoftmaxFocalLoss's
``ignore_index`` mapped onto the kernel's -1.  GeneralizedIoULoss (losses.py:109-114) is 1 - box_utils.generalized_iou on
csrc/boxes.hip, forward only (no autograd: MultiboxLoss's GIoU term has its backward inside the fused kernel).

IoULoss, DistanceIoULoss, CompleteIoULoss and EfficientIoULoss are not in the reference either: MultiboxLoss fuses them like
GeneralizedIoULoss, and on their own they run box_utils.iou_loss (csrc/boxes.hip), which has a backward and 'none' (DESIGN.md §29).

QualityFocalLoss and VarifocalLoss are not in the reference: the IoU-aware sigmoid losses that train on every anchor (sampler
``valid_sampler``), on the dense kernels of csrc/loss.hip; same surface, same limits.

torch's own loss classes are re-exported as the reference does (``from torch.nn.modules.loss import *``).  MultiboxLoss puts these of them
on the fused kernels: CrossEntropyLoss (``label_smoothing``, ``weight``), SmoothL1Loss (``beta``, 0 included), L1Loss, MSELoss and
HuberLoss (``delta``); any other it refuses with NotImplementedError.
"""
import ctypes

import torch
import torch.nn as nn
from torch.nn.modules.loss import *  # noqa: F401,F403  (losses.py:4 re-exports torch's: a config may name any of them)

SSDK_CLS_SIGMOID_FOCAL = 1
SSDK_CLS_SOFTMAX_FOCAL = 2
SSDK_CLS_CE_SOFT = 3
SSDK_CLS_BCE_SOFT = 4
SSDK_CLS_QUALITY_FOCAL = 5
SSDK_CLS_VARIFOCAL = 6


class _SliceLossFn(torch.autograd.Function):
    """class-loss sum of ssdk_multibox_loss_fwd over a [rows, classes] slice (every row sampled, no box term)."""

    @staticmethod
    def forward(ctx, prediction, cls_col, score_col, kind, gamma, alpha, epsilon):
        from ... import _lib
        from ...detection import sampler as _sampler
        lib = _lib.lib()
        P, C = prediction.shape
        dev = prediction.device
        scores = prediction.float().contiguous()
        target = torch.zeros((1, P, 6), dtype=torch.float32, device=dev)
        target[0, :, 4] = cls_col
        target[0, :, 5] = score_col
        locs = torch.zeros((1, P * 4), dtype=torch.float32, device=dev)
        anchors = torch.ones((P, 4), dtype=torch.float32, device=dev)   # (box term: weight 0, and finite: log(0 / 1 + eps) with eps = 1)
        # (the IoU-aware kinds: no mask -- every row's class is >= 0 here, and NULL means "every row that is not ignored")
        sampled = None if kind in (SSDK_CLS_QUALITY_FOCAL, SSDK_CLS_VARIFOCAL) else torch.ones((1, P), dtype=torch.uint8, device=dev)
        ws = _sampler.loss_workspace(1, P, C, dev)
        params = _lib.LossParams(kind, 0, float(gamma), float(alpha), 2, float(epsilon), 1.0, 0.0, 10.0, 5.0, 1.0, 1.0)
        out3 = torch.empty((3,), dtype=torch.float32, device=dev)
        _lib.check(lib.ssdk_multibox_loss_fwd(ctypes.byref(params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target),
                                              _lib.ptr(sampled), 1, P, C, 0, _lib.ptr(out3), _lib.ptr(ws), ws.numel(), _lib.current_stream()),
                   'ssdk_multibox_loss_fwd')
        ctx.save_for_backward(scores, locs, anchors, target, sampled, ws)
        ctx.params = params
        ctx.dtype = prediction.dtype
        return out3[1]

    @staticmethod
    def backward(ctx, grad):
        from ... import _lib
        scores, locs, anchors, target, sampled, ws = ctx.saved_tensors
        P, C = scores.shape
        grad_out = grad.float().reshape(1).expand(2).contiguous()
        dscores = torch.empty_like(scores)
        dlocs = torch.empty_like(locs)
        _lib.check(_lib.lib().ssdk_multibox_loss_bwd_ex(ctypes.byref(ctx.params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors),
                                                        _lib.ptr(target), _lib.ptr(sampled), _lib.ptr(grad_out), 0, 1, P, C, _lib.ptr(dscores),
                                                        _lib.ptr(dlocs), None, _lib.ptr(ws), ws.numel(), _lib.current_stream()),
                   'ssdk_multibox_loss_bwd')
        return dscores.to(ctx.dtype), None, None, None, None, None, None


class _Loss(nn.Module):
    def __init__(self, reduction='mean', epsilon=0.0):  # losses.py:8-17
        super(_Loss, self).__init__()
        if reduction not in ['mean', 'sum', 'none']:
            raise ValueError(f'Wrong value for reduction: {reduction}')
        assert 0.0 <= epsilon < 1
        self.reduction = reduction
        self.epsilon = epsilon

    def _check(self, prediction):
        if not prediction.is_cuda:
            raise RuntimeError(f'{type(self).__name__}.forward runs on libssdk: CUDA tensors only')
        if self.reduction == 'none':
            raise NotImplementedError(f"{type(self).__name__}: reduction='none' (the fused kernel has no per-row output)")
        if prediction.dim() != 2:
            raise ValueError(f'{type(self).__name__}: prediction must be [rows, classes]')

    @staticmethod
    def _one_entry_rows(target, what):
        """(column of the non-zero entry or -1, its value) of every row of a dense [rows, classes] target; rows with more than one
        non-zero entry are not what multibox_loss.py:62-74 builds and not what the kernel reads."""
        nz = target != 0
        if bool((nz.sum(-1) > 1).any()):
            raise NotImplementedError(f'{what}: a target row with more than one non-zero entry')
        col = torch.where(nz.any(-1), nz.float().argmax(-1), torch.full((target.shape[0],), -1, device=target.device, dtype=torch.long))
        val = target.float().sum(-1)
        return col, val


class SigmoidFocalLoss(_Loss):
    MULTICLASS = True

    def __init__(self, gamma=2.0, alpha=0.25, **kwargs):  # losses.py:37-40
        super(SigmoidFocalLoss, self).__init__(**kwargs)
        self.gamma = gamma
        self.alpha = alpha

    def forward(self, prediction, target):  # losses.py:42-54; target [rows, classes], column j = class j + 1 (multibox_loss.py:64-67)
        self._check(prediction)
        col, val = self._one_entry_rows(target, 'SigmoidFocalLoss')
        total = _SliceLossFn.apply(prediction, (col + 1).float(), val, SSDK_CLS_SIGMOID_FOCAL, self.gamma, self.alpha, 0.0)
        return total / prediction.shape[0] if self.reduction == 'mean' else total   # (:52 sums a row's classes, _reduce means over the rows)


class _QualityLoss(_Loss):
    """The IoU-aware sigmoid losses (not in the reference; csrc/loss.hip's dense kernels).  Inside MultiboxLoss a positive's class column
    is asked for y = mixup weight * q, q = the IoU of the anchor's own decoded box with its ground-truth box (``use_iou``; q = 1 without),
    every other column and every negative row for 0, and q is a constant of the step.  On their own, ``forward(prediction, target)`` takes
    the dense target -- at most one non-zero entry per row, whose value is y."""
    MULTICLASS = True
    KIND = None

    def _slice(self, prediction, target, gamma, alpha):
        self._check(prediction)
        col, val = self._one_entry_rows(target, type(self).__name__)
        total = _SliceLossFn.apply(prediction, (col + 1).float(), val, self.KIND, gamma, alpha, 0.0)
        return total / prediction.shape[0] if self.reduction == 'mean' else total   # (like SigmoidFocalLoss: the mean is over the rows)


class QualityFocalLoss(_QualityLoss):
    """Quality Focal Loss (arXiv:2006.04388): |y - s|^beta * bce(x, y), s = sigmoid(x)."""
    KIND = SSDK_CLS_QUALITY_FOCAL

    def __init__(self, beta=2.0, use_iou=True, reduction='mean'):   # (reduction by name, no **kwargs: MultiboxLoss's 'sum' survives filter_kwargs)
        super(QualityFocalLoss, self).__init__(reduction=reduction)
        if not beta >= 1.0:
            raise ValueError(f'QualityFocalLoss: beta={beta} must be >= 1')
        self.beta = beta
        self.use_iou = bool(use_iou)

    def forward(self, prediction, target):
        return self._slice(prediction, target, self.beta, 0.0)


class VarifocalLoss(_QualityLoss):
    """Varifocal Loss (arXiv:2008.13367): y * bce(x, y) where y > 0, alpha * s^gamma * bce(x, 0) where y == 0."""
    KIND = SSDK_CLS_VARIFOCAL

    def __init__(self, alpha=0.75, gamma=2.0, use_iou=True, reduction='mean'):
        super(VarifocalLoss, self).__init__(reduction=reduction)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f'VarifocalLoss: alpha={alpha} outside [0, 1]')
        if not gamma >= 0.0:
            raise ValueError(f'VarifocalLoss: gamma={gamma} must be >= 0')
        self.alpha = alpha
        self.gamma = gamma
        self.use_iou = bool(use_iou)

    def forward(self, prediction, target):
        return self._slice(prediction, target, self.gamma, self.alpha)


class SoftmaxFocalLoss(_Loss):
    def __init__(self, gamma=0.0, alpha=None, ignore_index=-100, **kwargs):  # losses.py:57-61
        super(SoftmaxFocalLoss, self).__init__(**kwargs)
        self.gamma = gamma
        self.alpha = alpha
        self.ignore_index = ignore_index

    def forward(self, input_, target):  # losses.py:63-78; target [rows] class ids
        self._check(input_)
        cls = torch.where(target == self.ignore_index, torch.full_like(target, -1), target).float()
        total = _SliceLossFn.apply(input_, cls, torch.zeros_like(cls), SSDK_CLS_SOFTMAX_FOCAL, self.gamma,
                                   -1.0 if self.alpha is None else self.alpha, 0.0)
        return total / target.numel() if self.reduction == 'mean' else total   # (:65 the ignored rows stay in the mean, as zeros)


class CrossEntropyWithSoftTargetsLoss(_Loss):  # losses.py:80-93
    SOFT_TARGET = True

    def forward(self, logits, target):  # target [rows, classes], column j = class j (multibox_loss.py:68-71); an all-zero row = ignored
        self._check(logits)
        col, val = self._one_entry_rows(target, 'CrossEntropyWithSoftTargetsLoss')
        total = _SliceLossFn.apply(logits, col.float(), val, SSDK_CLS_CE_SOFT, 0.0, 0.0, self.epsilon)
        return total / logits.shape[0] if self.reduction == 'mean' else total


class BinaryCrossEntropyWithSoftTargetsLoss(_Loss):  # losses.py:95-106
    SOFT_TARGET = True
    MULTICLASS = True

    def forward(self, logits, target):  # target [rows, classes], column j = class j + 1 (multibox_loss.py:64-67)
        self._check(logits)
        col, val = self._one_entry_rows(target, 'BinaryCrossEntropyWithSoftTargetsLoss')
        total = _SliceLossFn.apply(logits, (col + 1).float(), val, SSDK_CLS_BCE_SOFT, 0.0, 0.0, self.epsilon)
        return total / logits.numel() if self.reduction == 'mean' else total   # (:106 F.binary_cross_entropy_with_logits means over the elements)


class GeneralizedIoULoss(_Loss):  # losses.py:109-114
    IOU_LOSS = True

    def forward(self, boxes, target):
        from ..utils import box_utils
        if self.reduction == 'none':
            raise NotImplementedError("GeneralizedIoULoss: reduction='none'")
        if boxes.requires_grad:
            raise NotImplementedError('GeneralizedIoULoss.forward on its own has no backward; inside MultiboxLoss it is fused (csrc/loss.hip)')
        loss = 1.0 - box_utils.generalized_iou(boxes, target, cartesian=False)
        return loss.mean() if self.reduction == 'mean' else loss.sum()


class _IoUFamilyLoss(_Loss):
    """The IoU-based box losses that are not in the reference.  Inside MultiboxLoss the term is fused into csrc/loss.hip (decoded corners
    against the raw target, like GeneralizedIoULoss); on their own, ``forward(boxes, target)`` takes [Boxes, 4] corner boxes and runs
    ``box_utils.iou_loss`` -- the same per-box arithmetic (csrc/iou_loss.h), with a backward towards ``boxes`` and all three reductions."""
    IOU_LOSS = True
    KIND = None

    def __init__(self, reduction='mean'):   # (reduction by name, no **kwargs: MultiboxLoss's 'sum' survives filter_kwargs)
        super(_IoUFamilyLoss, self).__init__(reduction=reduction)

    def forward(self, boxes, target):
        from ..utils import box_utils
        loss = box_utils.iou_loss(boxes, target, self.KIND)
        if self.reduction == 'none':
            return loss
        return loss.mean() if self.reduction == 'mean' else loss.sum()


class IoULoss(_IoUFamilyLoss):
    """1 - IoU."""
    KIND = 'iou'


class DistanceIoULoss(_IoUFamilyLoss):
    """Distance-IoU loss (arXiv:1911.08287): 1 - IoU + rho^2 / c^2."""
    KIND = 'diou'


class CompleteIoULoss(_IoUFamilyLoss):
    """Complete-IoU loss (arXiv:1911.08287): DIoU + alpha v; alpha is a constant of the step."""
    KIND = 'ciou'


class EfficientIoULoss(_IoUFamilyLoss):
    """Efficient-IoU loss (arXiv:2101.08158, without the focal factor): DIoU + the width and height terms over the enclosing box's."""
    KIND = 'eiou'


class DistributionFocalLoss(_Loss):
    """Distribution Focal Loss (arXiv:2006.04388; not in the reference) on its own: ``prediction`` [rows, reg_max + 1] logits of one
    discrete distribution per row, ``target`` [rows] positions in bin units; a row's value is the cross-entropy against the two bins that
    bracket its target, weighted by their distance to it.  Stock torch ops on any device: the name a config looks up and the yardstick
    of tools/bench_dfl.py.  Inside MultiboxLoss the term is fused into the integral box head's kernels (csrc/integral.hip), which this
    class only selects."""

    def __init__(self, reduction='mean', reg_max=16, **kwargs):   # (reduction by name: MultiboxLoss's 'sum' survives filter_kwargs)
        super(DistributionFocalLoss, self).__init__(reduction=reduction, **kwargs)
        if not 1 <= int(reg_max) <= 63:
            raise ValueError(f'DistributionFocalLoss: reg_max={reg_max} outside [1, 63]')
        self.reg_max = int(reg_max)

    def forward(self, prediction, target):
        import torch.nn.functional as F
        if prediction.dim() != 2 or prediction.shape[1] != self.reg_max + 1:
            raise ValueError(f'DistributionFocalLoss: prediction must be [rows, {self.reg_max + 1}]')
        y = target.to(prediction.dtype).clamp(0, self.reg_max)
        yl = y.floor().clamp(max=self.reg_max - 1)
        left = yl.long()
        loss = (F.cross_entropy(prediction, left, reduction='none') * (yl + 1 - y) +
                F.cross_entropy(prediction, left + 1, reduction='none') * (y - yl))
        if self.reduction == 'none':
            return loss
        return loss.mean() if self.reduction == 'mean' else loss.sum()
