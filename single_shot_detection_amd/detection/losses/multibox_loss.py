"""MultiboxLoss -- mirror of detection/losses/multibox_loss.py:10-94 on libssdk (csrc/loss.hip)."""
import ctypes
import functools

import torch
import torch.nn as nn

from ... import _lib
from ...bf.modules import losses
from ...utils import get_ctor
from .. import sampler as _sampler
from ..target_assigner import LOC_INDEX_START, LOC_INDEX_END, CLASS_INDEX, SCORE_INDEX, IGNORE_CLASS, NEGATIVE_CLASS  # noqa: F401

SSDK_CLS_CROSS_ENTROPY = 0
SSDK_CLS_SIGMOID_FOCAL = 1
SSDK_CLS_SOFTMAX_FOCAL = 2
SSDK_CLS_CE_SOFT = 3
SSDK_CLS_BCE_SOFT = 4
SSDK_CLS_QUALITY_FOCAL = 5
SSDK_CLS_VARIFOCAL = 6
# the sigmoid-target kinds: for these "every anchor that is not ignored" needs no mask (sampled = NULL: the dense kernels of csrc/loss.hip)
_NULL_MASK_KINDS = (SSDK_CLS_SIGMOID_FOCAL, SSDK_CLS_QUALITY_FOCAL, SSDK_CLS_VARIFOCAL)
SSDK_LOC_SMOOTH_L1 = 0
SSDK_LOC_GIOU = 1
SSDK_LOC_L1 = 2
SSDK_LOC_MSE = 3
SSDK_LOC_HUBER = 4
SSDK_LOC_IOU = 8
SSDK_LOC_DIOU = 9
SSDK_LOC_CIOU = 10
SSDK_LOC_EIOU = 11


_NO_ROW_HINT = bool(__import__('os').environ.get('SSDK_NO_ROW_HINT'))   # (measurement knob: the heads scan dscores as before round 4)


def _unwrap_sampler(fn):
    """(base function, kwargs) of a possibly functools.partial-wrapped sampler (detection/init.py:90-92)."""
    kwargs = {}
    while isinstance(fn, functools.partial):
        kwargs = {**fn.keywords, **kwargs}
        if fn.args:
            return fn, {}
        fn = fn.func
    return fn, kwargs


class _MultiboxLossFn(torch.autograd.Function):
    """(class_loss, loc_loss) = f(scores, locs); target is mutated in place like the reference does."""

    @staticmethod
    def forward(ctx, scores, locs, anchors, target, module):
        lib = _lib.lib()
        B, A = target.shape[:2]
        C = scores.numel() // (B * A)
        dev = scores.device
        ws = _sampler.loss_workspace(B, A, C, dev)
        cls_col = target[..., CLASS_INDEX]
        fn, kw = _unwrap_sampler(module.sampler)
        lse_valid = 0
        null_mask = False
        if fn is _sampler.hard_negative_mining and {'negative_per_positive_ratio', 'min_negative_per_image'} <= set(kw):
            mask = torch.empty((B, A), dtype=torch.uint8, device=dev)
            _lib.check(lib.ssdk_hard_negative_mining(_lib.ptr(scores), cls_col.data_ptr(), 6, B, A, C,
                                                     float(kw['negative_per_positive_ratio']),
                                                     int(kw['min_negative_per_image']), _lib.ptr(mask), _lib.ptr(ws),
                                                     ws.numel(), _lib.current_stream()), 'ssdk_hard_negative_mining')
            lse_valid = 1 if module.cls_kind in (SSDK_CLS_CROSS_ENTROPY, SSDK_CLS_SOFTMAX_FOCAL) else 0
        elif fn is _sampler.naive_sampler:
            mask = torch.empty((B, A), dtype=torch.uint8, device=dev)
            _lib.check(lib.ssdk_naive_sampler(cls_col.data_ptr(), 6, B, A, _lib.ptr(mask), _lib.current_stream()),
                       'ssdk_naive_sampler')
        elif fn is _sampler.valid_sampler:
            # the mask is this function's output (last_sampled_mask) only: the sigmoid-target kinds read the class column instead
            mask = torch.empty((B, A), dtype=torch.uint8, device=dev)
            _lib.check(lib.ssdk_valid_sampler(cls_col.data_ptr(), 6, B, A, _lib.ptr(mask), _lib.current_stream()),
                       'ssdk_valid_sampler')
            null_mask = module.cls_kind in _NULL_MASK_KINDS
        else:  # any user sampler with the reference's signature (multibox_loss.py:58)
            mask = module.sampler(scores.view(B, A, C), cls_col.long()).to(torch.uint8).contiguous()
        out3 = torch.empty((3,), dtype=torch.float32, device=dev)
        params = module.loss_params(dev, C)
        _lib.check(lib.ssdk_multibox_loss_fwd(ctypes.byref(params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors),
                                              _lib.ptr(target), None if null_mask else _lib.ptr(mask), B, A, C, lse_valid, _lib.ptr(out3), _lib.ptr(ws),
                                              ws.numel(), _lib.current_stream()), 'ssdk_multibox_loss_fwd')
        ctx.save_for_backward(scores, locs, anchors, target, mask, ws)
        ctx.module = module
        ctx.shape = (B, A, C)
        ctx.null_mask = null_mask
        ctx.sparse_rows = fn is _sampler.hard_negative_mining or fn is _sampler.naive_sampler   # (the gradient rows of the anchors that were not sampled are zeros)
        ctx.mark_non_differentiable(mask)
        ctx.set_materialize_grads(False)   # (an output nobody differentiated arrives as None, not as a zero tensor made by a fill launch)
        return out3[0], out3[1], out3[2], mask   # loss = class_loss + loc_loss (summed by the kernel: multibox_loss.py:93), class_loss, loc_loss

    @staticmethod
    def backward(ctx, g_total, g_class, g_loc, _g_mask):
        scores, locs, anchors, target, mask, ws = ctx.saved_tensors
        module = ctx.module
        B, A, C = ctx.shape
        if g_total is None and g_class is None and g_loc is None:
            return None, None, None, None, None
        # the usual case: only `loss` was differentiated -- its gradient (one device scalar) goes to the kernel as it is; anything else
        # (class_loss / loc_loss used on their own in the same backward pass) is combined into the two-element form first
        single = g_class is None and g_loc is None
        if single:
            grad_out = g_total.float().reshape(1).contiguous()
        else:
            zero = scores.new_zeros(())
            gt = zero if g_total is None else g_total.float().reshape(())
            grad_out = torch.stack([gt + (zero if g_class is None else g_class.float().reshape(())),
                                    gt + (zero if g_loc is None else g_loc.float().reshape(()))]).contiguous()
        dscores = torch.empty_like(scores)
        dlocs = torch.empty_like(locs)
        params = module.loss_params(scores.device, C)
        # under hard-negative mining a few % of the anchors carry a gradient: the kernel also writes which (row_mask), and the heads'
        # backward of this pass -- if it receives these very tensors -- reads only those rows instead of scanning all of dscores
        row_mask = torch.empty((B, A), dtype=torch.uint8, device=scores.device) if ctx.sparse_rows and not _NO_ROW_HINT else None
        _lib.check(_lib.lib().ssdk_multibox_loss_bwd_ex(ctypes.byref(params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors),
                                                        _lib.ptr(target), None if ctx.null_mask else _lib.ptr(mask), _lib.ptr(grad_out), 1 if single else 0, B, A, C,
                                                        _lib.ptr(dscores),
                                                        _lib.ptr(dlocs), _lib.ptr(row_mask), _lib.ptr(ws), ws.numel(), _lib.current_stream()),
                   'ssdk_multibox_loss_bwd')
        if row_mask is not None:
            from ..modules import heads as heads_mod
            heads_mod.set_row_hint(dscores, dlocs, row_mask)
        return dscores, dlocs, None, None, None


class MultiboxLoss(nn.Module):
    def __init__(self,
                 sampler,
                 box_coder,
                 classification_loss,
                 localization_loss,
                 classification_weight=1.0,
                 localization_weight=1.0,
                 distribution_loss=None,
                 distribution_weight=0.25):
        super(MultiboxLoss, self).__init__()
        self.sampler = sampler
        self.box_coder = box_coder

        # the integral box head (IntegralBoxCoder: pred[1] holds 4 * bins logits per anchor) and its Distribution Focal Loss, which runs
        # inside the integral's kernels (csrc/integral.hip); without distribution_loss the head is integral regression alone (weight 0)
        self.integral = hasattr(box_coder, 'integrate_with_target')
        self.distribution_loss = None
        self.distribution_weight = 0.0
        if distribution_loss is not None:
            if not isinstance(distribution_loss, dict) or distribution_loss.get('name') != 'DistributionFocalLoss':
                raise ValueError(f"distribution_loss: {distribution_loss!r}, expected {{'name': 'DistributionFocalLoss'}}")
            if not self.integral:
                raise ValueError('distribution_loss needs an IntegralBoxCoder (the loc head must predict distributions)')
            self.distribution_loss = get_ctor(losses, 'DistributionFocalLoss')(reduction='sum', **{'reg_max': box_coder.reg_max, **distribution_loss})
            if self.distribution_loss.reg_max != box_coder.reg_max:
                raise ValueError(f'distribution_loss: reg_max={self.distribution_loss.reg_max}, the box coder has {box_coder.reg_max}')
            self.distribution_weight = float(distribution_weight)
        self.last_distribution_loss = None

        # multibox_loss.py:23-30 -- same constructor dance, so the same keywords survive filter_kwargs
        ClassificationLoss = get_ctor(losses, classification_loss['name'])
        self.classification_loss = ClassificationLoss(reduction='sum', ignore_index=IGNORE_CLASS, **classification_loss)
        self.soft_target = getattr(self.classification_loss, 'SOFT_TARGET', False)
        self.multiclass = getattr(self.classification_loss, 'MULTICLASS', False)
        LocalizationLoss = get_ctor(losses, localization_loss['name'])
        self.localization_loss = LocalizationLoss(reduction='sum', **localization_loss)
        self.iou_loss = getattr(self.localization_loss, 'IOU_LOSS', False)

        self.classification_weight = classification_weight
        self.localization_weight = localization_weight

        cl = self.classification_loss
        self.focal_gamma, self.focal_alpha, self.focal_reduce_mean, self.soft_epsilon = 2.0, 0.25, 0, 0.0
        self.ce_label_smoothing, self.class_weight = 0.0, None
        self.quality_from_iou = 0
        if isinstance(cl, losses.CrossEntropyLoss):
            if cl.reduction != 'sum' or cl.ignore_index != IGNORE_CLASS:
                raise NotImplementedError('CrossEntropyLoss: only reduction=sum, ignore_index=-1')
            self.cls_kind = SSDK_CLS_CROSS_ENTROPY
            self.ce_label_smoothing = float(cl.label_smoothing)
            if not 0.0 <= self.ce_label_smoothing <= 1.0:
                raise ValueError(f'CrossEntropyLoss: label_smoothing={self.ce_label_smoothing} outside [0, 1]')
            if cl.weight is not None:
                if cl.weight.dim() != 1:
                    raise ValueError('CrossEntropyLoss: weight must be a 1-D tensor of one value per class')
                self.class_weight = cl.weight.detach()
        elif isinstance(cl, losses.SigmoidFocalLoss):
            if cl.reduction not in ('mean', 'sum'):
                raise NotImplementedError("SigmoidFocalLoss: reduction must be 'mean' or 'sum'")
            self.cls_kind = SSDK_CLS_SIGMOID_FOCAL
            self.focal_gamma, self.focal_alpha = float(cl.gamma), float(cl.alpha)
            self.focal_reduce_mean = 1 if cl.reduction == 'mean' else 0
        elif isinstance(cl, (losses.QualityFocalLoss, losses.VarifocalLoss)):
            if cl.reduction not in ('mean', 'sum'):
                raise NotImplementedError(f"{type(cl).__name__}: reduction must be 'mean' or 'sum'")
            if isinstance(cl, losses.QualityFocalLoss):
                self.cls_kind, self.focal_gamma = SSDK_CLS_QUALITY_FOCAL, float(cl.beta)
            else:
                self.cls_kind, self.focal_gamma, self.focal_alpha = SSDK_CLS_VARIFOCAL, float(cl.gamma), float(cl.alpha)
            self.focal_reduce_mean = 1 if cl.reduction == 'mean' else 0
            self.quality_from_iou = 1 if cl.use_iou else 0
        elif isinstance(cl, losses.SoftmaxFocalLoss):
            if cl.reduction not in ('mean', 'sum') or cl.ignore_index != IGNORE_CLASS:
                raise NotImplementedError("SoftmaxFocalLoss: reduction must be 'mean' or 'sum' and ignore_index -1")
            self.cls_kind = SSDK_CLS_SOFTMAX_FOCAL
            self.focal_gamma = float(cl.gamma)
            self.focal_alpha = -1.0 if cl.alpha is None else float(cl.alpha)
            self.focal_reduce_mean = 1 if cl.reduction == 'mean' else 0
        elif isinstance(cl, (losses.CrossEntropyWithSoftTargetsLoss, losses.BinaryCrossEntropyWithSoftTargetsLoss)):
            if cl.reduction != 'sum':
                raise NotImplementedError(f'{type(cl).__name__}: only reduction=sum')
            self.cls_kind = SSDK_CLS_BCE_SOFT if self.multiclass else SSDK_CLS_CE_SOFT   # multibox_loss.py:64 tests multiclass first
            self.soft_epsilon = float(cl.epsilon)
        else:
            raise NotImplementedError(f'classification loss {type(cl).__name__} is not on the GPU path')
        ll = self.localization_loss
        self.smooth_l1_beta = 1.0   # (SmoothL1Loss beta; HuberLoss delta)
        if isinstance(ll, losses.SmoothL1Loss) and ll.reduction == 'sum':
            self.loc_kind = SSDK_LOC_SMOOTH_L1
            self.smooth_l1_beta = float(getattr(ll, 'beta', 1.0))   # (0: torch's L1 case, taken by the kernel as such)
            if self.smooth_l1_beta < 0:
                raise ValueError(f'SmoothL1Loss: beta={self.smooth_l1_beta} must be >= 0')
        elif isinstance(ll, losses.GeneralizedIoULoss) and ll.reduction == 'sum':
            self.loc_kind = SSDK_LOC_GIOU
        elif isinstance(ll, losses.IoULoss) and ll.reduction == 'sum':
            self.loc_kind = SSDK_LOC_IOU
        elif isinstance(ll, losses.DistanceIoULoss) and ll.reduction == 'sum':
            self.loc_kind = SSDK_LOC_DIOU
        elif isinstance(ll, losses.CompleteIoULoss) and ll.reduction == 'sum':
            self.loc_kind = SSDK_LOC_CIOU
        elif isinstance(ll, losses.EfficientIoULoss) and ll.reduction == 'sum':
            self.loc_kind = SSDK_LOC_EIOU
        elif isinstance(ll, losses.L1Loss) and ll.reduction == 'sum':
            self.loc_kind = SSDK_LOC_L1
        elif isinstance(ll, losses.MSELoss) and ll.reduction == 'sum':
            self.loc_kind = SSDK_LOC_MSE
        elif isinstance(ll, losses.HuberLoss) and ll.reduction == 'sum':
            self.loc_kind = SSDK_LOC_HUBER
            self.smooth_l1_beta = float(ll.delta)
            if self.smooth_l1_beta <= 0:
                raise ValueError(f'HuberLoss: delta={self.smooth_l1_beta} must be > 0')
        else:
            raise NotImplementedError(f'localization loss {type(ll).__name__}(reduction={ll.reduction}) is not on the GPU path')
        self._class_weight_dev = {}   # device -> the fp32 [C] copy of class_weight the kernels read (one per device, kept: graph replays)
        self.last_sampled_mask = None

    def class_weight_on(self, device, num_classes):
        """CrossEntropyLoss ``weight`` as a contiguous fp32 [C] tensor on ``device`` (None without weights).  Made on the first call for a
        device and kept by this object, so every later forward / backward -- and a captured graph's replays -- read the same address."""
        if self.class_weight is None:
            return None
        if self.class_weight.numel() != num_classes:
            raise ValueError(f'CrossEntropyLoss: weight has {self.class_weight.numel()} values for {num_classes} classes')
        w = self._class_weight_dev.get(device)
        if w is None:
            w = self.class_weight.to(device=device, dtype=torch.float32).contiguous()
            self._class_weight_dev[device] = w
        return w

    def loss_params(self, device=None, num_classes=None):
        """ssdk_loss_params of this loss; ``device`` / ``num_classes`` place the class weights (needed only with a ``weight``)."""
        w = self.class_weight_on(device, num_classes) if self.class_weight is not None else None
        return _lib.LossParams(self.cls_kind, self.loc_kind, self.focal_gamma, self.focal_alpha, self.focal_reduce_mean,
                               self.soft_epsilon, float(self.classification_weight), float(self.localization_weight),
                               float(self.box_coder.xy_scale), float(self.box_coder.wh_scale), float(self.box_coder.eps),
                               self.smooth_l1_beta, self.ce_label_smoothing, None if w is None else w.data_ptr(), self.quality_from_iou)

    def forward(self, pred, anchors, target):
        """
        Args:
            pred: tuple of
                torch.tensor(:shape [Batch, AnchorBoxes * Classes])
                torch.tensor(:shape [Batch, AnchorBoxes * 4])  -- with an IntegralBoxCoder: [Batch, AnchorBoxes * 4 * bins] logits
            target: torch.tensor(:shape [Batch, AnchorBoxes, 6])  -- columns 0..3 are overwritten with the encoded
                regression targets, exactly like multibox_loss.py:81-82
        Returns:
            losses: (loss, class_loss, loc_loss) 0-dim tensors with autograd
        """
        scores, locs = pred
        _lib.require_cuda(scores, locs, anchors, target)
        if target.dtype != torch.float32 or not target.is_contiguous():
            raise ValueError('target must be a contiguous float32 [Batch, AnchorBoxes, 6] tensor')
        scores = scores.float().contiguous()
        locs = locs.float().contiguous()
        anchors = anchors.float().contiguous()
        dfl = None
        if self.integral:   # the integral node sees the RAW target first: _MultiboxLossFn may encode it in place
            if locs.dim() != 2 or locs.shape[1] != anchors.shape[0] * 4 * self.box_coder.bins:
                raise ValueError(f'IntegralBoxCoder: pred[1] of shape {tuple(locs.shape)} is not [Batch, AnchorBoxes * 4 * {self.box_coder.bins}]')
            locs, dfl = self.box_coder.integrate_with_target(locs, anchors, target, self.distribution_weight)
        loss, class_loss, loc_loss, mask = _MultiboxLossFn.apply(scores, locs, anchors, target, self)
        self.last_sampled_mask = mask
        if dfl is not None:
            self.last_distribution_loss = dfl.detach()
            if self.distribution_weight != 0.0:
                loss, loc_loss = loss + dfl, loc_loss + dfl
        return loss, class_loss, loc_loss
