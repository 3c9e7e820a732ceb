"""BoxCoder -- mirror of detection/box_coder.py:4-57 on libssdk (csrc/loss.hip)."""
import ctypes

import torch

from .. import _lib


class BoxCoder(torch.nn.Module):
    def __init__(self, xy_scale, wh_scale, eps=1e-8):
        super(BoxCoder, self).__init__()
        self.xy_scale = xy_scale
        self.wh_scale = wh_scale
        self.eps = eps

    @staticmethod
    def _shape(boxes, priors):
        A = priors.size(0)
        assert boxes.size(-1) == 4 and boxes.numel() % (A * 4) == 0
        return boxes.numel() // (A * 4), A

    def encode_box(self, boxes, priors, inplace=False):
        """boxes [Batch, AnchorBoxes, 4] centroid form -> encoded (box_coder.py:13-34).  ``inplace`` selects the
        reference's in-place arithmetic (eps added after the divide) and overwrites ``boxes``."""
        _lib.require_cuda(boxes, priors)
        B, A = self._shape(boxes, priors)
        src = boxes if boxes.is_contiguous() and boxes.dtype == torch.float32 else boxes.contiguous().float()
        out = src if inplace else torch.empty_like(src)
        _lib.check(_lib.lib().ssdk_encode_box(_lib.ptr(src), _lib.ptr(priors.contiguous().float()), _lib.ptr(out), B, A,
                                              float(self.xy_scale), float(self.wh_scale), float(self.eps),
                                              1 if inplace else 0, _lib.current_stream()), 'ssdk_encode_box')
        if inplace and out is not boxes:
            boxes.copy_(out)
            return boxes
        return out

    def decode_box(self, boxes, priors, inplace=torch.tensor(0)):
        """encoded [Batch, AnchorBoxes, 4] -> centroid boxes (box_coder.py:37-57)."""
        _lib.require_cuda(boxes, priors)
        B, A = self._shape(boxes, priors)
        do_inplace = bool(inplace)
        src = boxes if boxes.is_contiguous() and boxes.dtype == torch.float32 else boxes.contiguous().float()
        out = src if do_inplace else torch.empty_like(src)
        _lib.check(_lib.lib().ssdk_decode_box(_lib.ptr(src), _lib.ptr(priors.contiguous().float()), _lib.ptr(out), B, A,
                                              float(self.xy_scale), float(self.wh_scale), 1 if do_inplace else 0,
                                              _lib.current_stream()), 'ssdk_decode_box')
        if do_inplace and out is not boxes:
            boxes.copy_(out)
            return boxes
        return out


class _IntegralFn(torch.autograd.Function):
    """(locs [B, A*4], dfl) = f(logits [B, A*4*bins]) on ssdk_integral_fwd / ssdk_integral_bwd (csrc/integral.hip).  With a target the
    forward also takes the Distribution Focal Loss of the positive rows and keeps their target positions in its workspace, so it has to run
    before the multibox loss encodes the target in place; the backward is ONE launch for both upstream gradients."""

    @staticmethod
    def forward(ctx, logits, anchors, target, coder, weight):
        lib = _lib.lib()
        B = logits.shape[0]
        A = logits.numel() // (B * 4 * coder.bins)
        dev = logits.device
        params = coder.integral_params(weight)
        locs = torch.empty((B, A * 4), dtype=torch.float32, device=dev)
        out2 = ws = None
        if target is not None:
            out2 = torch.empty((2,), dtype=torch.float32, device=dev)
            ws = torch.empty((lib.ssdk_integral_workspace_bytes(B, A),), dtype=torch.uint8, device=dev)
        _lib.check(lib.ssdk_integral_fwd(ctypes.byref(params), _lib.ptr(logits), _lib.ptr(anchors), _lib.ptr(target), B, A, _lib.ptr(locs),
                                         _lib.ptr(out2), _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.current_stream()),
                   'ssdk_integral_fwd')
        ctx.save_for_backward(logits, target, ws)
        ctx.params = params
        ctx.shape = (B, A)
        ctx.set_materialize_grads(False)   # (a gradient nobody asked for arrives as None -> NULL, not as a zero tensor made by a fill launch)
        if target is None:
            return locs, logits.new_zeros(())
        return locs, out2[0]

    @staticmethod
    def backward(ctx, dlocs, g_dfl):
        logits, target, ws = ctx.saved_tensors
        if dlocs is None and g_dfl is None:
            return None, None, None, None, None
        B, A = ctx.shape
        if dlocs is not None:
            dlocs = dlocs.float().contiguous()
        if target is None or ctx.params.distribution_weight == 0.0:
            g_dfl = None
        elif g_dfl is not None:
            g_dfl = g_dfl.float().reshape(1).contiguous()
        dlogits = torch.empty_like(logits)
        cls = None if target is None else target[..., 4]
        _lib.check(_lib.lib().ssdk_integral_bwd(ctypes.byref(ctx.params), _lib.ptr(logits), _lib.ptr(dlocs), None if cls is None else cls.data_ptr(), 6,
                                                _lib.ptr(g_dfl), B, A, _lib.ptr(dlogits), _lib.ptr(ws), 0 if ws is None else ws.numel(),
                                                _lib.current_stream()), 'ssdk_integral_bwd')
        return dlogits, None, None, None, None


class IntegralBoxCoder(BoxCoder):
    """BoxCoder whose loc head predicts, per encoded coordinate, a discrete distribution over ``bins = reg_max + 1`` grid values
    (Generalized Focal Loss, arXiv:2006.04388; not in the reference): side k's grid is ``-L_k + i * 2 L_k / reg_max`` with L = ``xy_limit``
    for tx, ty and ``wh_limit`` for tw, th, and the coordinate is the distribution's expectation.  ``encode_box`` / ``decode_box`` are
    BoxCoder's; ``integrate`` turns the logits into an ordinary ``locs`` tensor (include/ssdk.h: ssdk_integral_fwd)."""

    def __init__(self, xy_scale, wh_scale, eps=1e-8, reg_max=16, xy_limit=8.0, wh_limit=8.0):
        super(IntegralBoxCoder, self).__init__(xy_scale, wh_scale, eps)
        reg_max = int(reg_max)
        if not 1 <= reg_max <= 63:
            raise ValueError(f'IntegralBoxCoder: reg_max={reg_max} outside [1, 63]')
        if not (xy_limit > 0 and wh_limit > 0):
            raise ValueError('IntegralBoxCoder: xy_limit and wh_limit must be positive')
        self.reg_max = reg_max
        self.bins = reg_max + 1
        self.xy_limit = float(xy_limit)
        self.wh_limit = float(wh_limit)

    def integral_params(self, distribution_weight=0.0):
        return _lib.IntegralParams(self.bins, self.xy_limit, self.wh_limit, float(self.xy_scale), float(self.wh_scale), float(self.eps),
                                   float(distribution_weight))

    def check_logits(self, logits, num_anchors):
        if logits.dim() < 1 or logits.numel() != logits.shape[0] * num_anchors * 4 * self.bins:
            raise ValueError(f'IntegralBoxCoder: loc logits of shape {tuple(logits.shape)} are not [Batch, {num_anchors} * 4 * {self.bins}]')

    def integrate(self, logits, num_anchors):
        """logits [Batch, AnchorBoxes * 4 * bins] -> encoded locs [Batch, AnchorBoxes * 4], with autograd."""
        _lib.require_cuda(logits)
        self.check_logits(logits, num_anchors)
        return _IntegralFn.apply(logits.float().contiguous(), None, None, self, 0.0)[0]

    def integrate_with_target(self, logits, anchors, target, distribution_weight):
        """(locs, Distribution Focal Loss value) for MultiboxLoss: ``target`` is the RAW [Batch, AnchorBoxes, 6] target (before the loss
        encodes it in place)."""
        _lib.require_cuda(logits, anchors, target)
        self.check_logits(logits, anchors.shape[0])
        return _IntegralFn.apply(logits.float().contiguous(), anchors, target, self, float(distribution_weight))


BOX_CODERS = {'BoxCoder': BoxCoder, 'IntegralBoxCoder': IntegralBoxCoder}


def build_box_coder(args):
    """A config's ``box_coder`` dict.  ``'name'`` (not in the reference) picks the class, by default ``'BoxCoder'``, whose keywords the
    other entries are: ``{'name': 'IntegralBoxCoder', 'xy_scale': 10.0, 'wh_scale': 5.0, 'reg_max': 16}``."""
    args = dict(args)
    name = args.pop('name', 'BoxCoder')
    if name not in BOX_CODERS:
        raise ValueError(f'box_coder: name={name!r}, expected one of {sorted(BOX_CODERS)}')
    return BOX_CODERS[name](**args)
