"""TargetAssigner -- mirror of detection/target_assigner.py:17-63 on libssdk (csrc/match.hip); AtssTargetAssigner, the adaptive assigner
the reference does not have, beside it; TaskAlignedAssigner, the prediction-aware one of TOOD, and SimOtaAssigner, the dynamic top-k of
YOLOX, which it does not have either."""
import ctypes

import numpy as np
import torch

from .. import _lib

# detection/target_assigner.py:7-14
LOC_INDEX_START = 0
LOC_INDEX_END = 4
CLASS_INDEX = 4
SCORE_INDEX = 5
TARGET_SIZE = 6

NEGATIVE_CLASS = 0  # bf/datasets/detection_dataset.py:17
IGNORE_CLASS = -1

GT_ROW = 6  # x1, y1, x2, y2, class, score (bf/datasets/detection_dataset.py:11-15); extra columns are dropped


class PackedGroundTruth(object):
    """A batch's ground truth already on the device in the library's layout: ``rows`` [capacity, 6] fp32 (boxes of all images back to
    back, rows past ``offsets[-1]`` are padding), ``offsets`` int32 [B + 1].  ``TargetAssigner.encode_ground_truth`` takes it in place of
    the list of per-image tensors -- with no host-side packing and no H2D copy in the call, the training step can be captured in a HIP
    graph (graphs.py): keep ONE PackedGroundTruth of fixed capacity and ``update_`` it between replays."""

    def __init__(self, rows, offsets):
        assert rows.is_cuda and offsets.is_cuda and rows.dim() == 2 and rows.shape[1] == GT_ROW and rows.dtype == torch.float32
        assert offsets.dtype == torch.int32 and offsets.dim() == 1
        self.rows, self.offsets = rows.contiguous(), offsets.contiguous()

    @classmethod
    def from_list(cls, ground_truth, device, capacity=None):
        rows, offs, total = pack_ground_truth(ground_truth, device)
        cap = total if capacity is None else int(capacity)
        if cap < total:
            raise ValueError(f'PackedGroundTruth: {total} boxes do not fit the capacity of {cap}')
        buf = torch.zeros((max(cap, 1), GT_ROW), dtype=torch.float32, device=device)
        buf[:total] = rows
        return cls(buf, offs.clone())

    def update_(self, ground_truth):
        """New boxes into the same buffers (same batch size, at most the capacity): what a training loop does between graph replays."""
        rows, offs, total = pack_ground_truth(ground_truth, self.rows.device)
        if total > self.rows.shape[0] or offs.numel() != self.offsets.numel():
            raise ValueError('PackedGroundTruth.update_: batch size or capacity exceeded')
        self.rows[:total].copy_(rows, non_blocking=True)
        self.offsets.copy_(offs, non_blocking=True)
        return self

    def __len__(self):
        return self.offsets.numel() - 1


def pack_ground_truth(ground_truth, device, row=GT_ROW):
    """list[B] of [G_i, >=row] tensors (any device) -> (rows [sum G, row] fp32, offsets int32 [B+1]) on ``device``.

    One pinned staging buffer and one async H2D copy per batch (the reference moves each image's tensor
    separately, target_assigner.py:35).  ``row``: columns kept per box (6 for the target assigner; mixup keeps every
    attribute, e.g. the `difficult` flag at column 6 that the evaluation metric reads)."""
    GT_ROW = row   # (shadows the module constant below)
    counts = [int(g.size(0)) if g.dim() == 2 else 0 for g in ground_truth]
    total = sum(counts)
    if all((not g.is_cuda) for g in ground_truth):
        stage = torch.empty((total * GT_ROW + len(counts) + 1,), dtype=torch.float32)
        if torch.cuda.is_available():
            stage = stage.pin_memory()
        rows = stage[:total * GT_ROW].view(total, GT_ROW)
        offs = stage[total * GT_ROW:].view(torch.int32)
        pos = 0
        offs[0] = 0
        for i, (g, n) in enumerate(zip(ground_truth, counts)):
            if n:
                rows[pos:pos + n] = g[:, :GT_ROW].to(torch.float32)
            pos += n
            offs[i + 1] = pos
        dev = stage.to(device, non_blocking=True)
        return dev[:total * GT_ROW].view(total, GT_ROW), dev[total * GT_ROW:].view(torch.int32), total
    rows = torch.cat([g[:, :GT_ROW].to(device=device, dtype=torch.float32) for g, n in zip(ground_truth, counts) if n], dim=0) \
        if total else torch.zeros((0, GT_ROW), dtype=torch.float32, device=device)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(device, non_blocking=True)
    return rows.contiguous(), offs, total


class _Assigner(object):
    """What the four assigners do around their library call.  Every ``ssdk_encode_ground_truth*`` entry takes (rows, stride, offsets, batch,
    total, anchors, num_anchors, <its own arguments>, target, box_idx, <its further outputs>, workspace, bytes, stream) and has a
    ``*_workspace_bytes(batch, total, ...)`` beside it."""

    def __init__(self):
        self._ws = None
        self._levels = {}

    @staticmethod
    def _pack(ground_truth, device):
        """(rows, offsets, total) of a list of per-image tensors or of a ``PackedGroundTruth``."""
        if isinstance(ground_truth, PackedGroundTruth):
            return ground_truth.rows, ground_truth.offsets, ground_truth.rows.shape[0]   # (total = capacity: padding is skipped on the device)
        return pack_ground_truth(ground_truth, device)

    def _encode(self, entry, ground_truth, anchors, return_box_idx, ws_args, args, outputs=(), keep=(), packed=None):
        """Packs the ground truth, allocates ``target`` / ``box_idx``, grows the workspace and calls ``entry``: (target, box_idx)."""
        lib = _lib.lib()
        device = anchors.device
        batch_size = len(ground_truth)
        num_anchors = anchors.size(0)
        anchors = anchors.contiguous().float()
        rows, offs, total = packed or self._pack(ground_truth, device)
        target = torch.empty((batch_size, num_anchors, TARGET_SIZE), dtype=torch.float32, device=device)
        box_idx = torch.empty((batch_size, num_anchors), dtype=torch.int32, device=device) if return_box_idx else None
        need = getattr(lib, entry + '_workspace_bytes')(batch_size, total, *ws_args)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty((max(need, 4096),), dtype=torch.uint8, device=device)
        _lib.check(getattr(lib, entry)(_lib.ptr(rows), GT_ROW, _lib.ptr(offs), batch_size, total, _lib.ptr(anchors), num_anchors, *args,
                                       _lib.ptr(target), _lib.ptr(box_idx), *outputs, _lib.ptr(self._ws), self._ws.numel(),
                                       _lib.current_stream()), entry)
        # keep the staging tensors alive until the stream has consumed them
        target._ssdk_keepalive = (rows, offs) + tuple(keep)
        return target, box_idx

    def _prediction(self, prediction, box_coder):
        """``prediction = (scores, locs)`` and the box coder are there: (scores, locs)."""
        name = type(self).__name__
        if prediction is None or len(prediction) != 2:
            raise ValueError(f'{name}.encode_ground_truth: prediction must be (scores, locs)')
        if box_coder is None:
            raise ValueError(f'{name}.encode_ground_truth: box_coder is required (its scales decode the predicted boxes)')
        return prediction

    def _prepare(self, scores, locs, box_coder, batch_size, num_anchors):
        """The predictions as the library reads them -- detached, integrated where the coder is integral, fp32, contiguous -- and their
        shapes checked: (scores, locs, num_columns)."""
        name = type(self).__name__
        with torch.no_grad():
            scores, locs = scores.detach(), locs.detach()
            if hasattr(box_coder, 'integrate'):
                locs = box_coder.integrate(locs, num_anchors)
            scores, locs = scores.float().contiguous(), locs.float().contiguous()
        if scores.shape[0] != batch_size or locs.shape[0] != batch_size or locs.numel() != batch_size * num_anchors * 4:
            raise ValueError(f'{name}.encode_ground_truth: locs of shape {tuple(locs.shape)} / scores of shape '
                             f'{tuple(scores.shape)} for a batch of {batch_size} and {num_anchors} anchors')
        num_columns, rest = divmod(scores.numel(), batch_size * num_anchors)
        if rest or num_columns < 1:
            raise ValueError(f'{name}.encode_ground_truth: scores of shape {tuple(scores.shape)} are not [Batch, {num_anchors} * C]')
        return scores, locs, num_columns

    def _level_table(self, sizes, strides=()):
        """The host arrays the library reads the levels from, built once per (sizes, strides): (int32 sizes, float (sx, sy) pairs)."""
        key = (sizes, strides)
        if key not in self._levels:
            self._levels[key] = ((ctypes.c_int32 * len(sizes))(*sizes), (ctypes.c_float * (2 * len(strides)))(*[v for s in strides for v in s]))
        return self._levels[key]


FORCE_MATCH = {'per_prediction': 0, 'bipartite': 1}   # SSDK_FORCE_MATCH_* (include/ssdk.h)


class TargetAssigner(_Assigner):
    """``force_match`` (not in the reference; default ``'per_prediction'`` = the reference's rule): how every ground-truth box is given
    an anchor regardless of the thresholds.  ``'per_prediction'``: each box's best anchor, the highest box index winning an anchor that
    several boxes share (matcher.py:52-54) -- the boxes that lose it may end up with no positive anchor at all.  ``'bipartite'``: the
    threshold stage is ``match_per_prediction(..., force_match_for_each_target=False)``, then ``box_idx[anchor_idx] = box_idx_b`` with
    ``match_bipartite``'s greedy matching (matcher.py:7-31) -- every box an anchor of its own.  Unlike ``matcher.match_bipartite``, the
    fused stage stops once no remaining box overlaps a free anchor: those boxes get no forced anchor and box 0 keeps its own."""

    def __init__(self, matched_threshold, unmatched_threshold, force_match='per_prediction'):
        if force_match not in FORCE_MATCH:
            raise ValueError(f'TargetAssigner: force_match={force_match!r}, expected one of {sorted(FORCE_MATCH)}')
        super().__init__()
        self.matched_threshold = matched_threshold
        self.unmatched_threshold = unmatched_threshold
        self.force_match = force_match

    def encode_ground_truth(self, ground_truth, anchors, return_box_idx=False):
        """
        Args:
            ground_truth: list(:len Batch) of torch.tensor(:shape [Boxes_i, >=6])
            anchors: torch.tensor(:shape [AnchorBoxes, 4]) on the GPU
        Returns:
            target: torch.tensor(:shape [Batch, AnchorBoxes, 6]) on anchors.device
            (the reference runs this on the CPU because its anchors live there; here anchors are device-resident
            and so is the result -- the ``target.to(device)`` of detection/init.py:115 becomes a no-op)
        """
        _lib.require_cuda(anchors)
        mode = FORCE_MATCH[self.force_match]
        thresholds = (float(self.matched_threshold), float(self.unmatched_threshold))
        if mode:
            target, box_idx = self._encode('ssdk_encode_ground_truth_ex', ground_truth, anchors, return_box_idx, (mode,), thresholds + (mode,))
        else:   # the default: the entry point and the kernels it always had
            target, box_idx = self._encode('ssdk_encode_ground_truth', ground_truth, anchors, return_box_idx, (), thresholds)
        return (target, box_idx) if return_box_idx else target


ATSS_MAX_TOPK = 32     # SSDK_ATSS_MAX_TOPK (include/ssdk.h)


class AtssTargetAssigner(_Assigner):
    """Adaptive Training Sample Selection (arXiv:1912.02424, Algorithm 1; not in the reference) in place of the two IoU thresholds.  Per
    ground-truth box the ``topk`` anchors of every pyramid level nearest to the box centre are its candidates; the mean plus the
    (unbiased) standard deviation of their IoUs is that box's own threshold; a candidate is positive when its IoU reaches the threshold
    and its centre lies strictly inside the box; an anchor positive for several boxes takes the largest IoU, then the lowest box index.
    There is no ignore band and NO force stage: a box none of whose candidates qualifies (a sliver between anchor centres) has no
    positive anchor at all -- that is ATSS.  The exact rule, operation by operation: ``ssdk_encode_ground_truth_atss`` in include/ssdk.h."""

    def __init__(self, topk=9):
        if int(topk) != topk or not 1 <= topk <= ATSS_MAX_TOPK:
            raise ValueError(f'AtssTargetAssigner: topk={topk!r}, expected an integer in 1..{ATSS_MAX_TOPK}')
        super().__init__()
        self.topk = int(topk)

    def encode_ground_truth(self, ground_truth, anchors, return_box_idx=False, level_sizes=None):
        """Inputs and outputs as ``TargetAssigner.encode_ground_truth``; ``level_sizes``: the anchor count of every pyramid level, in the
        anchors' order (``Detector.anchor_level_sizes(anchors)``)."""
        num_anchors = anchors.size(0)
        if level_sizes is None:
            raise ValueError('AtssTargetAssigner.encode_ground_truth: level_sizes is required (Detector.anchor_level_sizes(anchors))')
        sizes = tuple(int(n) for n in level_sizes)
        if sum(sizes) != num_anchors:
            raise ValueError(f'AtssTargetAssigner.encode_ground_truth: level_sizes sum to {sum(sizes)}, the anchors are {num_anchors}')
        _lib.require_cuda(anchors)
        c_sizes, _ = self._level_table(sizes)
        target, box_idx = self._encode('ssdk_encode_ground_truth_atss', ground_truth, anchors, return_box_idx, (len(sizes),),
                                       (c_sizes, len(sizes), self.topk))
        return (target, box_idx) if return_box_idx else target


TAL_MAX_TOPK = 32      # SSDK_TAL_MAX_TOPK (include/ssdk.h)


class TaskAlignedAssigner(_Assigner):
    """Task Alignment Learning (TOOD, arXiv:2108.07755 section 3.2; not in the reference): the prediction-aware assigner of TOOD,
    PP-YOLOE and YOLOv6/v8.  An anchor is a candidate of a box when its centre lies strictly inside the box and its alignment
    ``m = s^alpha * u^beta`` -- ``s`` its OWN predicted probability of the box's class (sigmoid layout: class k is column k - 1), ``u``
    the IoU of its OWN decoded box with the box -- is among the ``topk`` largest of the box; a candidate of several boxes goes to the
    largest ``u``, then the lowest box index.  Column 5 of a positive row is ``score * m / (m_max + 1e-9) * u_max`` over the anchors its
    box kept: the soft target of ``QualityFocalLoss`` / ``VarifocalLoss`` with ``use_iou=False``.  There is no ignore band and NO force
    stage: a box without an anchor centre inside has no positive anchor.  The predictions are constants of the step (detached here;
    nothing has a gradient).  The exact rule, operation by operation: ``ssdk_encode_ground_truth_tal`` in include/ssdk.h."""

    def __init__(self, topk=13, alpha=1.0, beta=6.0):
        if isinstance(topk, bool) or int(topk) != topk or not 1 <= topk <= TAL_MAX_TOPK:
            raise ValueError(f'TaskAlignedAssigner: topk={topk!r}, expected an integer in 1..{TAL_MAX_TOPK}')
        for name, v in (('alpha', alpha), ('beta', beta)):
            try:
                ok = not isinstance(v, str) and 0.0 <= float(v) < float('inf')
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f'TaskAlignedAssigner: {name}={v!r}, expected a finite number >= 0')
        super().__init__()
        self.topk, self.alpha, self.beta = int(topk), float(alpha), float(beta)

    def encode_ground_truth(self, ground_truth, anchors, prediction, box_coder, return_box_idx=False):
        """Inputs and outputs as ``TargetAssigner.encode_ground_truth``; beside them ``prediction = (scores, locs)`` as the detector returns
        them (``[Batch, AnchorBoxes * C]`` class logits -- C is taken from the shape -- and ``[Batch, AnchorBoxes * 4]`` encoded boxes) and
        the ``box_coder`` whose ``xy_scale`` / ``wh_scale`` decode them.  With an ``IntegralBoxCoder`` the loc head's distributions are
        first integrated (``box_coder.integrate`` under ``no_grad``): one more pass over the loc logits than the loss itself makes."""
        scores, locs = self._prediction(prediction, box_coder)
        _lib.require_cuda(anchors, scores, locs)
        scores, locs, num_columns = self._prepare(scores, locs, box_coder, len(ground_truth), anchors.size(0))
        target, box_idx = self._encode('ssdk_encode_ground_truth_tal', ground_truth, anchors, return_box_idx, (self.topk,),
                                       (_lib.ptr(scores), num_columns, _lib.ptr(locs), float(box_coder.xy_scale), float(box_coder.wh_scale),
                                        self.topk, self.alpha, self.beta), keep=(scores, locs))
        return (target, box_idx) if return_box_idx else target


SIMOTA_MAX_TOPK = 32   # SSDK_SIMOTA_MAX_TOPK (include/ssdk.h)
SIMOTA_MAX_LEVELS = 16   # SSDK_ATSS_MAX_LEVELS


class SimOtaAssigner(_Assigner):
    """SimOTA (YOLOX, arXiv:2107.08430 section 2.4: OTA with the Sinkhorn iteration replaced by a dynamic top-k; not in the reference):
    the assigner that decides HOW MANY positives a box gets from the prediction itself.  A box's region is the anchors whose centre lies
    strictly inside it or inside a square of ``center_radius`` cells of the anchor's own level around the box centre; the cost of a region
    anchor is the binary cross-entropy of its OWN class logits against the box's one-hot row plus ``iou_weight * -log(u)``, ``u`` the IoU
    of its OWN decoded box with the box; the box gets ``k = clamp(int(sum of its candidate_topk largest u), 1, #region)`` positives, its
    ``k`` region anchors smallest by (outside the box or the square, cost, anchor index); a candidate of several boxes goes to the
    smallest (outside, cost), then the lowest box index.  Column 5 of a positive row is the box's score -- ``QualityFocalLoss(use_iou=True)``
    forms YOLOX's IoU-aware class target from it.  There is no ignore band and NO force stage: a box without a region anchor has no
    positive anchor.  One stated deviation from YOLOX: a box ranks only anchors of its own region.  The predictions are constants of the
    step (detached here; nothing has a gradient).  The exact rule, operation by operation: ``ssdk_encode_ground_truth_simota`` in
    include/ssdk.h."""

    def __init__(self, center_radius=2.5, candidate_topk=10, iou_weight=3.0):
        try:
            ok = not isinstance(candidate_topk, (bool, str)) and int(candidate_topk) == candidate_topk and 1 <= candidate_topk <= SIMOTA_MAX_TOPK
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(f'SimOtaAssigner: candidate_topk={candidate_topk!r}, expected an integer in 1..{SIMOTA_MAX_TOPK}')
        for name, v, strict in (('center_radius', center_radius, True), ('iou_weight', iou_weight, False)):
            try:
                ok = not isinstance(v, (str, bool)) and 0.0 <= float(v) < float('inf') and not (strict and float(v) == 0.0)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"SimOtaAssigner: {name}={v!r}, expected a finite number {'> 0' if strict else '>= 0'}")
        super().__init__()
        self.center_radius, self.candidate_topk, self.iou_weight = float(center_radius), int(candidate_topk), float(iou_weight)

    def encode_ground_truth(self, ground_truth, anchors, prediction, box_coder, level_sizes=None, level_strides=None, return_box_idx=False,
                            return_dynamic_k=False):
        """Inputs and outputs as ``TaskAlignedAssigner.encode_ground_truth``; beside them ``level_sizes``, the anchor count of every pyramid
        level in the anchors' order (``Detector.anchor_level_sizes(anchors)``), and ``level_strides``, per level ``(sx, sy)`` image pixels
        per cell of its map or one number for both (``Detector.anchor_level_strides(anchors)``).  ``return_dynamic_k``: also the int32
        ``[capacity]`` tensor of every box's ``k`` (after ``box_idx`` when both are asked for).  With an ``IntegralBoxCoder`` the loc head's
        distributions are first integrated (``box_coder.integrate`` under ``no_grad``): one more pass over the loc logits than the loss
        itself makes."""
        scores, locs = self._prediction(prediction, box_coder)
        num_anchors = anchors.size(0)
        if level_sizes is None or level_strides is None:
            raise ValueError('SimOtaAssigner.encode_ground_truth: level_sizes and level_strides are required '
                             '(Detector.anchor_level_sizes(anchors), Detector.anchor_level_strides(anchors))')
        sizes = tuple(int(n) for n in level_sizes)
        strides = tuple((float(s), float(s)) if not hasattr(s, '__len__') else (float(s[0]), float(s[1])) for s in level_strides)
        if sum(sizes) != num_anchors:
            raise ValueError(f'SimOtaAssigner.encode_ground_truth: level_sizes sum to {sum(sizes)}, the anchors are {num_anchors}')
        if len(strides) != len(sizes) or not 1 <= len(sizes) <= SIMOTA_MAX_LEVELS:
            raise ValueError(f'SimOtaAssigner.encode_ground_truth: {len(strides)} level_strides for {len(sizes)} levels (1..{SIMOTA_MAX_LEVELS})')
        if not all(0.0 < v < float('inf') for s in strides for v in s):
            raise ValueError(f'SimOtaAssigner.encode_ground_truth: level_strides={strides!r} must be finite and positive')
        _lib.require_cuda(anchors, scores, locs)
        c_sizes, c_strides = self._level_table(sizes, strides)
        scores, locs, num_columns = self._prepare(scores, locs, box_coder, len(ground_truth), num_anchors)
        packed = self._pack(ground_truth, anchors.device)
        total = packed[2]
        dynamic_k = torch.empty((max(total, 1),), dtype=torch.int32, device=anchors.device)[:total] if return_dynamic_k else None
        target, box_idx = self._encode('ssdk_encode_ground_truth_simota', ground_truth, anchors, return_box_idx, (num_anchors, len(sizes)),
                                       (c_sizes, c_strides, len(sizes), _lib.ptr(scores), num_columns, _lib.ptr(locs), float(box_coder.xy_scale),
                                        float(box_coder.wh_scale), self.center_radius, self.candidate_topk, self.iou_weight),
                                       outputs=(_lib.ptr(dynamic_k) if total else None,), keep=(scores, locs), packed=packed)
        out = (target,) + ((box_idx,) if return_box_idx else ()) + ((dynamic_k,) if return_dynamic_k else ())
        return out if len(out) > 1 else target
