"""detection/matcher.py.  In the training path the matcher (match_per_prediction, matcher.py:33-56) is fused with the IoU into
``ssdk_encode_ground_truth`` (csrc/match.hip) and no [Boxes, AnchorBoxes] matrix exists; ``match_per_prediction`` below is the
reference's own function on a given weight matrix (``ssdk_match_per_prediction``), ``match_boxes`` the fused form for one box set.
``match_bipartite`` (matcher.py:7-31) is the reference's own function on a given matrix too (``ssdk_match_bipartite``); nothing in the
reference calls it, here it is also the opt-in force stage of the fused path (``TargetAssigner(force_match='bipartite')``).
``match_atss`` is the one-image form of ``AtssTargetAssigner`` (``ssdk_encode_ground_truth_atss``), which the reference does not have;
``match_task_aligned`` that of ``TaskAlignedAssigner`` (``ssdk_encode_ground_truth_tal``) and ``match_simota`` that of ``SimOtaAssigner``
(``ssdk_encode_ground_truth_simota``), which it does not have either."""
import torch

from .. import _lib

NOT_MATCHED = -2  # matcher.py:4
IGNORE = -1       # matcher.py:5


def match_bipartite(weights, inplace=False):
    """
    Args:
        weights: torch.tensor(:shape [Boxes, AnchorBoxes]) fp32 on the GPU
    Returns:
        box_idx: torch.tensor(:shape [Boxes]) int64
        anchor_idx: torch.tensor(:shape [Boxes]) int64 -- matcher.py:7-31: Boxes times, the argmax of the whole matrix (first flat index
        on ties) gives that row that column, then the column and the row are zeroed.

    Exhaustion (two boxes whose only positive entry is the same column, or Boxes > AnchorBoxes): once the maximum is 0 the reference's
    argmax is flat index 0 in every later round, so ``anchor_idx[0] == 0`` whenever a box was left over, as there; the left-over boxes'
    entries, which the reference leaves as ``torch.empty`` made them, are -1 here.  ``inplace=True`` (fp32 contiguous ``weights``)
    leaves ``weights`` as the reference leaves it; otherwise it is untouched.  The reference's assert (a row without a positive entry,
    a NaN maximum included) raises AssertionError here too and costs one sync, as there.
    """
    _lib.require_cuda(weights)
    if weights.dim() != 2 or weights.size(0) == 0 or weights.size(1) == 0:
        raise ValueError('weights must be [Boxes, AnchorBoxes] with at least one box and one anchor')
    assert weights.max(dim=1)[0].gt(0).all().item()   # matcher.py:15
    if inplace and not (weights.dtype == torch.float32 and weights.is_contiguous()):
        raise ValueError('match_bipartite(inplace=True) takes a contiguous fp32 matrix')
    lib = _lib.lib()
    w = weights if inplace else weights.float().contiguous()
    G, A = w.shape
    anchor_idx = torch.empty((G,), dtype=torch.int64, device=w.device)
    num_matched = torch.empty((1,), dtype=torch.int32, device=w.device)
    ws = _lib.scratch(lib.ssdk_match_bipartite_workspace_bytes(G, A), w.device, 'match_bipartite')
    _lib.check(lib.ssdk_match_bipartite(_lib.ptr(w), G, A, int(bool(inplace)), _lib.ptr(anchor_idx), _lib.ptr(num_matched), _lib.ptr(ws),
                                        ws.numel(), _lib.current_stream()), 'ssdk_match_bipartite')
    return torch.arange(G, dtype=torch.int64, device=w.device), anchor_idx


def _gt_rows(gt_boxes, gt_classes=None):
    """One image's [G, 6] rows for the assigners: the corners; with ``gt_classes`` also the class and a score of 1, else both 0."""
    gt = torch.zeros((gt_boxes.size(0), 6), dtype=torch.float32, device=gt_boxes.device)
    gt[:, :4] = gt_boxes[:, :4]
    if gt_classes is not None:
        gt[:, 4] = gt_classes.to(gt.device).reshape(-1).float()
        gt[:, 5] = 1.0
    return gt


def match_boxes(gt_boxes, anchors, matched_threshold, unmatched_threshold=None, force_match='per_prediction'):
    """box_idx int64 [A] for one image: IoU (box_utils.py:83-101) + match_per_prediction (matcher.py:33-56,
    force_match_for_each_target=True) on the GPU.  ``gt_boxes`` [G, >=4] corner form, ``anchors`` [A,4] centroid.
    ``force_match='bipartite'``: the force stage is match_bipartite's (see ``TargetAssigner``)."""
    from .target_assigner import TargetAssigner
    if unmatched_threshold is None:
        unmatched_threshold = matched_threshold
    gt = _gt_rows(gt_boxes)
    _, idx = TargetAssigner(matched_threshold, unmatched_threshold, force_match).encode_ground_truth([gt], anchors, return_box_idx=True)
    return idx[0].long()


def match_atss(gt_boxes, anchors, level_sizes, topk=9):
    """box_idx int64 [A] for one image by Adaptive Training Sample Selection (``AtssTargetAssigner``; not in the reference): the box an
    anchor is positive for, else NOT_MATCHED -- there is no ignore band and no force stage.  ``gt_boxes`` [G, >=4] corner form,
    ``anchors`` [A,4] centroid, ``level_sizes`` the anchor count of every pyramid level."""
    from .target_assigner import AtssTargetAssigner
    gt = _gt_rows(gt_boxes)
    _, idx = AtssTargetAssigner(topk).encode_ground_truth([gt], anchors, return_box_idx=True, level_sizes=level_sizes)
    return idx[0].long()


def match_per_prediction(weights, matched_threshold, unmatched_threshold=None, force_match_for_each_target=True):
    """
    Args:
        weights: torch.tensor(:shape [Boxes, AnchorBoxes]) on the GPU
    Returns:
        box_idx: torch.tensor(:shape [AnchorBoxes]) int64 -- matcher.py:33-56
    """
    if unmatched_threshold is None:
        unmatched_threshold = matched_threshold
    else:
        assert matched_threshold >= unmatched_threshold   # matcher.py:43
    _lib.require_cuda(weights)
    if weights.dim() != 2 or weights.size(0) == 0:
        raise ValueError('weights must be [Boxes, AnchorBoxes] with at least one box (torch.max over an empty dim fails in the reference)')
    lib = _lib.lib()
    w = weights.float().contiguous()
    G, A = w.shape
    box_idx = torch.empty((A,), dtype=torch.int64, device=w.device)
    ws = _lib.scratch(lib.ssdk_match_per_prediction_workspace_bytes(G), w.device, 'match_per_prediction')
    _lib.check(lib.ssdk_match_per_prediction(_lib.ptr(w), G, A, float(matched_threshold), float(unmatched_threshold),
                                             int(bool(force_match_for_each_target)), _lib.ptr(box_idx), _lib.ptr(ws), ws.numel(),
                                             _lib.current_stream()), 'ssdk_match_per_prediction')
    return box_idx


def match_task_aligned(gt_boxes, gt_classes, anchors, scores, locs, box_coder, topk=13, alpha=1.0, beta=6.0):
    """box_idx int64 [A] for one image by Task Alignment Learning (``TaskAlignedAssigner``; not in the reference): the box an anchor is
    positive for, else NOT_MATCHED -- there is no ignore band and no force stage.  ``gt_boxes`` [G, >=4] corner form, ``gt_classes`` [G]
    (1-based: class k is column k - 1 of the logits), ``anchors`` [A, 4] centroid, ``scores`` [A, C] (or [A * C]) class logits and ``locs``
    [A, 4] (or [A * 4]) encoded boxes of that image, ``box_coder`` the coder that decodes them."""
    from .target_assigner import TaskAlignedAssigner
    gt = _gt_rows(gt_boxes, gt_classes)
    _, idx = TaskAlignedAssigner(topk, alpha, beta).encode_ground_truth([gt], anchors, (scores.reshape(1, -1), locs.reshape(1, -1)), box_coder,
                                                                         return_box_idx=True)
    return idx[0].long()


def match_simota(gt_boxes, gt_classes, anchors, scores, locs, box_coder, level_sizes, level_strides, center_radius=2.5, candidate_topk=10,
                 iou_weight=3.0):
    """box_idx int64 [A] for one image by SimOTA (``SimOtaAssigner``; not in the reference): the box an anchor is positive for, else
    NOT_MATCHED -- there is no ignore band and no force stage.  ``gt_boxes`` [G, >=4] corner form, ``gt_classes`` [G] (1-based: class k is
    column k - 1 of the logits), ``anchors`` [A, 4] centroid, ``scores`` [A, C] (or [A * C]) class logits and ``locs`` [A, 4] (or [A * 4])
    encoded boxes of that image, ``box_coder`` the coder that decodes them, ``level_sizes`` the anchor count and ``level_strides`` the
    ``(sx, sy)`` image pixels per cell of every pyramid level."""
    from .target_assigner import SimOtaAssigner
    gt = _gt_rows(gt_boxes, gt_classes)
    _, idx = SimOtaAssigner(center_radius, candidate_topk, iou_weight).encode_ground_truth(
        [gt], anchors, (scores.reshape(1, -1), locs.reshape(1, -1)), box_coder, level_sizes=level_sizes, level_strides=level_strides,
        return_box_idx=True)
    return idx[0].long()
