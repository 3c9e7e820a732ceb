"""coco_evaluation -- COCO-style bbox metrics (AP@[.50:.95], AP50, AP75, the small / medium / large bins, AR@1/10/100) on libssdk
(csrc/metrics.hip, ``ssdk_coco_eval``; the rules are restated in include/ssdk.h and DESIGN.md §30).

Not part of the reference, whose only metric is ``mean_average_precision`` (one IoU threshold, VOC integration, a difficult flag).
Predictions and ground truth take the same form as there and may live on the host or on the GPU; they are packed once and
evaluated on the device.  Column 6 of a ground-truth row, when present, marks a crowd region (COCO's ``iscrowd``)."""
import logging

import numpy as np
import torch

from ... import _lib

STAT_NAMES = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')
MAX_PAIRS, MAX_MAX_DETS, MAX_RECALL_THRESHOLDS = 64, 4, 1024   # the kernels' limits (include/ssdk.h)


def default_tables():
    """(iou_thresholds [10], recall_thresholds [101], area_ranges [4, 2], max_detections [3]) -- pycocotools' Params, from the same numpy
    expressions, so that the host and the device hold the same bits."""
    return (np.linspace(.5, .95, 10), np.linspace(0, 1, 101), np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64),
            np.array([1, 10, 100], np.int32))


def check_tables(iou_thresholds, recall_thresholds, area_ranges, max_detections):
    """The four tables as contiguous numpy arrays; ValueError for what the kernels refuse (no GPU needed)."""
    d_iou, d_rec, d_area, d_max = default_tables()
    iou = np.ascontiguousarray(d_iou if iou_thresholds is None else iou_thresholds, np.float64).reshape(-1)
    rec = np.ascontiguousarray(d_rec if recall_thresholds is None else recall_thresholds, np.float64).reshape(-1)
    area = np.ascontiguousarray(d_area if area_ranges is None else area_ranges, np.float64)
    if area.ndim != 2 or area.shape[1] != 2:
        raise ValueError(f'area_ranges: [A, 2] rows of (lo, hi), got shape {area.shape}')
    md64 = np.asarray(d_max if max_detections is None else max_detections).reshape(-1)
    T, R, A, M = iou.size, rec.size, area.shape[0], md64.size
    if min(T, R, A, M) < 1:
        raise ValueError(f'every table needs at least one entry (T={T}, R={R}, A={A}, M={M})')
    if T * A > MAX_PAIRS:
        raise ValueError(f'{T} IoU thresholds x {A} area ranges = {T * A} pairs; the matching kernel holds at most {MAX_PAIRS} (one lane each)')
    if M > MAX_MAX_DETS or R > MAX_RECALL_THRESHOLDS:
        raise ValueError(f'at most {MAX_MAX_DETS} max_detections and {MAX_RECALL_THRESHOLDS} recall thresholds (got {M}, {R})')
    if md64[0] < 1 or np.any(np.diff(md64.astype(np.int64)) <= 0) or md64[-1] >= 2 ** 31:
        raise ValueError(f'max_detections must be positive and ascending, got {md64.tolist()}')
    return iou, rec, area, np.ascontiguousarray(md64, np.int32)


def coco_evaluation(predictions, gts, class_labels, gt_areas=None, image_area_scale=None, iou_thresholds=None, recall_thresholds=None,
                    area_ranges=None, max_detections=(1, 10, 100), verbose=True, details=False):
    """
    Args:
        predictions: torch.tensor(:shape [NumBoxes, 7] ~ {[0] - image_id, [1-4] - corner box, [5] - class, [6] - score})
        gts: list(:len NumImages) ~ torch.tensor(:shape [NumBoxes_i, 6 or 7]); a non-zero column 6 marks a crowd region
        class_labels: dict(:keys ClassId, :values ClassName)
        gt_areas: None (box areas) or list(:len NumImages) ~ tensor [NumBoxes_i] / one tensor [TotalBoxes]: the annotations' areas
        image_area_scale: None or [NumImages]: multiplies every area of that image for the area-range test (normalised boxes)
        iou_thresholds, recall_thresholds, area_ranges, max_detections: the tables; None -> pycocotools' defaults
        verbose: log the twelve lines in pycocotools' wording
        details: also return 'rank', 'flags', 'order' and 'npig' (``ssdk_coco_eval_ex``)
    Returns:
        dict: the twelve statistics by name (python floats), 'precision' [T, R, K, A, M] and 'recall' [T, K, A, M] (host fp64 tensors)
    """
    iou, rec, area, md = check_tables(iou_thresholds, recall_thresholds, area_ranges, max_detections)
    T, R, A, M = iou.size, rec.size, area.shape[0], md.size
    num_classes = max([int(k) for k in class_labels] + [0]) + 1
    lib = _lib.lib()
    device = predictions.device if predictions.is_cuda else torch.device('cuda', torch.cuda.current_device())
    pred = predictions.to(device=device, dtype=torch.float32).contiguous()
    assert pred.dim() == 2 and pred.size(1) == 7, 'predictions: [NumBoxes, 7] = image id, box, class, score'
    stride = int(gts[0].size(1)) if len(gts) else 6
    counts = [int(g.size(0)) for g in gts]
    total = sum(counts)
    rows = torch.cat([g.reshape(-1, stride).to(torch.float32) for g in gts], dim=0).to(device).contiguous() if total else \
        torch.zeros((0, stride), dtype=torch.float32, device=device)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(device)
    areas = None
    if gt_areas is not None:
        flat = torch.cat([torch.as_tensor(x).reshape(-1) for x in gt_areas]) if isinstance(gt_areas, (list, tuple)) else torch.as_tensor(gt_areas).reshape(-1)
        assert flat.numel() == total, f'gt_areas: {flat.numel()} values for {total} ground-truth rows'
        areas = flat.to(device=device, dtype=torch.float64).contiguous()
    scale = None
    if image_area_scale is not None:
        scale = torch.as_tensor(image_area_scale).reshape(-1).to(device=device, dtype=torch.float64).contiguous()
        assert scale.numel() == len(gts), f'image_area_scale: {scale.numel()} values for {len(gts)} images'
    n = pred.size(0)
    d_iou, d_rec, d_area = (torch.from_numpy(x).to(device) for x in (iou, rec, area))
    ws = torch.empty((max(lib.ssdk_coco_eval_workspace_bytes(n, total, num_classes, T, A), 256),), dtype=torch.uint8, device=device)
    precision = torch.empty((T, R, num_classes, A, M), dtype=torch.float64, device=device)
    recall = torch.empty((T, num_classes, A, M), dtype=torch.float64, device=device)
    stats = torch.empty((12,), dtype=torch.float64, device=device)
    head = (_lib.ptr(pred), n, _lib.ptr(rows), stride, _lib.ptr(offs), len(gts), total, num_classes, _lib.ptr(areas), _lib.ptr(scale), _lib.ptr(d_iou), T,
            _lib.ptr(d_rec), R, _lib.ptr(d_area), A, md.ctypes.data, M, _lib.ptr(precision), _lib.ptr(recall), _lib.ptr(stats))
    tail = (_lib.ptr(ws), ws.numel(), _lib.current_stream())
    extra = {}
    if details:
        rank = torch.empty((n,), dtype=torch.int32, device=device)
        flags = torch.empty((n, T * A), dtype=torch.uint8, device=device)
        order = torch.empty((n,), dtype=torch.int32, device=device)     # (uint32 on the device; n < 2^31, so the bits are the int32's)
        npig = torch.empty((num_classes, A), dtype=torch.int32, device=device)
        _lib.check(lib.ssdk_coco_eval_ex(*head, _lib.ptr(rank), _lib.ptr(flags), _lib.ptr(order), _lib.ptr(npig), *tail), 'ssdk_coco_eval_ex')
        extra = dict(rank=rank.cpu(), flags=flags.cpu(), order=order.cpu().to(torch.int64), npig=npig.cpu())
    else:
        _lib.check(lib.ssdk_coco_eval(*head, *tail), 'ssdk_coco_eval')
    values = stats.cpu()
    out = {name: float(values[i]) for i, name in enumerate(STAT_NAMES)}
    out['precision'], out['recall'] = precision.cpu(), recall.cpu()
    out.update(extra)
    if verbose:
        for line in summary_lines(out, iou, area, md):
            logging.info(line)
    return out


def summary_lines(stats, iou_thresholds, area_ranges, max_detections):
    """The twelve lines of COCOeval.summarize, in its wording."""
    iou_all = f'{iou_thresholds[0]:0.2f}:{iou_thresholds[-1]:0.2f}'
    last = len(max_detections) - 1
    spec = [('AP', True, iou_all, 'all', last), ('AP50', True, '0.50', 'all', last), ('AP75', True, '0.75', 'all', last), ('APs', True, iou_all, 'small', last),
            ('APm', True, iou_all, 'medium', last), ('APl', True, iou_all, 'large', last), ('AR1', False, iou_all, 'all', 0), ('AR10', False, iou_all, 'all', 1),
            ('AR100', False, iou_all, 'all', 2), ('ARs', False, iou_all, 'small', last), ('ARm', False, iou_all, 'medium', last),
            ('ARl', False, iou_all, 'large', last)]
    lines = []
    for name, is_ap, iou, area, m in spec:
        title, kind = ('Average Precision', '(AP)') if is_ap else ('Average Recall', '(AR)')
        dets = int(max_detections[m]) if m < len(max_detections) else -1
        lines.append(f' {title:<18} {kind} @[ IoU={iou:<9} | area={area:>6s} | maxDets={dets:>3d} ] = {stats[name]:0.3f}')
    return lines


def coco_average_precision(predictions, gts, class_labels, **kw):
    """AP@[.50:.95] as a python float: an entry for the evaluator's ``metrics`` dict (same leading arguments as mean_average_precision)."""
    kw.setdefault('verbose', False)
    return coco_evaluation(predictions, gts, class_labels, **kw)['AP']
