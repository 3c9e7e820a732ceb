#!/usr/bin/env python3
"""Time the SimOTA encode call alone (``ssdk_encode_ground_truth_simota``: simota_class_sum_kernel + simota_candidates_kernel +
simota_assign_kernel, csrc/match.hip) against the task-aligned call (``ssdk_encode_ground_truth_tal``, the yardstick for this class of
work) and against a stock-PyTorch dense ``[G, A]`` restatement of the rule, on the same inputs, the library calls through the C ABI on
ground truth that is already packed on the device, at RetinaNet-500 geometry (47 961 anchors in five levels, batch 32, 80 logit columns):

  retina500_b32_default_g   synthetic.make_ground_truth's default 1..8 boxes per image (142 boxes)
  retina500_b32_g32         32 boxes per image (1 024 boxes)

The predictions are drawn on the device from a fixed seed: logits 2 * N(0, 1) - 2, locs N(0, 1) * (1.5, 1.5, 1, 1).  Device events around
--inner back-to-back calls, queued behind ~1 ms of device spin so that the host is ahead of the GPU.  After a warm-up four arms alternate
within the process -- TAL (A), SimOTA, the dense restatement, TAL again (A') -- over --rounds rounds of --reps timings; --inner is raised
until the library arms' timed calls fill --seconds (the dense arm, an image at a time in some forty stock launches each, runs --inner / 8
calls).  Per case: the median of the round medians of each arm, SimOTA over the mean of A and A' and the dense form over SimOTA, and the
A/A' spread |A - A'| / mean beside them -- a ratio inside that spread says nothing.  The dense form is a yardstick for time, not a
reference for bits (it sorts with torch.topk and adds 1e5 to a penalised cost as YOLOX does); the count of anchors on which it and the
library disagree is printed.  The bytes the shapes imply per launch are computed beside the times; the time per launch comes from a
``rocprofv3 --kernel-trace --stats`` run of the short form below.

Usage:  python tools/bench_simota.py [--rounds 5] [--reps 7] [--seconds 1.0] [--out FILE.txt]
        python tools/bench_simota.py --rounds 1 --reps 2 --seconds 0 --no-dense      (a short run, e.g. under rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from single_shot_detection_amd import _lib, synthetic as syn                                       # noqa: E402
from single_shot_detection_amd.detection.target_assigner import pack_ground_truth                  # noqa: E402

CONFIG, BATCH, COLUMNS = 'retina_rn50_500_coco', 32, 80
XY_SCALE, WH_SCALE = 10.0, 5.0
CASES = {
    'retina500_b32_default_g': dict(seed=1),
    'retina500_b32_g32': dict(seed=1, fixed_g=32),
}


def regions(b, anchors, radii):
    """(in_box, in_centre) bool [G, A] of one image's boxes b [G, 6]."""
    cx, cy = anchors[:, 0][None], anchors[:, 1][None]
    in_box = (b[:, 0:1] < cx) & (cx < b[:, 2:3]) & (b[:, 1:2] < cy) & (cy < b[:, 3:4])
    gcx, gcy = (b[:, 0:1] + b[:, 2:3]) * 0.5, (b[:, 1:2] + b[:, 3:4]) * 0.5
    rx, ry = radii[:, 0][None], radii[:, 1][None]
    in_centre = (gcx - rx < cx) & (cx < gcx + rx) & (gcy - ry < cy) & (cy < gcy + ry)
    return in_box, in_centre


def dense_image(b, anchors, radii, scores, locs, q, iou_weight):
    """box_idx int64 [A] of one image from stock ops on [G, A] tensors: the rule as YOLOX writes it."""
    A = anchors.shape[0]
    if b.shape[0] == 0:
        return torch.full((A,), -2, dtype=torch.int64, device=anchors.device)
    cx = anchors[:, 0] + anchors[:, 2] * locs[:, 0] / XY_SCALE
    cy = anchors[:, 1] + anchors[:, 3] * locs[:, 1] / XY_SCALE
    w, h = anchors[:, 2] * torch.exp(locs[:, 2] / WH_SCALE), anchors[:, 3] * torch.exp(locs[:, 3] / WH_SCALE)
    px1, py1, px2, py2 = (cx - w / 2)[None], (cy - h / 2)[None], (cx + w / 2)[None], (cy + h / 2)[None]
    iw = (torch.minimum(px2, b[:, 2:3]) - torch.maximum(px1, b[:, 0:1])).clamp(min=0)
    ih = (torch.minimum(py2, b[:, 3:4]) - torch.maximum(py1, b[:, 1:2])).clamp(min=0)
    inter = iw * ih
    union = (w * h)[None] + ((b[:, 2] - b[:, 0]).clamp(min=0) * (b[:, 3] - b[:, 1]).clamp(min=0))[:, None] - inter
    u = torch.where(union > 0, inter / union, torch.zeros_like(inter)).clamp(0, 1)
    in_box, in_centre = regions(b, anchors, radii)
    region = in_box | in_centre
    S = torch.nn.functional.softplus(scores).sum(dim=1)
    cls = S[None] - scores[:, (b[:, 4].long() - 1).clamp(0, scores.shape[1] - 1)].t()
    cost = cls + iou_weight * -torch.log(u + 1e-8) + 1e5 * (~(in_box & in_centre)).float()
    cost = torch.where(region, cost, torch.full_like(cost, float('inf')))
    n = region.sum(dim=1)
    topq = torch.topk(u * region.float(), min(q, A), dim=1).values.sum(dim=1)
    k = torch.minimum(topq.int().clamp(min=1), n.clamp(max=q).int())
    order = torch.topk(cost, min(q, A), dim=1, largest=False)
    keep = torch.arange(order.indices.shape[1], device=b.device)[None] < k[:, None]
    matching = torch.zeros_like(region)
    matching.scatter_(1, order.indices, keep)
    cost = torch.where(matching, cost, torch.full_like(cost, float('inf')))
    best, who = cost.min(dim=0)
    return torch.where(torch.isfinite(best), who, torch.full_like(who, -2))


def make_calls(case, args, dev):
    cfg = syn.CONFIGS[CONFIG]
    anchors = torch.from_numpy(np.load(os.path.join(REPO, 'tests', 'golden', f'{CONFIG}.npz'))['anchors']).to(dev)
    sizes = [h * h * nb for _, h, nb in cfg['levels']]
    strides = [float(cfg['size']) / float(h) for _, h, _ in cfg['levels']]
    gt = syn.make_ground_truth(BATCH, cfg['size'], COLUMNS + 1, **CASES[case])
    rows, offs, total = pack_ground_truth([torch.from_numpy(g) for g in gt], dev)
    boxes = [torch.from_numpy(g).to(dev) for g in gt]
    A = anchors.shape[0]
    assert sum(sizes) == A
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    scores = torch.randn((BATCH, A, COLUMNS), generator=gen, device=dev) * 2.0 - 2.0
    locs = torch.randn((BATCH, A, 4), generator=gen, device=dev) * torch.tensor([1.5, 1.5, 1.0, 1.0], device=dev)
    radii = torch.cat([torch.full((n, 2), np.float32(args.center_radius) * np.float32(s), device=dev) for n, s in zip(sizes, strides)])
    lib = _lib.lib()
    target = torch.empty((BATCH, A, 6), dtype=torch.float32, device=dev)
    box_idx = torch.empty((BATCH, A), dtype=torch.int32, device=dev)
    levels = (ctypes.c_int32 * len(sizes))(*sizes)
    level_strides = (ctypes.c_float * (2 * len(sizes)))(*[s for s in strides for _ in range(2)])
    ws_t = torch.empty((max(lib.ssdk_encode_ground_truth_tal_workspace_bytes(BATCH, total, args.tal_topk), 4096),), dtype=torch.uint8, device=dev)
    ws_s = torch.empty((max(lib.ssdk_encode_ground_truth_simota_workspace_bytes(BATCH, total, A, len(sizes)), 4096),), dtype=torch.uint8, device=dev)

    def tal():
        _lib.check(lib.ssdk_encode_ground_truth_tal(_lib.ptr(rows), 6, _lib.ptr(offs), BATCH, total, _lib.ptr(anchors), A, _lib.ptr(scores), COLUMNS,
                                                    _lib.ptr(locs), XY_SCALE, WH_SCALE, args.tal_topk, 1.0, 6.0, _lib.ptr(target), None, _lib.ptr(ws_t),
                                                    ws_t.numel(), _lib.current_stream()), 'ssdk_encode_ground_truth_tal')

    def simota():
        _lib.check(lib.ssdk_encode_ground_truth_simota(_lib.ptr(rows), 6, _lib.ptr(offs), BATCH, total, _lib.ptr(anchors), A, levels, level_strides,
                                                       len(sizes), _lib.ptr(scores), COLUMNS, _lib.ptr(locs), XY_SCALE, WH_SCALE, args.center_radius,
                                                       args.candidate_topk, args.iou_weight, _lib.ptr(target), _lib.ptr(box_idx), None,
                                                       _lib.ptr(ws_s), ws_s.numel(), _lib.current_stream()), 'ssdk_encode_ground_truth_simota')

    def dense():
        return torch.stack([dense_image(boxes[i], anchors, radii, scores[i], locs[i], args.candidate_topk, args.iou_weight) for i in range(BATCH)])
    tal.keep = simota.keep = dense.keep = (anchors, rows, offs, target, box_idx, ws_t, ws_s, levels, level_strides, scores, locs, radii, boxes)
    # the (box, anchor) pairs of the regions -- the only ones whose loc, class sum and logit launch 2 loads -- and the anchors in any region
    pairs, inside, region_anchors = 0, 0, 0
    for b in boxes:
        in_box, in_centre = regions(b, anchors, radii)
        pairs += int((in_box | in_centre).sum())
        inside += int(in_box.sum())
        region_anchors += int((in_box | in_centre).any(dim=0).sum())
    simota()
    torch.cuda.synchronize()
    shape = {'anchors': A, 'levels': sizes, 'level_strides': [round(s, 3) for s in strides], 'batch': BATCH, 'columns': COLUMNS, 'boxes': total,
             'center_radius': args.center_radius, 'candidate_topk': args.candidate_topk, 'iou_weight': args.iou_weight, 'tal_topk': args.tal_topk,
             'region_pairs': pairs, 'inside_pairs': inside, 'region_anchors': region_anchors, 'positives': int((box_idx >= 0).sum()),
             'class_sum_launch_anchor_bytes': BATCH * A * 16, 'class_sum_launch_logit_bytes': region_anchors * COLUMNS * 4,
             'class_sum_launch_bytes_written': region_anchors * 4,
             'candidate_launch_anchor_bytes': total * A * 16, 'candidate_launch_loc_bytes': pairs * 16, 'candidate_launch_logit_bytes': pairs * 4,
             'candidate_launch_class_sum_bytes': pairs * 4,
             'assign_launch_anchor_bytes': BATCH * A * 16, 'assign_launch_loc_bytes': BATCH * A * 16, 'assign_launch_logit_bytes': pairs * 4,
             'assign_launch_class_sum_bytes': region_anchors * 4, 'target_bytes_written': BATCH * A * 24 + BATCH * A * 4}
    if not args.no_dense:
        shape['dense_disagrees_on_anchors'] = int((dense() != box_idx.long()).sum())
    calls = {'tal_a': tal, 'simota': simota, 'dense': dense, 'tal_b': tal}
    if args.no_dense:
        del calls['dense']
    return calls, shape


def time_us(call, inner, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(2_000_000)
        e0.record()
        for _ in range(inner):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20, help='calls per timing, at least; raised to fill --seconds')
    ap.add_argument('--seconds', type=float, default=1.0, help='timed device work per library arm, at least')
    ap.add_argument('--center-radius', type=float, default=2.5)
    ap.add_argument('--candidate-topk', type=int, default=10)
    ap.add_argument('--iou-weight', type=float, default=3.0)
    ap.add_argument('--tal-topk', type=int, default=13)
    ap.add_argument('--no-dense', action='store_true', help='leave the stock-PyTorch arm out (a kernel trace of the library calls alone)')
    ap.add_argument('--cases', nargs='+', default=list(CASES), choices=list(CASES))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_simota.py needs a GPU: there is nothing to time without one')
    dev = torch.device('cuda:0')
    lines = []
    for case in args.cases:
        calls, shape = make_calls(case, args, dev)
        inner_of = lambda arm, inner: max(2, inner // 8) if arm == 'dense' else inner                         # noqa: E731
        warm = {arm: time_us(call, inner_of(arm, args.inner), 2) for arm, call in calls.items()}   # warm-up, and the call time that sizes --inner
        fastest = min(v for arm, v in warm.items() if arm != 'dense')
        inner = max(args.inner, math.ceil(1.15 * args.seconds * 1e6 / (fastest * args.rounds * args.reps)))   # (warm-up calls run a little slow)
        rounds = {arm: [] for arm in calls}
        for _ in range(args.rounds):
            for arm, call in calls.items():
                rounds[arm].append(time_us(call, inner_of(arm, inner), args.reps))
        med = {arm: statistics.median(r) for arm, r in rounds.items()}
        base = (med['tal_a'] + med['tal_b']) / 2
        line = dict(shape, case=case, simota_us=round(med['simota'], 2), tal_a_us=round(med['tal_a'], 2), tal_b_us=round(med['tal_b'], 2),
                    simota_over_tal=round(med['simota'] / base, 3), aa_spread=round(abs(med['tal_a'] - med['tal_b']) / base, 3),
                    round_medians_us={arm: [round(x, 2) for x in r] for arm, r in rounds.items()}, inner=inner, reps_per_round=args.reps)
        if 'dense' in med:
            line.update(dense_us=round(med['dense'], 2), dense_over_simota=round(med['dense'] / med['simota'], 2))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.writelines(json.dumps(line) + '\n' for line in lines)


if __name__ == '__main__':
    main()
