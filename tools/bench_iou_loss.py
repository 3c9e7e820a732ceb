#!/usr/bin/env python3
"""Time the box term of the fused loss per kind (SmoothL1, GIoU and the IoU, DIoU, CIoU, EIoU kinds of csrc/iou_loss.h) through the C ABI,
forward and backward separately, and the row-wise pair ``ssdk_box_iou_loss_fwd`` / ``_bwd`` against the same formula in stock PyTorch:

  sampled   ssdk_multibox_loss_fwd / _bwd_ex at SSD-300 geometry (8 732 anchors), 81 classes, batch 64, CrossEntropyLoss under hard-negative
            mining (ratio 3; the mask and the sampler's log-sum-exp are made once, outside the timing): DESIGN.md §11.10's workload
  dense     the same two calls at RetinaNet-500 geometry (47 961 anchors), 80 classes, batch 32, ATSS targets, Quality Focal Loss with
            sampled = NULL (the dense kernels; q from the IoU)
  rows      the row-wise pair at 10^6 boxes, against torch ops with autograd (torch.autograd.grad, retain_graph) on the same tensors

Device events around --inner back-to-back calls, queued behind ~1 ms of device spin so that the host is ahead of the GPU.  After a warm-up
the arms (the kinds; for ``rows`` ssdk, stock and ssdk again) alternate within the process over --rounds rounds of --reps timings; --inner
is raised until every arm's timed calls fill --seconds.  Reported per arm and direction: the median of the round medians, and its
difference to the GIoU arm (``rows``: stock over ssdk, with the A/A' spread of the two ssdk arms beside it).

Usage:  python tools/bench_iou_loss.py [--rounds 5] [--reps 5] [--seconds 0.3] [--out FILE.txt]
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
from single_shot_detection_amd.detection.target_assigner import AtssTargetAssigner, TargetAssigner  # noqa: E402

XY_SCALE, WH_SCALE, EPS = 10.0, 5.0, 1e-8
LOC = {'smooth_l1': 0, 'giou': 1, 'iou': 8, 'diou': 9, 'ciou': 10, 'eiou': 11}
IOU_EPS = 1e-7


def loss_calls(config, batch, C, dense, dev):
    """{kind: (fwd, bwd)} on one set of tensors, and the shape's figures."""
    lib = _lib.lib()
    cfg = syn.CONFIGS[config]
    anchors = torch.from_numpy(np.load(os.path.join(REPO, 'tests', 'golden', f'{config}.npz'))['anchors']).to(dev)
    A = anchors.shape[0]
    gt = [torch.from_numpy(g) for g in syn.make_ground_truth(batch, cfg['size'], C if dense else C - 1, seed=1, background=False)]
    if dense:
        levels = tuple(h * h * nb for _, h, nb in cfg['levels'])
        raw = AtssTargetAssigner(9).encode_ground_truth(gt, anchors, level_sizes=levels)
    else:
        raw = TargetAssigner(0.5, 0.5).encode_ground_truth(gt, anchors)
    cls = raw[..., 4]
    positive = (cls != 0) & (cls != -1)
    wh = raw[..., 2:4] - raw[..., 0:2]
    enc = torch.cat([(raw[..., 0:2] + wh / 2 - anchors[:, :2]) / anchors[:, 2:] * XY_SCALE, torch.log(wh / anchors[:, 2:] + EPS) * WH_SCALE], -1)
    gen = torch.Generator(device=dev).manual_seed(2)
    noise = torch.randn((batch, A, 4), device=dev, generator=gen) * torch.tensor([2.0, 2.0, 1.0, 1.0], device=dev)
    locs = torch.where(positive.unsqueeze(-1), enc + noise, noise).reshape(batch, A * 4).contiguous()
    scores = torch.randn((batch, A * C), device=dev, generator=gen) * 2.0
    ws = torch.empty((lib.ssdk_multibox_loss_workspace_bytes(batch, A, C),), dtype=torch.uint8, device=dev)
    mask = None
    if not dense:
        mask = torch.empty((batch, A), dtype=torch.uint8, device=dev)
        _lib.check(lib.ssdk_hard_negative_mining(_lib.ptr(scores), cls.data_ptr(), 6, batch, A, C, 3.0, 0, _lib.ptr(mask), _lib.ptr(ws), ws.numel(),
                                                 _lib.current_stream()), 'ssdk_hard_negative_mining')
    out3, grad = torch.empty((3,), device=dev), torch.ones((1,), device=dev)
    dscores, dlocs = torch.empty_like(scores), torch.empty_like(locs)
    row_mask = None if dense else torch.empty((batch, A), dtype=torch.uint8, device=dev)
    calls = {}
    for kind, code in LOC.items():
        params = _lib.LossParams(5 if dense else 0, code, 2.0, 0.25, 0, 0.0, 1.0, 1.0, XY_SCALE, WH_SCALE, EPS, 1.0, 0.0, None, 1 if dense else 0)
        target = raw.clone()    # (SmoothL1 encodes its own copy in place, once: the later forwards re-encode encoded rows, at the same cost)

        def fwd(params=params, target=target):
            _lib.check(lib.ssdk_multibox_loss_fwd(ctypes.byref(params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target),
                                                  _lib.ptr(mask), batch, A, C, 0 if dense else 1, _lib.ptr(out3), _lib.ptr(ws), ws.numel(),
                                                  _lib.current_stream()), 'ssdk_multibox_loss_fwd')

        def bwd(params=params, target=target):
            _lib.check(lib.ssdk_multibox_loss_bwd_ex(ctypes.byref(params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target),
                                                     _lib.ptr(mask), _lib.ptr(grad), 1, batch, A, C, _lib.ptr(dscores), _lib.ptr(dlocs),
                                                     _lib.ptr(row_mask), _lib.ptr(ws), ws.numel(), _lib.current_stream()), 'ssdk_multibox_loss_bwd')
        fwd.keep = (params, target)
        calls[kind] = (fwd, bwd)
    shape = dict(workload='dense' if dense else 'sampled', config=config, batch=batch, anchors=A, classes=C, positives=int(positive.sum()),
                 rows=batch * A, ssdk_version=lib.ssdk_version())
    return calls, shape


def torch_iou_loss(p, t, kind):
    """The kind's per-row value in torch ops (include/ssdk.h's definitions)."""
    area = lambda b: (b[:, 2] - b[:, 0]).clamp(min=0) * (b[:, 3] - b[:, 1]).clamp(min=0)   # noqa: E731
    inter = area(torch.cat([torch.max(p[:, :2], t[:, :2]), torch.min(p[:, 2:], t[:, 2:])], -1))
    union = area(p) + area(t) - inter
    iou = inter / union
    cw, ch = torch.max(p[:, 2], t[:, 2]) - torch.min(p[:, 0], t[:, 0]), torch.max(p[:, 3], t[:, 3]) - torch.min(p[:, 1], t[:, 1])
    if kind == 'giou':
        enc = cw.clamp(min=0) * ch.clamp(min=0)
        return 1.0 - (iou - (enc - union) / enc)
    if kind == 'iou':
        return 1.0 - iou
    c2 = cw * cw + ch * ch + IOU_EPS
    dx, dy = (p[:, 0] + p[:, 2] - t[:, 0] - t[:, 2]) / 2, (p[:, 1] + p[:, 3] - t[:, 1] - t[:, 3]) / 2
    diou = 1.0 - iou + (dx * dx + dy * dy) / c2
    w, h, wg, hg = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1], t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
    if kind == 'diou':
        return diou
    if kind == 'ciou':
        v = (4.0 / math.pi ** 2) * (torch.atan(wg / hg) - torch.atan(w / h)) ** 2
        with torch.no_grad():
            alpha = v / (1.0 - iou + v + IOU_EPS)
        return diou + alpha * v
    return diou + (w - wg) ** 2 / (cw * cw + IOU_EPS) + (h - hg) ** 2 / (ch * ch + IOU_EPS)


def row_calls(kind, n, dev):
    """{arm: (fwd, bwd)} of the row-wise pair for one kind: ssdk, stock torch, ssdk again; and how far the two agree."""
    lib = _lib.lib()
    gen = torch.Generator(device=dev).manual_seed(3)
    wh = torch.rand((n, 2), device=dev, generator=gen) * 156.0 + 24.0
    xy = torch.rand((n, 2), device=dev, generator=gen) * (300.0 - wh)
    t = torch.cat([xy, xy + wh], -1)
    c = (t[:, :2] + t[:, 2:]) / 2 + (torch.rand((n, 2), device=dev, generator=gen) - 0.5) * wh
    pwh = wh * torch.exp((torch.rand((n, 2), device=dev, generator=gen) - 0.5) * 1.4)
    p = torch.cat([c - pwh / 2, c + pwh / 2], -1).contiguous()
    g = torch.rand((n,), device=dev, generator=gen) + 0.5
    out, dp = torch.empty((n,), device=dev), torch.empty((n, 4), device=dev)
    code = LOC[kind]

    def ssdk_fwd():
        _lib.check(lib.ssdk_box_iou_loss_fwd(code, _lib.ptr(p), _lib.ptr(t), n, _lib.ptr(out), _lib.current_stream()), 'ssdk_box_iou_loss_fwd')

    def ssdk_bwd():
        _lib.check(lib.ssdk_box_iou_loss_bwd(code, _lib.ptr(p), _lib.ptr(t), _lib.ptr(g), n, _lib.ptr(dp), _lib.current_stream()), 'ssdk_box_iou_loss_bwd')
    x = p.clone().requires_grad_(True)
    state = {}

    def stock_fwd():
        state['out'] = torch_iou_loss(x, t, kind)

    def stock_bwd():
        state['dx'] = torch.autograd.grad(state['out'], x, g, retain_graph=True)[0]
    for fn in (ssdk_fwd, ssdk_bwd, stock_fwd, stock_bwd):
        fn()
    torch.cuda.synchronize()
    agree = {'values_max_abs': float((state['out'].detach() - out).abs().max()), 'grad_max_abs': float((state['dx'] - dp).abs().max())}
    ssdk_fwd.keep = (p, t, g, out, dp, x, state)
    return {'ssdk': (ssdk_fwd, ssdk_bwd), 'stock': (stock_fwd, stock_bwd), 'ssdk2': (ssdk_fwd, ssdk_bwd)}, agree


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


def measure(fns, args):
    """{arm: median of the round medians in us}, the rounds, and the inner count, for arms that alternate."""
    warm = {arm: time_us(fn, args.inner, 2) for arm, fn in fns.items()}
    inner = max(args.inner, math.ceil(1.15 * args.seconds * 1e6 / (min(warm.values()) * args.rounds * args.reps)))
    rounds = {arm: [] for arm in fns}
    for _ in range(args.rounds):
        for arm, fn in fns.items():
            rounds[arm].append(time_us(fn, inner, args.reps))
    return {arm: statistics.median(r) for arm, r in rounds.items()}, rounds, inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=5, help='calls per timing, at least; raised to fill --seconds')
    ap.add_argument('--seconds', type=float, default=0.3, help='timed device work per arm and direction, at least')
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_iou_loss.py needs a GPU: there is nothing to time without one')
    dev = torch.device('cuda:0')
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
    for config, batch, C, dense in (('ssd_300_vgg16_voc', 64, 81, False), ('retina_rn50_500_coco', 32, 80, True)):
        calls, shape = loss_calls(config, batch, C, dense, dev)
        for k, direction in enumerate(('fwd', 'bwd')):
            med, rounds, inner = measure({kind: pair[k] for kind, pair in calls.items()}, args)
            emit(dict(shape, direction=direction, us={a: round(x, 2) for a, x in med.items()}, inner=inner, reps_per_round=args.reps,
                      minus_giou_us={a: round(x - med['giou'], 2) for a, x in med.items()},
                      round_medians_us={a: [round(x, 2) for x in r] for a, r in rounds.items()}))
        del calls
    for kind in ('giou', 'iou', 'diou', 'ciou', 'eiou'):
        calls, agree = row_calls(kind, args.rows, dev)
        for k, direction in enumerate(('fwd', 'bwd')):
            med, rounds, inner = measure({arm: pair[k] for arm, pair in calls.items()}, args)
            base = (med['ssdk'] + med['ssdk2']) / 2
            emit(dict(workload='rows', kind=kind, rows=args.rows, direction=direction, us={a: round(x, 2) for a, x in med.items()}, inner=inner,
                      reps_per_round=args.reps, stock_over_ssdk=round(med['stock'] / base, 2), aa_spread=round(abs(med['ssdk'] - med['ssdk2']) / base, 3),
                      stock_vs_ssdk=agree, round_medians_us={a: [round(x, 2) for x in r] for a, r in rounds.items()}))
        del calls
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.writelines(json.dumps(line) + '\n' for line in lines)


if __name__ == '__main__':
    main()
