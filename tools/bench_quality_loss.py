#!/usr/bin/env python3
"""Time the multibox loss calls alone (``ssdk_multibox_loss_fwd`` / ``ssdk_multibox_loss_bwd_ex``, csrc/loss.hip) through the C ABI when
every anchor that is not ignored is sampled, at RetinaNet-500 geometry (47 961 anchors, batch 32, 80 classes, synthetic.make_ground_truth's
default 1..8 boxes per image, TargetAssigner(0.5, 0.4) targets, GIoU box term), forward and backward separately:

  a   SigmoidFocalLoss through loss_fwd_kernel / loss_bwd_kernel with an explicit all-valid mask (what a custom sampler gets)
  b   SigmoidFocalLoss on the dense kernels (sampled = NULL)
  c   Quality Focal Loss, dense, quality_from_iou = 1
  d   Varifocal Loss, dense, quality_from_iou = 1
  a2  a again: the A/A' control

and, as a second table (--hnm), c and d under a hard_negative_mining mask (ratio 3, at least 5 per image).

Device events around --inner back-to-back calls, queued behind ~1 ms of device spin so that the host is ahead of the GPU.  After a warm-up
the arms alternate within the process over --rounds rounds of --reps timings; --inner is raised until every arm's timed calls fill
--seconds.  Per direction: the median of the round medians of each arm, each arm over the mean of a and a2, and the A/A' spread
|a - a2| / mean beside it -- a ratio inside that spread says nothing.  The floors are computed from the shapes at 6.0 TB/s (an in-order HBM
sweep): the forward reads the scores once, the backward reads them and writes dscores.  They are not measured.

--arms a a2 runs on a library that predates the dense kernels as well (SSDK_LIB=<that build>).

Usage:  python tools/bench_quality_loss.py [--rounds 5] [--reps 5] [--seconds 0.5] [--hnm] [--out FILE.txt]
        python tools/bench_quality_loss.py --rounds 1 --reps 2 --seconds 0      (a short run, e.g. under rocprofv3 --kernel-trace --stats)
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
from single_shot_detection_amd.detection import sampler                                            # noqa: E402
from single_shot_detection_amd.detection.target_assigner import TargetAssigner                     # noqa: E402

CONFIG, BATCH = 'retina_rn50_500_coco', 32
HBM_BYTES_PER_US = 6.0e6          # 6.0 TB/s
FOCAL, QFL, VFL, GIOU = 1, 5, 6, 1
ARMS = {'a': (FOCAL, 'mask'), 'b': (FOCAL, None), 'c': (QFL, None), 'd': (VFL, None), 'a2': (FOCAL, 'mask')}
HNM_ARMS = {'c_hnm': (QFL, 'hnm'), 'd_hnm': (VFL, 'hnm')}


def make_calls(arms, dev):
    cfg = syn.CONFIGS[CONFIG]
    anchors = torch.from_numpy(np.load(os.path.join(REPO, 'tests', 'golden', f'{CONFIG}.npz'))['anchors']).to(dev)
    A, C = anchors.shape[0], cfg['num_classes']
    gt = syn.make_ground_truth(BATCH, cfg['size'], C, seed=1, background=False)
    target = TargetAssigner(0.5, 0.4).encode_ground_truth([torch.from_numpy(g) for g in gt], anchors)
    scores = torch.from_numpy(syn.make_logits(BATCH, A, C, seed=2)).to(dev)
    locs = torch.from_numpy(syn.make_locs(BATCH, A, seed=3, scale=0.5)).to(dev)
    lib = _lib.lib()
    ws = sampler.loss_workspace(BATCH, A, C, dev)
    cls = target[..., 4]
    masks = {'mask': (cls != -1).to(torch.uint8).contiguous(), None: None}
    if any(m == 'hnm' for _, m in arms.values()):
        masks['hnm'] = sampler.hard_negative_mining(scores, cls, 3, 5).to(torch.uint8).contiguous()
    out3 = torch.empty((3,), device=dev)
    grad = torch.ones((1,), device=dev)
    dscores, dlocs = torch.empty_like(scores), torch.empty_like(locs)
    keep = (anchors, target, scores, locs, ws, masks, out3, grad, dscores, dlocs)

    def pair(kind, mask):
        quality = 1 if kind in (QFL, VFL) else 0
        fields = [kind, GIOU, 2.0, 0.75 if kind == VFL else 0.25, 0, 0.0, 1.0, 1.0, 10.0, 5.0, 1e-8, 1.0, 0.0, None]
        if quality:
            fields.append(quality)      # (a library that predates the field never sees these kinds)
        params = _lib.LossParams(*fields)
        m = masks[mask]

        def fwd():
            _lib.check(lib.ssdk_multibox_loss_fwd(ctypes.byref(params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target), _lib.ptr(m),
                                                  BATCH, A, C, 0, _lib.ptr(out3), _lib.ptr(ws), ws.numel(), _lib.current_stream()), 'ssdk_multibox_loss_fwd')

        def bwd():
            _lib.check(lib.ssdk_multibox_loss_bwd_ex(ctypes.byref(params), _lib.ptr(scores), _lib.ptr(locs), _lib.ptr(anchors), _lib.ptr(target),
                                                     _lib.ptr(m), _lib.ptr(grad), 1, BATCH, A, C, _lib.ptr(dscores), _lib.ptr(dlocs), None, _lib.ptr(ws),
                                                     ws.numel(), _lib.current_stream()), 'ssdk_multibox_loss_bwd_ex')
        fwd.keep = bwd.keep = (params, keep)
        fwd()        # (the backward reads the forward's state -- divider, q -- from the workspace; every arm leaves the same counts there)
        return fwd, bwd
    calls = {arm: pair(*spec) for arm, spec in arms.items()}
    score_bytes = BATCH * A * C * 4
    shape = {'anchors': A, 'batch': BATCH, 'classes': C, 'boxes': int(sum(len(g) for g in gt)), 'rows_sampled': int(masks['mask'].sum()),
             'rows_sampled_hnm': int(masks['hnm'].sum()) if 'hnm' in masks else None, 'positives': int((cls > 0).sum()),
             'score_bytes': score_bytes, 'floor_fwd_us': round(score_bytes / HBM_BYTES_PER_US, 1), 'floor_bwd_us': round(2 * score_bytes / HBM_BYTES_PER_US, 1),
             'floors': 'computed from the shapes at 6.0 TB/s, not measured', 'ssdk_version': lib.ssdk_version()}
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=5, help='calls per timing, at least; raised to fill --seconds')
    ap.add_argument('--seconds', type=float, default=0.5, help='timed device work per arm and direction, at least')
    ap.add_argument('--arms', nargs='+', default=list(ARMS), choices=list(ARMS))
    ap.add_argument('--hnm', action='store_true', help='also the second table: c and d under a hard_negative_mining mask')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_quality_loss.py needs a GPU: there is nothing to time without one')
    dev = torch.device('cuda:0')
    arms = {arm: ARMS[arm] for arm in args.arms}
    if args.hnm:
        arms.update(HNM_ARMS)
    calls, shape = make_calls(arms, dev)
    lines = []
    for k, direction in enumerate(('fwd', 'bwd')):
        fns = {arm: pair[k] for arm, pair in calls.items()}
        warm = {arm: time_us(fn, args.inner, 2) for arm, fn in fns.items()}
        inner = max(args.inner, math.ceil(1.15 * args.seconds * 1e6 / (min(warm.values()) * args.rounds * args.reps)))
        rounds = {arm: [] for arm in fns}
        for _ in range(args.rounds):
            for arm, fn in fns.items():
                rounds[arm].append(time_us(fn, inner, args.reps))
        med = {arm: statistics.median(r) for arm, r in rounds.items()}
        line = dict(shape, direction=direction, us={arm: round(v, 2) for arm, v in med.items()}, inner=inner, reps_per_round=args.reps,
                    round_medians_us={arm: [round(x, 2) for x in r] for arm, r in rounds.items()})
        if 'a' in med and 'a2' in med:
            base = (med['a'] + med['a2']) / 2
            line['over_a'] = {arm: round(v / base, 3) for arm, v in med.items()}
            line['aa_spread'] = round(abs(med['a'] - med['a2']) / base, 3)
        floor = shape['floor_fwd_us'] if direction == 'fwd' else shape['floor_bwd_us']
        line['over_floor'] = {arm: round(v / floor, 2) for arm, v in med.items()}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.writelines(json.dumps(line) + '\n' for line in lines)


if __name__ == '__main__':
    main()
