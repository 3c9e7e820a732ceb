#!/usr/bin/env python3
"""Time the integral box head with its Distribution Focal Loss alone (``ssdk_integral_fwd`` / ``ssdk_integral_bwd``, csrc/integral.hip)
through the C ABI at RetinaNet-500 geometry (47 961 anchors, batch 32, reg_max 16: 417 MB of loc logits, synthetic.make_ground_truth's
default 1..8 boxes per image, TargetAssigner(0.5, 0.4) targets), forward and backward separately, against stock PyTorch on the same tensors:

  ssdk    the two entry points (forward: integral + DFL + positive count + finalize; backward: one launch, dlocs and the DFL scalar)
  stock   softmax, product with the grid, sum, a gather of the positives, bf.modules.losses.DistributionFocalLoss (two F.cross_entropy),
          and torch.autograd.grad for the backward (retain_graph; the target positions y are prepared outside the timing)
  ssdk2   ssdk again: the A/A' control

Device events around --inner back-to-back calls, queued behind ~1 ms of device spin so that the host is ahead of the GPU.  After a warm-up
the arms alternate within the process over --rounds rounds of --reps timings; --inner is raised until every arm's timed calls fill
--seconds.  Per direction: the median of the round medians of each arm, each arm over the mean of ssdk and ssdk2, and the A/A' spread
|ssdk - ssdk2| / mean beside it -- a ratio inside that spread says nothing.  The floors are computed from the shapes at 6.0 TB/s (an in-order
HBM sweep): the forward reads the logits once and writes locs, the backward writes dlogits once and reads dlocs.  They are not measured.

Usage:  python tools/bench_dfl.py [--batch 32] [--rounds 5] [--reps 5] [--seconds 0.5] [--out FILE.txt]
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
from single_shot_detection_amd.bf.modules.losses import DistributionFocalLoss                      # noqa: E402
from single_shot_detection_amd.detection.target_assigner import TargetAssigner                     # noqa: E402

CONFIG = 'retina_rn50_500_coco'
HBM_BYTES_PER_US = 6.0e6          # 6.0 TB/s
REG_MAX, LIMIT, XY_SCALE, WH_SCALE, EPS, WEIGHT = 16, 8.0, 10.0, 5.0, 1e-8, 0.25


def make_calls(batch, dev):
    cfg = syn.CONFIGS[CONFIG]
    bins = REG_MAX + 1
    anchors = torch.from_numpy(np.load(os.path.join(REPO, 'tests', 'golden', f'{CONFIG}.npz'))['anchors']).to(dev)
    A = anchors.shape[0]
    gt = syn.make_ground_truth(batch, cfg['size'], cfg['num_classes'], seed=1, background=False)
    target = TargetAssigner(0.5, 0.4).encode_ground_truth([torch.from_numpy(g) for g in gt], anchors)
    cls = target[..., 4]
    positive = (cls != 0) & (cls != -1)
    # the positives' target positions in bin units (box_coder.py:22-30 on the raw corners), for the logits' peaks and for the stock arm
    wh = target[..., 2:4] - target[..., 0:2]
    cxy = target[..., 0:2] + wh / 2
    enc = torch.cat([(cxy - anchors[:, :2]) / anchors[:, 2:] * XY_SCALE, torch.log(wh / anchors[:, 2:] + EPS) * WH_SCALE], -1)
    y = ((enc + LIMIT) / (2 * LIMIT / REG_MAX)).clamp(0, REG_MAX)
    y = torch.where(positive.unsqueeze(-1), y, torch.full_like(y, REG_MAX / 2))
    gen = torch.Generator(device=dev).manual_seed(2)
    logits = torch.randn((batch, A, 4, bins), device=dev, generator=gen)
    logits.scatter_add_(-1, y.round().long().unsqueeze(-1), torch.full((batch, A, 4, 1), 4.0, device=dev))
    dlocs = torch.randn((batch, A, 4), device=dev, generator=gen) * positive.unsqueeze(-1)
    grad = torch.ones((1,), device=dev)
    lib = _lib.lib()
    params = _lib.IntegralParams(bins, LIMIT, LIMIT, XY_SCALE, WH_SCALE, EPS, WEIGHT)
    ws = torch.empty((lib.ssdk_integral_workspace_bytes(batch, A),), dtype=torch.uint8, device=dev)
    locs, out2, dlogits = torch.empty((batch, A, 4), device=dev), torch.empty((2,), device=dev), torch.empty_like(logits)
    cls_ptr = cls.data_ptr()

    def ssdk_fwd():
        _lib.check(lib.ssdk_integral_fwd(ctypes.byref(params), _lib.ptr(logits), _lib.ptr(anchors), _lib.ptr(target), batch, A, _lib.ptr(locs),
                                         _lib.ptr(out2), _lib.ptr(ws), ws.numel(), _lib.current_stream()), 'ssdk_integral_fwd')

    def ssdk_bwd():
        _lib.check(lib.ssdk_integral_bwd(ctypes.byref(params), _lib.ptr(logits), _lib.ptr(dlocs), cls_ptr, 6, _lib.ptr(grad), batch, A,
                                         _lib.ptr(dlogits), _lib.ptr(ws), ws.numel(), _lib.current_stream()), 'ssdk_integral_bwd')
    ssdk_fwd()

    v = (-LIMIT + torch.arange(bins, device=dev, dtype=torch.float32) * (2 * LIMIT / REG_MAX)).view(1, 1, 1, bins)
    dfl = DistributionFocalLoss(reduction='sum', reg_max=REG_MAX)
    y_pos = y[positive].reshape(-1)
    scale = WEIGHT / 4.0 / max(1, int(positive.sum()))
    z = logits.clone().requires_grad_(True)
    state = {}

    def stock_fwd():
        s_locs = (torch.softmax(z, -1) * v).sum(-1)
        s_dfl = dfl(z[positive].reshape(-1, bins), y_pos) * scale
        state['out'] = (s_locs, s_dfl)

    def stock_bwd():
        state['dz'] = torch.autograd.grad(state['out'], z, (dlocs, grad[0]), retain_graph=True)[0]
    stock_fwd()
    stock_bwd()
    ssdk_bwd()
    torch.cuda.synchronize()
    agree = {'locs_max_abs': float((state['out'][0] - locs).abs().max()), 'dfl': [float(state['out'][1].detach()), float(out2[0])],
             'dlogits_max_abs': float((state['dz'] - dlogits).abs().max())}
    keep = (anchors, target, logits, dlocs, grad, ws, locs, out2, dlogits, params, z, v, y_pos, state)
    ssdk_fwd.keep = keep
    n = batch * A * 4
    shape = {'anchors': A, 'batch': batch, 'bins': bins, 'positives': int(positive.sum()), 'logit_bytes': n * bins * 4,
             'floor_fwd_us': round((n * bins * 4 + n * 4) / HBM_BYTES_PER_US, 1), 'floor_bwd_us': round((n * bins * 4 + n * 4) / HBM_BYTES_PER_US, 1),
             'floors': 'computed from the shapes at 6.0 TB/s, not measured', 'stock_vs_ssdk': agree, 'ssdk_version': lib.ssdk_version()}
    return {'ssdk': (ssdk_fwd, ssdk_bwd), 'stock': (stock_fwd, stock_bwd), 'ssdk2': (ssdk_fwd, ssdk_bwd)}, shape


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
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=5, help='calls per timing, at least; raised to fill --seconds')
    ap.add_argument('--seconds', type=float, default=0.5, help='timed device work per arm and direction, at least')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_dfl.py needs a GPU: there is nothing to time without one')
    calls, shape = make_calls(args.batch, torch.device('cuda:0'))
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
        base = (med['ssdk'] + med['ssdk2']) / 2
        floor = shape['floor_fwd_us'] if direction == 'fwd' else shape['floor_bwd_us']
        line = dict(shape, direction=direction, us={arm: round(x, 2) for arm, x in med.items()}, inner=inner, reps_per_round=args.reps,
                    round_medians_us={arm: [round(x, 2) for x in r] for arm, r in rounds.items()},
                    over_ssdk={arm: round(x / base, 3) for arm, x in med.items()}, aa_spread=round(abs(med['ssdk'] - med['ssdk2']) / base, 3),
                    over_floor={arm: round(x / floor, 2) for arm, x in med.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.writelines(json.dumps(line) + '\n' for line in lines)


if __name__ == '__main__':
    main()
