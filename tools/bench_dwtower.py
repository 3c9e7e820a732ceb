#!/usr/bin/env python3
"""Time the depthwise RetinaNet-lite tower alone -- SharedConvPredictor(..., use_depthwise=True), detection/modules/predictors.py:8-76 --
train mode, forward + backward, at the RetinaNet-500 geometry (five levels 63, 32, 16, 8, 4; 4 layers; both heads):

  grouped    the tower as it runs now: per layer and head one grouped depthwise stencil over the levels, one grouped 1 x 1 GEMM with
             ReLU and BatchNorm statistics in its epilogue, the per-level norm kernels;
  per_level  what the tower ran before the grouped stencil existed, restated here on the same library: level by level the block's own
             forward (single-level stencil + single-problem 1 x 1 GEMM), then the stock nn.ReLU and nn.BatchNorm2d modules.

Device events around each iteration; after a warm-up the two versions alternate over --rounds rounds of --iters iterations, in both
modes of ops.set_deterministic; the report is the median of the round medians and their spread for every (channels, mode, version).
Eager calls: the time includes the host's enqueue time.

Usage:  python tools/bench_dwtower.py [--batch 32] [--channels 256 64] [--rounds 5] [--iters 20] [--out FILE.json]
        python tools/bench_dwtower.py --only grouped --channels 256 --iters 5 --rounds 1 --warmup 0 [--forward-only]
        (a short one-version run, e.g. under a kernel trace: the launches per forward pass, and per forward + backward pass)
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from single_shot_detection_amd import ops                                                       # noqa: E402
from single_shot_detection_amd.detection.modules.predictors import SharedConvPredictor          # noqa: E402

LEVELS = (63, 32, 16, 8, 4)


def per_level_forward(tower, sources):
    """The tower's forward with every layer on the level-by-level path."""
    s = l = list(sources)
    if tower.training:
        ops.prepare_weight_transposes(tower.convs)
    for sc, lc, sn, ln in zip(tower.convs['score'], tower.convs['loc'], tower.norms['score'], tower.norms['loc']):
        s = [norm(tower.activation(sc(x))) for norm, x in zip(sn, s)]
        l = [norm(tower.activation(lc(x))) for norm, x in zip(ln, l)]
    return s, l


def make(batch, channels, layers, dev, forward_only=False):
    torch.manual_seed(0)
    grouped = SharedConvPredictor([channels] * len(LEVELS), [9] * len(LEVELS), 80, True, num_layers=layers, num_channels=channels)
    per_level = copy.deepcopy(grouped).to(dev).train()
    grouped = grouped.to(dev).train()
    srcs = [torch.randn((batch, channels, n, n), device=dev).contiguous(memory_format=torch.channels_last) for n in LEVELS]
    inputs = {'grouped': [s.clone().requires_grad_(True) for s in srcs], 'per_level': [s.clone().requires_grad_(True) for s in srcs]}
    params = {'grouped': list(grouped.parameters()) + inputs['grouped'], 'per_level': list(per_level.parameters()) + inputs['per_level']}
    gs = {}

    def step(name, fwd):
        s, l = fwd(inputs[name])
        outs = list(s) + list(l)
        if name not in gs:
            gs[name] = [torch.ones_like(o) for o in outs]
        if not forward_only:
            torch.autograd.backward(outs, gs[name])
    return {'grouped': lambda: step('grouped', grouped), 'per_level': lambda: step('per_level', lambda xs: per_level_forward(per_level, xs))}, params


def time_iters(step, params, iters):
    times = []
    for _ in range(iters):
        for p in params:
            p.grad = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times) if times else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--channels', type=int, nargs='+', default=[256, 64])
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', choices=['grouped', 'per_level'], default=None)
    ap.add_argument('--modes', choices=['default', 'deterministic'], nargs='+', default=['default', 'deterministic'])
    ap.add_argument('--forward-only', action='store_true', help='forward passes only (launch counts: run once with, once without)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    results = []
    names = [args.only] if args.only else ['grouped', 'per_level']
    for c in args.channels:
        steps, params = make(args.batch, c, args.layers, dev, args.forward_only)
        for mode in args.modes:
            ops.set_deterministic(mode == 'deterministic')
            for n in names:
                time_iters(steps[n], params[n], args.warmup)
            rounds = {n: [] for n in names}
            for _ in range(args.rounds):
                for n in names:
                    rounds[n].append(time_iters(steps[n], params[n], args.iters))
            for n in names:
                r = rounds[n]
                line = {'batch': args.batch, 'channels': c, 'layers': args.layers, 'mode': mode, 'version': n, 'forward_only': args.forward_only,
                        'median_us': statistics.median(r), 'min_round_us': min(r), 'max_round_us': max(r), 'round_medians_us': r,
                        'iters_per_round': args.iters}
                print(json.dumps(line), flush=True)
                results.append(line)
        ops.set_deterministic(False)
        del steps, params
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
