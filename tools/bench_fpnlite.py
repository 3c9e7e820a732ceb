#!/usr/bin/env python3
"""Time the FPN-lite neck alone -- FeaturePyramid(..., use_depthwise=True), bf/modules/features.py:52-120, everything behind the backbone
taps -- at the RetinaNet-lite geometry: batch 32, 256 and 128 pyramid channels, tapped levels 63 / 32 / 16 and two stride-2 extra levels;
forward + backward in train(), forward under no_grad in eval().  Versions:

  fused     the neck as it runs now: every pyramid_output block is ops.depthwise_conv2d_batch_norm -- in training the stencil's launch
            accumulates the norm's statistics and the norm is one apply launch, in evaluation the whole block is one launch;
  two_pass  the same with the SSDK_NO_FUSED_STATS knob: stencil, then the norm's own statistics + apply (training) or apply (evaluation);
  stock     the blocks' _forward_stock line -- MIOpen's grouped convolution, torch's batch norm and ReLU -- which is what the neck ran before
            the depthwise line existed; the laterals and the top-down step are on libssdk in all versions;
  stock_b   a second, independent copy of `stock`: the A/A pair whose spread is the yardstick of the acceptance.

Device events around each iteration; after a warm-up the versions alternate over --rounds rounds of --iters iterations, in both modes of
ops.set_deterministic; the report is the median of the round medians and their spread for every (channels, phase, mode, version), and per
(channels, phase, mode) the verdict: fused is accepted when it is not slower than stock by more than the A/A spread of stock / stock_b.
Eager calls: the time includes the host's enqueue time.

Usage:  python tools/bench_fpnlite.py [--batch 32] [--channels 256 128] [--rounds 5] [--iters 20] [--out FILE.json]
        python tools/bench_fpnlite.py --only fused --channels 256 --phases train --iters 5 --rounds 1 --warmup 0
        (a short one-version run, e.g. under a kernel trace: the launches per block)
"""
import argparse
import copy
import itertools
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from single_shot_detection_amd import ops                                   # noqa: E402
from single_shot_detection_amd.bf.modules import features                   # noqa: E402

TAPS = ((32, 63), (96, 32), (320, 16))   # (channels, size) of the backbone taps: MobileNetV2's at strides 8, 16, 32 of a 500 x 500 input
EXTRA = 2
VERSIONS = ('fused', 'two_pass', 'stock', 'stock_b')


class _Base(nn.Module):
    """Only the taps' channel counts matter: the neck is run on given tap tensors."""

    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for c, _ in TAPS:
            layers.append(nn.Conv2d(cin, c, 3, stride=2, padding=1))
            cin = c
        self.features = nn.Sequential(*layers)


def stock_neck(m, sources):
    """FeaturePyramid.neck with every pyramid_output block on its stock line."""
    if m.training:
        ops.prepare_weight_transposes(m.pyramid_lateral)
    feats = [ops.conv2d(s, lat.weight, lat.bias) for s, lat in zip(sources, m.pyramid_lateral)]
    for i in reversed(range(len(feats) - 1)):
        feats[i] = features._upsample_add(feats[i], feats[i + 1], m.interpolation_mode)
    outs = []
    for block, f in itertools.zip_longest(m.pyramid_output, feats):
        outs.append(block._forward_stock(f if f is not None else outs[-1]))
    return outs


def make(batch, channels, dev):
    torch.manual_seed(0)
    proto = features.FeaturePyramid(_Base(), tuple(range(len(TAPS))), pyramid_layers=len(TAPS) + EXTRA, pyramid_channels=channels, use_depthwise=True)
    assert all(b._why_not_hip() is None for b in proto.pyramid_output)
    srcs = [torch.randn((batch, c, n, n), device=dev).contiguous(memory_format=torch.channels_last) for c, n in TAPS]
    mods = {v: copy.deepcopy(proto).to(dev) for v in VERSIONS}
    inputs = {v: [s.clone().requires_grad_(True) for s in srcs] for v in VERSIONS}
    params = {v: [p for n, p in mods[v].named_parameters() if not n.startswith('base.')] + inputs[v] for v in VERSIONS}
    gs = {}

    def run(v, xs):
        if v.startswith('stock'):
            return stock_neck(mods[v], xs)
        ops._NO_FUSED_STATS = v == 'two_pass'
        try:
            return mods[v].neck(xs)[0]
        finally:
            ops._NO_FUSED_STATS = False

    def step(v, phase):
        if phase == 'train':
            mods[v].train()
            outs = run(v, inputs[v])
            if v not in gs:
                gs[v] = [torch.ones_like(o) for o in outs]
            torch.autograd.backward(outs, gs[v])
        else:
            mods[v].eval()
            with torch.no_grad():
                run(v, [x.detach() for x in inputs[v]])
    return step, params


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
    ap.add_argument('--channels', type=int, nargs='+', default=[256, 128])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', choices=VERSIONS, default=None)
    ap.add_argument('--phases', choices=['train', 'eval'], nargs='+', default=['train', 'eval'])
    ap.add_argument('--modes', choices=['default', 'deterministic'], nargs='+', default=['default', 'deterministic'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    results = []
    names = [args.only] if args.only else list(VERSIONS)
    for c in args.channels:
        step, params = make(args.batch, c, dev)
        for phase in args.phases:
            for mode in args.modes:
                ops.set_deterministic(mode == 'deterministic')
                for n in names:
                    time_iters(lambda: step(n, phase), params[n], args.warmup)
                rounds = {n: [] for n in names}
                for _ in range(args.rounds):
                    for n in names:
                        rounds[n].append(time_iters(lambda: step(n, phase), params[n], args.iters))
                med = {}
                for n in names:
                    r = rounds[n]
                    med[n] = statistics.median(r)
                    line = {'batch': args.batch, 'channels': c, 'phase': phase, 'mode': mode, 'version': n, 'median_us': med[n], 'min_round_us': min(r),
                            'max_round_us': max(r), 'round_medians_us': r, 'iters_per_round': args.iters}
                    print(json.dumps(line), flush=True)
                    results.append(line)
                if all(n in med for n in VERSIONS):
                    # A/A spread: the largest difference between the two stock copies' medians of the same round, and between their medians
                    aa = max([abs(a - b) for a, b in zip(rounds['stock'], rounds['stock_b'])] + [abs(med['stock'] - med['stock_b'])])
                    base = min(med['stock'], med['stock_b'])
                    verdict = {'channels': c, 'phase': phase, 'mode': mode, 'aa_spread_us': aa, 'stock_us': base, 'fused_us': med['fused'],
                               'two_pass_us': med['two_pass'], 'fused_accepted': med['fused'] <= base + aa, 'two_pass_beats_fused': med['two_pass'] < med['fused']}
                    print(json.dumps(verdict), flush=True)
                    results.append(verdict)
        ops.set_deterministic(False)
        del step, params
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
