#!/usr/bin/env python3
"""Time the task-aligned encode call alone (``ssdk_encode_ground_truth_tal``: tal_candidates_kernel + tal_assign_kernel +
tal_normalise_kernel, csrc/match.hip) against the default ``TargetAssigner(0.5, 0.4)`` call (``ssdk_encode_ground_truth``) and the ATSS call
(``ssdk_encode_ground_truth_atss``) on the same inputs, through the C ABI on ground truth that is already packed on the device, at
RetinaNet-500 geometry (47 961 anchors in five levels, batch 32, 80 logit columns):

  retina500_b32_default_g   synthetic.make_ground_truth's default 1..8 boxes per image (142 boxes)
  retina500_b32_g32         32 boxes per image (1 024 boxes)

The predictions are drawn on the device from a fixed seed: logits 2 * N(0, 1) - 2, locs N(0, 1) * (1.5, 1.5, 1, 1).  Device events around
--inner back-to-back calls, queued behind ~1 ms of device spin so that the host is ahead of the GPU.  After a warm-up four arms alternate
within the process -- default (A), ATSS, TAL, default again (A') -- over --rounds rounds of --reps timings; --inner is raised until every
arm's timed calls fill --seconds.  Per case: the median of the round medians of each arm, TAL over ATSS and over the mean of A and A', and
the A/A' spread |A - A'| / mean beside them -- a ratio inside that spread says nothing.  The bytes the shapes imply are computed beside
them: the anchor table once per box, B * A * 16 of locs once, the locs and the one logit of the inside anchors only, the target once.

Usage:  python tools/bench_tal.py [--rounds 5] [--reps 7] [--seconds 1.0] [--topk 13] [--out FILE.txt]
        python tools/bench_tal.py --rounds 1 --reps 2 --seconds 0      (a short run, e.g. under rocprofv3 --kernel-trace --stats)
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
CASES = {
    'retina500_b32_default_g': dict(seed=1),
    'retina500_b32_g32': dict(seed=1, fixed_g=32),
}


def make_calls(case, topk, atss_topk, dev):
    cfg = syn.CONFIGS[CONFIG]
    anchors = torch.from_numpy(np.load(os.path.join(REPO, 'tests', 'golden', f'{CONFIG}.npz'))['anchors']).to(dev)
    sizes = [h * h * nb for _, h, nb in cfg['levels']]
    gt = syn.make_ground_truth(BATCH, cfg['size'], COLUMNS + 1, **CASES[case])
    rows, offs, total = pack_ground_truth([torch.from_numpy(g) for g in gt], dev)
    A = anchors.shape[0]
    assert sum(sizes) == A
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    scores = torch.randn((BATCH, A, COLUMNS), generator=gen, device=dev) * 2.0 - 2.0
    locs = torch.randn((BATCH, A, 4), generator=gen, device=dev) * torch.tensor([1.5, 1.5, 1.0, 1.0], device=dev)
    lib = _lib.lib()
    target = torch.empty((BATCH, A, 6), dtype=torch.float32, device=dev)
    levels = (ctypes.c_int32 * len(sizes))(*sizes)
    ws_d = torch.empty((max(lib.ssdk_encode_ground_truth_workspace_bytes(BATCH, total), 4096),), dtype=torch.uint8, device=dev)
    ws_a = torch.empty((max(lib.ssdk_encode_ground_truth_atss_workspace_bytes(BATCH, total, len(sizes)), 4096),), dtype=torch.uint8, device=dev)
    ws_t = torch.empty((max(lib.ssdk_encode_ground_truth_tal_workspace_bytes(BATCH, total, topk), 4096),), dtype=torch.uint8, device=dev)

    def default():
        _lib.check(lib.ssdk_encode_ground_truth(_lib.ptr(rows), 6, _lib.ptr(offs), BATCH, total, _lib.ptr(anchors), A, 0.5, 0.4, _lib.ptr(target),
                                                None, _lib.ptr(ws_d), ws_d.numel(), _lib.current_stream()), 'ssdk_encode_ground_truth')

    def atss():
        _lib.check(lib.ssdk_encode_ground_truth_atss(_lib.ptr(rows), 6, _lib.ptr(offs), BATCH, total, _lib.ptr(anchors), A, levels, len(sizes), atss_topk,
                                                     _lib.ptr(target), None, _lib.ptr(ws_a), ws_a.numel(), _lib.current_stream()),
                   'ssdk_encode_ground_truth_atss')

    def tal():
        _lib.check(lib.ssdk_encode_ground_truth_tal(_lib.ptr(rows), 6, _lib.ptr(offs), BATCH, total, _lib.ptr(anchors), A, _lib.ptr(scores), COLUMNS,
                                                    _lib.ptr(locs), 10.0, 5.0, topk, 1.0, 6.0, _lib.ptr(target), None, _lib.ptr(ws_t), ws_t.numel(),
                                                    _lib.current_stream()), 'ssdk_encode_ground_truth_tal')
    default.keep = atss.keep = tal.keep = (anchors, rows, offs, target, ws_d, ws_a, ws_t, levels, scores, locs)
    # the (box, anchor) pairs whose centre lies inside: the only ones whose loc and logit the candidate launch loads
    inside = 0
    for g in gt:
        b = torch.from_numpy(g).to(dev)
        cx, cy = anchors[:, 0][None], anchors[:, 1][None]
        inside += int(((b[:, 0:1] < cx) & (cx < b[:, 2:3]) & (b[:, 1:2] < cy) & (cy < b[:, 3:4])).sum())
    tal()
    torch.cuda.synchronize()
    shape = {'anchors': A, 'levels': sizes, 'batch': BATCH, 'columns': COLUMNS, 'boxes': total, 'topk': topk, 'atss_topk': atss_topk,
             'inside_pairs': inside, 'positives': int((target[..., 4] > 0).sum()),
             'candidate_launch_anchor_bytes': total * A * 16, 'candidate_launch_loc_bytes': inside * 16, 'candidate_launch_logit_bytes': inside * 4,
             'assign_launch_anchor_bytes': BATCH * A * 16, 'assign_launch_loc_bytes': BATCH * A * 16, 'assign_launch_logit_bytes': inside * 4,
             'target_bytes_written': BATCH * A * 24, 'normalise_launch_slots': total * 32}
    return {'default_a': default, 'atss': atss, 'tal': tal, 'default_b': default}, shape


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
    ap.add_argument('--seconds', type=float, default=1.0, help='timed device work per arm, at least')
    ap.add_argument('--topk', type=int, default=13)
    ap.add_argument('--atss-topk', type=int, default=9)
    ap.add_argument('--cases', nargs='+', default=list(CASES), choices=list(CASES))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_tal.py needs a GPU: there is nothing to time without one')
    dev = torch.device('cuda:0')
    lines = []
    for case in args.cases:
        calls, shape = make_calls(case, args.topk, args.atss_topk, dev)
        warm = {arm: time_us(call, args.inner, 2) for arm, call in calls.items()}   # warm-up, and the call time that sizes --inner
        inner = max(args.inner, math.ceil(1.15 * args.seconds * 1e6 / (min(warm.values()) * args.rounds * args.reps)))   # (warm-up calls run a little slow)
        rounds = {arm: [] for arm in calls}
        for _ in range(args.rounds):
            for arm, call in calls.items():
                rounds[arm].append(time_us(call, inner, args.reps))
        med = {arm: statistics.median(r) for arm, r in rounds.items()}
        base = (med['default_a'] + med['default_b']) / 2
        line = dict(shape, case=case, tal_us=round(med['tal'], 2), atss_us=round(med['atss'], 2), default_a_us=round(med['default_a'], 2),
                    default_b_us=round(med['default_b'], 2), tal_over_atss=round(med['tal'] / med['atss'], 3),
                    tal_over_default=round(med['tal'] / base, 3), aa_spread=round(abs(med['default_a'] - med['default_b']) / base, 3),
                    round_medians_us={arm: [round(x, 2) for x in r] for arm, r in rounds.items()}, inner=inner, reps_per_round=args.reps,
                    timed_seconds_per_arm=round(min(med.values()) * inner * args.reps * args.rounds / 1e6, 2))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.writelines(json.dumps(line) + '\n' for line in lines)


if __name__ == '__main__':
    main()
