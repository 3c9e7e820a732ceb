#!/usr/bin/env python3
"""Timing of the COCO-style evaluation (ssdk_coco_eval, csrc/metrics.hip) on a COCO-val-sized input: 5 000 images, 80 classes, about 100
detections and 7 ground truths per image, 10 % crowd.

Three figures, the first two from device events in alternating rounds (medians):
  1. ssdk_coco_eval end to end on packed device buffers (all twelve statistics, 10 thresholds x 4 area ranges x 3 max_dets);
  2. ten calls of the existing ssdk_mean_average_precision on the same input, one per IoU threshold -- the naive "sweep the threshold"
     alternative, which computes less (no area bins, no AR, no cap, VOC integration);
  3. the numpy reference of tests/coco_eval_reference.py on the host for a 200-image slice, EXTRAPOLATED linearly to 5 000 images.
``--rounds N`` timed rounds (default 9), ``--no-reference`` skips 3 (profiler runs), ``--images N`` another size."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from single_shot_detection_amd import _lib, synthetic as syn                                   # noqa: E402
from single_shot_detection_amd.detection.metrics.coco_evaluation import STAT_NAMES, default_tables   # noqa: E402

K = 81


def make_input(num_images, seed=7):
    return syn.make_map_case(seed=seed, num_images=num_images, num_classes=K, with_difficult=True, difficult_p=0.1, max_gt=14, noise_fp=184, dup=0.5,
                             unique_scores=None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--no-reference', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark measures the GPU: there is nothing to fall back to'
    lib = _lib.lib()
    pred, gts = make_input(args.images)
    n, counts = pred.shape[0], [g.shape[0] for g in gts]
    total = sum(counts)
    crowd = sum(int(g[:, 6].sum()) for g in gts)
    print(f'{args.images} images, {n} predictions ({n / args.images:.1f} per image), {total} ground truths ({total / args.images:.1f} per image, {crowd} crowd)')
    dev = torch.device('cuda')
    d_pred = torch.from_numpy(pred).to(dev)
    d_rows = torch.from_numpy(np.concatenate(gts, 0)).to(dev)
    d_offs = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
    iou, rec, area, md = default_tables()
    T, R, A, M = iou.size, rec.size, area.shape[0], md.size
    d_iou, d_rec, d_area = (torch.from_numpy(x).to(dev) for x in (iou, rec, area))
    ws = torch.empty((lib.ssdk_coco_eval_workspace_bytes(n, total, K, T, A),), dtype=torch.uint8, device=dev)
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    stats = torch.empty((12,), dtype=torch.float64, device=dev)
    ws_map = torch.empty((lib.ssdk_mean_average_precision_workspace_bytes(n, total, K),), dtype=torch.uint8, device=dev)
    ap_out = torch.empty((K,), dtype=torch.float32, device=dev)
    map_out = torch.empty((1,), dtype=torch.float64, device=dev)
    print(f'workspace: coco {ws.numel() / 2 ** 20:.1f} MiB, precision table {precision.numel() * 8 / 2 ** 20:.1f} MiB; mean_average_precision {ws_map.numel() / 2 ** 20:.1f} MiB')
    p = _lib.ptr

    def coco():
        _lib.check(lib.ssdk_coco_eval(p(d_pred), n, p(d_rows), 7, p(d_offs), len(gts), total, K, None, None, p(d_iou), T, p(d_rec), R, p(d_area), A,
                                      ctypes.c_void_p(md.ctypes.data), M, p(precision), p(recall), p(stats), p(ws), ws.numel(), _lib.current_stream()), 'ssdk_coco_eval')

    def sweep():
        for t in iou:
            _lib.check(lib.ssdk_mean_average_precision(p(d_pred), n, p(d_rows), 7, p(d_offs), len(gts), total, K, float(t), 0, p(ap_out), p(map_out), p(ws_map),
                                                       ws_map.numel(), _lib.current_stream()), 'ssdk_mean_average_precision')

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(2):
        coco()
        sweep()
    torch.cuda.synchronize()
    times = {'coco': [], 'sweep': []}
    for _ in range(args.rounds):
        times['coco'].append(timed(coco))
        times['sweep'].append(timed(sweep))
    for k, label in (('coco', 'ssdk_coco_eval, one call'), ('sweep', 'ssdk_mean_average_precision x 10 thresholds')):
        v = times[k]
        print(f'{label}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f} over {len(v)} alternating rounds (device events)')
    values = stats.cpu().numpy()
    print('statistics: ' + ', '.join(f'{k}={values[i]:.4f}' for i, k in enumerate(STAT_NAMES)))
    if not args.no_reference:
        import coco_eval_reference as ref
        m = min(200, args.images)
        sel = pred[pred[:, 0] < m]
        t0 = time.perf_counter()
        want = ref.evaluate(sel, gts[:m], K)
        dt = time.perf_counter() - t0
        print(f'numpy reference on the host, {m}-image slice ({sel.shape[0]} predictions): {dt:.2f} s; EXTRAPOLATED x {args.images / m:.0f} to {args.images} images: '
              f'{dt * args.images / m:.0f} s (not measured at that size)')
        from single_shot_detection_amd.detection.metrics.coco_evaluation import coco_evaluation
        got = coco_evaluation(torch.from_numpy(sel), [torch.from_numpy(g) for g in gts[:m]], {c: str(c) for c in range(K)}, verbose=False)
        err = max(abs(got[k] - want['stats'][k]) for k in STAT_NAMES)
        print(f'the slice on the device against it: largest difference of the twelve statistics {err:.2e}, precision table {np.abs(got["precision"].numpy() - want["precision"]).max():.2e}')


if __name__ == '__main__':
    main()
