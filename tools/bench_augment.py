#!/usr/bin/env python3
"""Time the device-side SSD augmentation alone (``ssdk_augment_boxes`` / ``ssdk_augment_images``, csrc/augment.hip) through the C ABI:
32 images of 500 x 375 (random bytes, 1..8 boxes each) to 300 x 300 with the full SSD pipeline of the reference's sample configurations
(hue/saturation, brightness, contrast, expand, IoU-constrained crop, horizontal flip, resize, /255, normalise).  The parameter records are
drawn once with a seeded generator and everything is staged on the device before the timing, so the figures are the device work of
one batch: two launches for the boxes, three for the images.

  boxes    ssdk_augment_boxes   (choose + write)
  images   ssdk_augment_images  (two statistics passes + gather)
  images2  images again: the A/A' control

Device events around --inner back-to-back calls, queued behind ~1 ms of device spin so that the host is ahead of the GPU; the arms alternate
over --rounds rounds of --reps timings.  Bytes are computed from the shapes and the drawn records, not measured: a statistics pass reads the
source bytes of the images that need it, the gather writes B * 3 * out_h * out_w floats and reads the source bytes that lie inside each
image's window (once: the four taps of neighbouring output pixels come from the caches).  Per-launch times come from a separate
``rocprofv3 --kernel-trace --stats -- python tools/bench_augment.py --plain N`` run (N untimed batches, nothing else).

Usage:  python tools/bench_augment.py [--batch 32] [--rounds 5] [--reps 5] [--inner 20] [--out FILE.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from single_shot_detection_amd import _lib                                                          # noqa: E402
from single_shot_detection_amd.bf import preprocessing as P                                         # noqa: E402

H, W, OUT = 375, 500, (300, 300)
AUGMENTATIONS = [
    {'name': 'RandomAdjustHueSaturation', 'args': {'max_hue_delta': .1, 'saturation_delta_range': (.5, 1.5)}},
    {'name': 'ToFloat'},
    {'name': 'RandomAdjustBrightness', 'args': {'max_brightness_delta': .15}},
    {'name': 'RandomAdjustContrast', 'args': {'contrast_delta_range': (.5, 1.5)}},
    {'name': 'RandomExpand', 'args': {'aspect_ratio_range': (0.5, 2.0), 'area_range': (1.0, 16.0)}},
    {'name': 'OneOf', 'args': {'transforms': [{'name': 'Identity'}] + [{'name': 'RandomCrop', 'args': {'min_iou': v}} for v in (.0, .1, .3, .5, .7, .9)]}},
    {'name': 'RandomHorizontalFlip'},
]
PREPROCESSING = [{'name': 'ToFloatTensor', 'args': {'normalize': True}},
                 {'name': 'Normalize', 'args': {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}}]


def make_calls(batch, dev):
    rng = np.random.default_rng(1)
    aug = P.DeviceAugmentation(AUGMENTATIONS, PREPROCESSING, OUT)
    params = aug.draw([(H, W)] * batch, rng=np.random.default_rng(2))
    counts = rng.integers(1, 9, batch)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(offs[-1])
    x1, y1 = rng.uniform(0, W - 60, total), rng.uniform(0, H - 60, total)
    rows = np.stack([x1, y1, x1 + rng.uniform(20, 200, total), y1 + rng.uniform(20, 200, total), rng.integers(1, 21, total), np.ones(total)], 1)
    rows[:, 2], rows[:, 3] = np.minimum(rows[:, 2], W - 1), np.minimum(rows[:, 3], H - 1)
    desc = np.zeros(batch, P.IMAGE_DTYPE)
    desc['offset'], desc['height'], desc['width'] = np.arange(batch, dtype=np.int64) * (3 * H * W), H, W
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    d_src = up(rng.integers(0, 256, batch * 3 * H * W, dtype=np.uint8))
    d_desc, d_rec, d_cand = up(desc.view(np.uint8)), up(params.records.view(np.uint8)), up(params.candidates.reshape(-1))
    d_rows, d_offs = up(rows.astype(np.float32)), up(offs)
    rows_out, offs_out = torch.empty_like(d_rows), torch.empty_like(d_offs)
    attempt, windows = torch.empty((batch,), dtype=torch.int32, device=dev), torch.empty((batch, 4), dtype=torch.int32, device=dev)
    out = torch.empty((batch, 3, OUT[1], OUT[0]), dtype=torch.float32, device=dev)
    lib = _lib.lib()
    ws_b = torch.empty((lib.ssdk_augment_boxes_workspace_bytes(batch),), dtype=torch.uint8, device=dev)
    ws_i = torch.empty((lib.ssdk_augment_images_workspace_bytes(batch),), dtype=torch.uint8, device=dev)
    mean_std, T = aug.mean_std, int(params.candidates.shape[1])

    def boxes():
        _lib.check(lib.ssdk_augment_boxes(_lib.ptr(d_desc), _lib.ptr(d_rec), _lib.ptr(d_cand), T, _lib.ptr(d_rows), 6, _lib.ptr(d_offs), batch, total,
                                          OUT[0], OUT[1], _lib.ptr(rows_out), _lib.ptr(offs_out), _lib.ptr(attempt), _lib.ptr(windows), _lib.ptr(ws_b),
                                          ws_b.numel(), _lib.current_stream()), 'ssdk_augment_boxes')

    def images():
        _lib.check(lib.ssdk_augment_images(_lib.ptr(d_src), d_src.numel(), _lib.ptr(d_desc), _lib.ptr(d_rec), _lib.ptr(windows), batch, OUT[0], OUT[1],
                                           1, mean_std.ctypes.data_as(C.c_void_p), _lib.ptr(out), _lib.ptr(ws_i), ws_i.numel(), _lib.current_stream()),
                   'ssdk_augment_images')
    boxes()
    images()
    torch.cuda.synchronize()
    win = windows.cpu().numpy().astype(np.int64)
    inside = (np.clip(np.minimum(win[:, 0] + win[:, 2], W) - np.maximum(win[:, 0], 0), 0, None) *
              np.clip(np.minimum(win[:, 1] + win[:, 3], H) - np.maximum(win[:, 1], 0), 0, None))
    flags = params.records['flags']
    per_image = 3 * H * W
    shape = {'batch': batch, 'source': [H, W], 'out': list(OUT), 'boxes_in': total, 'boxes_out': int(offs_out[-1]),
             'attempts_chosen': attempt.cpu().tolist(), 'ssdk_version': lib.ssdk_version(),
             'bytes': {'stats1_read': int(((flags & P.CONTRAST) != 0).sum()) * per_image, 'stats2_read': int(((flags & P.EXPAND) != 0).sum()) * per_image,
                       'gather_read': int(3 * inside.sum()), 'gather_write': batch * 3 * OUT[0] * OUT[1] * 4,
                       'boxes': int(2 * total * 24 + params.candidates.nbytes)},
             'bytes_are': 'computed from the shapes and the drawn records, not measured', 'finite': bool(torch.isfinite(out).all())}
    images.keep = (d_src, d_desc, d_rec, d_cand, d_rows, d_offs, rows_out, offs_out, attempt, windows, out, ws_b, ws_i, mean_std)
    return {'boxes': boxes, 'images': images, 'images2': images}, shape


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
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--plain', type=int, default=0, help='run this many untimed batches and exit (for a kernel trace)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_augment.py needs a GPU: there is nothing to time without one')
    calls, shape = make_calls(args.batch, torch.device('cuda:0'))
    if args.plain:
        for _ in range(args.plain):
            calls['boxes']()
            calls['images']()
        torch.cuda.synchronize()
        print(json.dumps(shape))
        return
    for fn in calls.values():
        time_us(fn, args.inner, 2)
    rounds = {arm: [] for arm in calls}
    for _ in range(args.rounds):
        for arm, fn in calls.items():
            rounds[arm].append(time_us(fn, args.inner, args.reps))
    med = {arm: statistics.median(r) for arm, r in rounds.items()}
    img = (med['images'] + med['images2']) / 2
    moved = sum(v for k, v in shape['bytes'].items() if k != 'boxes')
    line = dict(shape, us={arm: round(x, 2) for arm, x in med.items()}, round_medians_us={arm: [round(x, 2) for x in r] for arm, r in rounds.items()},
                inner=args.inner, reps_per_round=args.reps, aa_spread=round(abs(med['images'] - med['images2']) / img, 3),
                batch_us=round(med['boxes'] + img, 2), images_per_s=round(args.batch / ((med['boxes'] + img) * 1e-6)),
                images_call_bytes=moved, images_call_gb_per_s=round(moved / (img * 1e-6) / 1e9, 1))
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
