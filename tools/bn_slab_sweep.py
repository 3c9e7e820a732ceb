#!/usr/bin/env python3
"""Event-timed sweep of the BatchNorm statistics launches (bn_reduce_kernel<0> forward, <1> backward with the ReLU mask) over the slab width
and the rows per workgroup, on one binary -- the library reads SSDK_BN_SLAB / SSDK_BN_ROWS / SSDK_BN_WGS per call:
    python tools/bn_slab_sweep.py [reps]
Maps: the eight layers of the SSD-300 tail at batch 32, the M2Det neck's maps at batch 16 (tools/bench_bn.py), the five levels of the
RetinaNet tower at batch 32.  us per launch = (events around `reps` back-to-back launches) / reps: it includes the launch boundary, as a step
does; the maps are warm in the last-level cache, as they are behind the convolution that wrote them.
BN_SWEEP_RULES=1: rules for the rows per workgroup instead (rows = max(floor, rows / target row blocks) rounded up to 16) at slab widths 8 - 32."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from single_shot_detection_amd import _lib  # noqa: E402

MAPS = ([('ssd300', 32 * h * h, c) for h, c in ((18, 256), (9, 512), (9, 128), (5, 256), (5, 128), (3, 256), (3, 128), (2, 256))] +
        [('m2det', 16 * h * h, c) for h, c in ((64, 512), (64, 896), (64, 128), (32, 256), (32, 128), (16, 256), (16, 128), (8, 128), (4, 256))] +
        [('retina', 32 * h * h, 256) for h in (63, 32, 16, 8, 4)])
# a setting: the knobs as the library reads them, or (slab, target row blocks, least rows per workgroup) turned into SSDK_BN_ROWS per map
SETTINGS = [dict(SSDK_BN_SLAB='0'), dict(SSDK_BN_SLAB='8'), dict(SSDK_BN_SLAB='16'), dict(SSDK_BN_SLAB='32'), dict(SSDK_BN_SLAB='64'),
            dict(SSDK_BN_SLAB='16', SSDK_BN_ROWS='32'), dict(SSDK_BN_SLAB='16', SSDK_BN_ROWS='128'), dict(SSDK_BN_SLAB='16', SSDK_BN_WGS='64'),
            dict(SSDK_BN_SLAB='16', SSDK_BN_WGS='256'), dict(SSDK_BN_SLAB='32', SSDK_BN_WGS='256')]
if os.environ.get('BN_SWEEP_RULES'):
    SETTINGS = [dict(SSDK_BN_SLAB='0'), dict(SSDK_BN_SLAB='16')] + [(16, t, f) for t, f in ((64, 64), (64, 128), (64, 256), (32, 128), (32, 256), (96, 128), (48, 128))] + \
               [(32, 64, 128), (8, 64, 128)]
KNOBS = ('SSDK_BN_SLAB', 'SSDK_BN_ROWS', 'SSDK_BN_WGS')


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    lib, st = _lib.lib(), _lib.current_stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    label = lambda s: ' '.join(f'{k[8:].lower()}={v}' for k, v in s.items()) if isinstance(s, dict) else 'slab=%d rows=max(%d, rows/%d)' % (s[0], s[2], s[1])
    print('us per launch, forward / backward statistics | ' + ' | '.join(label(s) for s in SETTINGS))
    totals = {}
    for net, rows, ch in MAPS:
        x, y, dy = (torch.randn(rows, ch, device='cuda') for _ in range(3))
        mean, rstd = torch.zeros(ch, device='cuda'), torch.ones(ch, device='cuda')
        sums = torch.zeros(2 * ch + 2, dtype=torch.float64, device='cuda')
        cells = []
        for k, s in enumerate(SETTINGS):
            for knob in KNOBS:
                os.environ.pop(knob, None)
            if not isinstance(s, dict):
                s = dict(SSDK_BN_SLAB=str(s[0]), SSDK_BN_ROWS=str(min(4096, max(s[2], (-(-rows // s[1]) + 15) // 16 * 16))))
            os.environ.update(s)
            plan = (C.c_longlong * 4)()
            assert lib.ssdk_debug_batchnorm_plan(rows, ch, plan) == 0
            f = timed(lambda: lib.ssdk_batchnorm_stats_accumulate(p(x), rows, ch, p(sums), st), reps)
            b = timed(lambda: lib.ssdk_batchnorm_bwd_stats(p(x), p(y), p(dy), rows, ch, p(mean), p(rstd), 1, p(sums), st), reps)
            # (_bwd_stats zero-fills `sums` first: one small fill launch rides along in every backward figure, the same in every column)
            cells.append(f'{f:5.1f} / {b:5.1f} ({plan[1] * plan[3]} wg)')
            t = totals.setdefault((net, k), [0.0, 0.0])
            t[0] += f
            t[1] += b
        print(f'{net} {rows} x {ch} | ' + ' | '.join(cells), flush=True)
    for net in ('ssd300', 'm2det', 'retina'):
        print(f'{net} sum | ' + ' | '.join('%6.1f / %6.1f' % tuple(totals[(net, k)]) for k in range(len(SETTINGS))))


if __name__ == '__main__':
    main()
