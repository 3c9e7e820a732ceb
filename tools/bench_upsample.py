#!/usr/bin/env python3
"""Event-timed top-down step of the necks -- out = fine + interpolate(coarse) and its coarse gradient -- in bilinear mode on libssdk
(ssdk_upsample_bilinear_add_fwd / _bwd) against (a) the nearest kernels at the same shapes and (b) torch's F.interpolate(mode='bilinear')
+ add / upsample_bilinear2d_backward on channels_last tensors.  Shapes: M2Det-512's TUM steps 2 -> 4 ... 32 -> 64 and the base upscaling
32 -> 64 (no `fine`), batch 16, 256 channels.

The entry points are called directly on preallocated buffers (no autograd, no allocation in the timed window; torch's path allocates
its results, as it does inside the neck).  The launches of a window walk a ring of buffer sets, about 1 GiB in all at the large shapes,
so the 256 MB infinity cache does not serve a launch what an earlier one left; the small shapes (a few hundred KB) are launch-bound and
cache-resident in any case.  A window is `--reps` back-to-back launches between two events; the variants alternate inside a trial and the
median and the minimum over `--trials` trials are printed.  Algorithmic bytes: 4 B C (2 hf wf + hc wc) forward with `fine`,
4 B C (hf wf + hc wc) forward without and backward.  `--hbm-tbs`: the streaming-copy rate tools/hbm_peak.hip printed on the same
machine (TB/s); fractions are of that rate.

    python tools/bench_upsample.py [--hbm-tbs 4.3] [--batch 16] [--channels 256] [--reps 50] [--trials 7]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from single_shot_detection_amd import _lib  # noqa: E402

STEPS = [(2, 4), (4, 8), (8, 16), (16, 32), (32, 64)]
RING_BYTES = 1 << 30


def window(fn, sets, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(reps):
        fn(sets[r % len(sets)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us per launch


def bench(variants, sets, reps, trials):
    for fn in variants.values():   # warm-up: code objects, torch's allocator
        for s in sets:
            fn(s)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(trials):
        for k, fn in variants.items():
            times[k].append(window(fn, sets, reps))
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hbm-tbs', type=float, default=None)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--trials', type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_upsample.py measures on the GPU; there is nothing to report without one'
    dev = torch.device('cuda')
    lib, B, C = _lib.lib(), args.batch, args.channels
    prop = torch.cuda.get_device_properties(0)
    print(f'{prop.name}, {prop.multi_processor_count} CUs (clocks as the machine runs them: nothing pinned); batch {B}, {C} channels, {args.reps} launches per window, {args.trials} trials; '
          f'HBM copy rate {args.hbm_tbs} TB/s')

    def cl(h, w):
        return torch.randn((B, C, h, w), device=dev).contiguous(memory_format=torch.channels_last)

    p = _lib.ptr
    for hc, hf, with_fine in [(a, b, True) for a, b in STEPS] + [(32, 64, False)]:   # the last row is the base upscaling
        fwd_bytes = 4 * B * C * ((2 if with_fine else 1) * hf * hf + hc * hc)
        bwd_bytes = 4 * B * C * (hf * hf + hc * hc)
        n_sets = max(2, min(8, RING_BYTES // (4 * B * C * (3 * hf * hf + 2 * hc * hc)) + 1))
        sets = [dict(fine=cl(hf, hf), coarse=cl(hc, hc), out=cl(hf, hf), dout=cl(hf, hf), dcoarse=cl(hc, hc)) for _ in range(n_sets)]
        st = _lib.current_stream()

        def lib_fwd(name):
            f = getattr(lib, name)
            return lambda s: f(p(s['fine']) if with_fine else None, p(s['coarse']), B, hf, hf, hc, hc, C, p(s['out']), st)

        def lib_bwd(name):
            f = getattr(lib, name)
            return lambda s: f(p(s['dout']), B, hf, hf, hc, hc, C, p(s['dcoarse']), st)

        def torch_fwd(s):
            up = F.interpolate(s['coarse'], size=(hf, hf), mode='bilinear')
            return s['fine'] + up if with_fine else up

        def torch_bwd(s):
            return torch.ops.aten.upsample_bilinear2d_backward(s['dout'], [hf, hf], [B, C, hc, hc], False, None, None)

        # parity at the timed size before any number is reported
        s0 = sets[0]
        assert lib_fwd('ssdk_upsample_bilinear_add_fwd')(s0) == 0 and lib_bwd('ssdk_upsample_bilinear_add_bwd')(s0) == 0
        ref_f, ref_b = torch_fwd(s0), torch_bwd(s0)
        assert (s0['out'] - ref_f).abs().max().item() <= 1e-4 * ref_f.abs().max().item()
        assert (s0['dcoarse'] - ref_b).abs().max().item() <= 1e-4 * ref_b.abs().max().item()

        with torch.no_grad():
            res = bench({'bilinear fwd': lib_fwd('ssdk_upsample_bilinear_add_fwd'), 'nearest fwd': lib_fwd('ssdk_upsample_nearest_add_fwd'),
                         'torch fwd': torch_fwd, 'bilinear bwd': lib_bwd('ssdk_upsample_bilinear_add_bwd'),
                         'nearest bwd': lib_bwd('ssdk_upsample_nearest_add_bwd'), 'torch bwd': torch_bwd}, sets, args.reps, args.trials)
        label = f'{hc:2d} -> {hf:2d}' + ('' if with_fine else ' (base, no fine)')
        for k, (med, best) in res.items():
            nbytes = fwd_bytes if k.endswith('fwd') else bwd_bytes
            tbs = nbytes / med / 1e6
            frac = f', {tbs / args.hbm_tbs:.2f} of the copy rate' if args.hbm_tbs else ''
            print(f'{label:24s} {k:13s} median {med:8.1f} us (min {best:8.1f}), {nbytes / 1e6:7.2f} MB -> {tbs:5.2f} TB/s{frac}   [{n_sets} buffer sets]')
        del sets
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
