#!/usr/bin/env python3
"""CPU emulation of the summation order of bn_reduce_kernel<1> (csrc/norm.hip) on the data of the dx-bar cases of
tests/test_batchnorm_kernels_gpu.py (the composed and the conditioning cases): per-lane fp32 chains in the kernel's row order, then the
cross-lane and cross-wave folds in fp32 or fp64, then the fp32 dx chain of bn_bwd_apply_kernel.  Prints the worst error / bar per case for
    the whole-row form, the slab form with fp32 folds, the slab form with fp64 folds
so that the choice of fp64 folds in the slab layouts can be checked without a GPU:   python tools/bn_fold_emulation.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import batchnorm_reference as bnref  # noqa: E402
import test_batchnorm_kernels_gpu as T  # noqa: E402  (its case builders are plain numpy)

F32 = np.float32


def sums_emul(x, y, dy, m, rs, relu, slab, rpb, fold64):
    rows, C = x.shape
    g = dy.copy()
    if relu & 1:
        g[~(y > 0)] = 0
    t0, t1 = g, (g * ((x - m) * rs)).astype(F32)
    rpw = 64 // slab
    S0, S1 = np.zeros(C, np.float64), np.zeros(C, np.float64)
    for r0 in range(0, rows, rpb):
        r1 = min(rows, r0 + rpb)
        acc0, acc1 = np.zeros((4, rpw, C), F32), np.zeros((4, rpw, C), F32)
        for wave in range(4):
            v = wave
            while r0 + v * rpw < r1:
                for u in range(4):
                    for sub in range(rpw):
                        ru = r0 + (v + 4 * u) * rpw + sub
                        if ru < r1:
                            acc0[wave, sub] = acc0[wave, sub] + t0[ru]
                            acc1[wave, sub] = acc1[wave, sub] + t1[ru]
                v += 16

        def fold(a):
            a = a.astype(np.float64) if fold64 else a
            n = rpw
            while n > 1:   # xor folds, lowest sub-row bit first
                a = np.stack([a[:, i] + a[:, i ^ 1] for i in range(0, n, 2)], axis=1)
                n //= 2
            t = a[0, 0]
            for w in range(1, 4):
                t = t + a[w, 0]
            return t.astype(np.float64)
        S0 += fold(acc0)
        S1 += fold(acc1)
    return S0, S1


def run_case(label, x, gamma, beta, dy, rm0, rv0, relu, skip_last=0):
    rows, C_ = x.shape
    args = (x, gamma, beta, rm0, rv0, T.MOMENTUM, T.EPS, True, relu, dy)
    ref, ideal = bnref.reference(*args), bnref.ideal_fp32(*args)
    m, rs = ref['save_mean'].astype(F32), ref['save_rstd'].astype(F32)
    bar = bnref.elementwise_bar(ideal['dx'], ref['dx'])
    C4 = C_ // 4
    for name, want, f64 in (('whole rows', 0, False), ('slab 16, fp32 folds', 16, False), ('slab 16, fp64 folds', 16, True)):
        target, least = (128, 64) if want == 0 else (64, 128)
        rpb = max(least, min(4096, -(-(-(-rows // target)) // 16) * 16))
        if want == 0:
            slab = C4 if (C4 <= 32 and 64 % C4 == 0) else 64
        else:
            slab = 1
            while slab < min(want, C4):
                slab *= 2
        S0, S1 = sums_emul(x, ref['y'], dy, m, rs, relu, slab, rpb, f64)
        m1, m2 = (S0 / rows).astype(F32), (S1 / rows).astype(F32)
        g = dy.copy()
        if relu & 1:
            g[~(ref['y'] > 0)] = 0
        xhat = ((x - m) * rs).astype(F32)
        v = (g - (m1 + xhat * m2).astype(F32)).astype(F32)
        dx = ((gamma * rs).astype(F32) * v).astype(F32)
        if relu & 2:
            dx = np.where(x > 0, dx, F32(0))
        err = np.abs(dx.astype(np.float64) - ref['dx']).max(axis=0)
        ratio = np.where(bar > 0, err / np.maximum(bar, 1e-300), 0)[:C_ - skip_last]
        print('%-34s %-20s slab %2d, %4d rows per workgroup: worst error / bar %.3f (channel %d)' % (label, name, slab, rpb, ratio.max(), ratio.argmax()))


def main():
    for seed in (31, 40):   # test_fwd_and_bwd_against_the_reference, test_chained_entry_points_over_three_cycles
        for rows, C_, relu in T.COMPOSED:
            run_case(f'composed {rows}x{C_} relu {relu} seed {seed}', *T._composed_case(rows, C_, relu, seed), relu)
    for rows, C_ in T.CONDITIONING:
        c = T._conditioning_case(rows, C_)
        run_case(f'conditioning {rows}x{C_}', c['x'], c['gamma'], c['beta'], c['dy'], c['rm0'], c['rv0'], 0, skip_last=2)


if __name__ == '__main__':
    main()
