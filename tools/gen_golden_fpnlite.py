#!/usr/bin/env python3
"""Golden vectors of the FPN-lite neck, produced by RUNNING THE REFERENCE'S ``FeaturePyramid(..., use_depthwise=True)``
(bf/modules/features.py:52-120; :79-98 builds every ``pyramid_output`` block as ``Conv2dBn(C, C, 3, groups=C)``, the extra levels with stride 2
and padding 1) on the CPU, on the cases of tests/fpnlite_cases.py: eval() and one train() step -- the outputs, the input gradient, every
parameter gradient and the BatchNorm buffers afterwards.  Every level's size is asserted as the cases file states it.

Written to tests/golden/fpn_lite.npz (keys as tests/bilinear_cases.pack_sampled writes them, per case: <case>/<mode>/y<i>, <case>/<mode>/dx0,
<case>/<mode>/dp/<name>, <case>/buffers/<name>, and `cases`, the list of case names).  Only results go into the fixture.

Uses tools/gen_golden.py's import shims (runs only where the reference tree is present).
Usage:  python tools/gen_golden_fpnlite.py [--out tests/golden]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools import gen_golden   # noqa: E402,F401  (shims first: torch.jit.scope, the stubbed third-party modules)

sys.path.insert(0, os.path.join(REPO, 'tests'))
import fpnlite_cases                                 # noqa: E402
from bf.modules import features as ref_features      # noqa: E402


def gen(out_dir):
    mods = types.SimpleNamespace(FeaturePyramid=ref_features.FeaturePyramid)
    res = {'cases': np.array(sorted(fpnlite_cases.CASES))}
    for name in fpnlite_cases.CASES:
        res.update(fpnlite_cases.run_case(name, mods, torch.device('cpu')))
    path = os.path.join(out_dir, 'fpn_lite.npz')
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print(f'fpn_lite -> {path} ({size / 1e3:.1f} KB, {len(res)} arrays)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    gen(args.out)


if __name__ == '__main__':
    main()
