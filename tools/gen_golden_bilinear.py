#!/usr/bin/env python3
"""Golden vectors of the necks in ``interpolation_mode='bilinear'``, produced by RUNNING THE REFERENCE'S ``FeaturePyramid``,
``ThinnedUshapeModule`` and ``MultilevelFeaturePyramid`` (bf/modules/features.py:52-120, :215-270, :303-393) on the CPU, on the cases of
tests/bilinear_cases.py: eval() and one train() step -- the outputs, the input gradient, every parameter gradient and the BatchNorm
buffers afterwards.

Written to tests/golden/necks_bilinear.npz (keys as tests/blocks_cases.pack writes them, per case: <case>/<mode>/y<i>, <case>/<mode>/dx0,
<case>/<mode>/dp/<name>, <case>/buffers/<name>, and `cases`, the list of case names).

Uses tools/gen_golden.py's import shims (runs only where the reference tree is present).
Usage:  python tools/gen_golden_bilinear.py [--out tests/golden]
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
import bilinear_cases                                # noqa: E402
from bf.modules import features as ref_features      # noqa: E402


def gen(out_dir):
    mods = types.SimpleNamespace(FeaturePyramid=ref_features.FeaturePyramid, ThinnedUshapeModule=ref_features.ThinnedUshapeModule,
                                 MultilevelFeaturePyramid=ref_features.MultilevelFeaturePyramid)
    res = {'cases': np.array(sorted(bilinear_cases.CASES))}
    for name in bilinear_cases.CASES:
        res.update(bilinear_cases.run_case(name, mods, torch.device('cpu')))
    path = os.path.join(out_dir, 'necks_bilinear.npz')
    np.savez_compressed(path, **res)
    print(f'necks_bilinear -> {path} ({os.path.getsize(path) / 1e3:.1f} KB, {len(res)} arrays)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    gen(args.out)


if __name__ == '__main__':
    main()
