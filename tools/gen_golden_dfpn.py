#!/usr/bin/env python3
"""Golden vectors of the depthwise feature pyramid (Tiny-DSOD D-FPN), produced by RUNNING THE REFERENCE'S ``DepthwiseFeaturePyramid``
(bf/modules/features.py:123-212) on the CPU, on the cases of tests/dfpn_cases.py: eval() and one train() step -- the pyramid levels, the
input gradient, every parameter gradient, the BatchNorm buffers afterwards, and the state_dict names and shapes.

Written to tests/golden/dfpn_small.npz (keys as tests/blocks_cases.pack writes them, per case: <case>/<mode>/y<i>, <case>/<mode>/dx0,
<case>/<mode>/dp/<name>, <case>/buffers/<name>, <case>/state_names, <case>/state_shapes).

Uses tools/gen_golden.py's import shims (runs only where the reference tree is present).
Usage:  python tools/gen_golden_dfpn.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools import gen_golden   # noqa: E402,F401  (shims first: torch.jit.scope, the stubbed third-party modules)

sys.path.insert(0, os.path.join(REPO, 'tests'))
import dfpn_cases                                    # noqa: E402
from bf.modules import features as ref_features      # noqa: E402


def gen(out_dir):
    res = {}
    for name in dfpn_cases.CASES:
        res.update(dfpn_cases.run_case(name, ref_features.DepthwiseFeaturePyramid, torch.device('cpu')))
    path = os.path.join(out_dir, 'dfpn_small.npz')
    np.savez_compressed(path, **res)
    print(f'dfpn -> {path} ({os.path.getsize(path) / 1e3:.1f} KB, {len(res)} arrays)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    gen(args.out)


if __name__ == '__main__':
    main()
