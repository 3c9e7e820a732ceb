#!/usr/bin/env python3
"""Golden vectors of the depthwise RetinaNet-lite tower, produced by RUNNING THE REFERENCE'S ``SharedConvPredictor(use_depthwise=True)``
(detection/modules/predictors.py:8-76 over bf/modules/conv.py:39-85) on the CPU, on the cases of tests/dwtower_cases.py: eval() and one
train() step -- both towers' outputs per level, the input gradients, every parameter gradient, the BatchNorm buffers afterwards, and the
state_dict names and shapes.

Written to tests/golden/tower_depthwise.npz (keys as tests/blocks_cases.pack writes them, per case: <case>/<mode>/y<i>, <case>/<mode>/dx<i>,
<case>/<mode>/dp/<name>, <case>/buffers/<name>, <case>/state_names, <case>/state_shapes).

Before writing, the same graph is run in float64 and the fp32 fixture is held to it: the GPU test compares at 2e-5, so the fixture's own
distance from the exact result has to be well inside that (printed; the generator refuses above a quarter of the bar).

Uses tools/gen_golden.py's import shims (runs only where the reference tree is present).
Usage:  python tools/gen_golden_dwtower.py [--out tests/golden]
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
import dwtower_cases                                              # noqa: E402
from detection.modules import predictors as ref_predictors        # noqa: E402

BAR = 2e-5


def gen(out_dir):
    res = {}
    for name in dwtower_cases.CASES:
        got = dwtower_cases.run_case(name, ref_predictors.SharedConvPredictor, torch.device('cpu'))
        exact = dwtower_cases.run_case(name, ref_predictors.SharedConvPredictor, torch.device('cpu'), dtype=torch.float64)
        ratio, key = dwtower_cases.worst_ratio(got, exact, BAR)
        print(f'{name}: fp32 against float64, worst entry at {ratio:.3f} of the {BAR:g} bar ({key})')
        assert ratio <= 0.25, 'the inputs of this case are ill-conditioned for a 2e-5 comparison: change them, not the bar'
        res.update(got)
    path = os.path.join(out_dir, 'tower_depthwise.npz')
    np.savez_compressed(path, **res)
    print(f'depthwise tower -> {path} ({os.path.getsize(path) / 1e3:.1f} KB, {len(res)} arrays)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    gen(args.out)


if __name__ == '__main__':
    main()
