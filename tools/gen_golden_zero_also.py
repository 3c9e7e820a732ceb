#!/usr/bin/env python3
"""Records what THIS build computes for the block of tests/zero_also_cases.py in deterministic mode, as tests/golden/zero_also_det.npz:
    python tools/gen_golden_zero_also.py [out.npz]
The fixture in the repository was written by the build of the commit before the zero-fill moved into the norm's backward apply launch:
deterministic mode must keep taking the path of that commit, bit for bit (tests/test_batchnorm_zero_also_gpu.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import zero_also_cases as cases
    from single_shot_detection_amd import ops
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'zero_also_det.npz')
    m, x, g = cases.block_and_input()
    with ops.deterministic():
        grads = cases.gradients(m, x, g, 'cuda')
    np.savez(out, **grads)
    print('wrote', out, {k: v.shape for k, v in grads.items()})


if __name__ == '__main__':
    main()
