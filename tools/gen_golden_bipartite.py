#!/usr/bin/env python3
"""Golden vectors of bipartite matching, produced by RUNNING THE REFERENCE'S ``match_bipartite`` (detection/matcher.py:7-31) on the CPU on
the cases of tests/bipartite_cases.py.

Written to tests/golden/bipartite.npz:
  matrix/<case>/anchor_idx, matrix/<case>/box_idx   the reference's outputs (int64)
  matrix/<case>/inplace                             the matrix the reference leaves with inplace=True
  matrix/<case>/defined                             exhaustion cases only: the entries of anchor_idx the reference's loop wrote (the rest
                                                    is torch.empty's); found with bipartite_cases.match_bipartite_np, values from the reference
  fused/<case>/box_idx                              int32 [B, A]: per image match_per_prediction(iou, matched, unmatched,
                                                    force_match_for_each_target=False), then box_idx[anchor_idx] = box_idx_b with
                                                    match_bipartite(iou), iou = box_utils.iou(gt[:, :4], to_corners(anchors)); an
                                                    image without boxes is NOT_MATCHED throughout (target_assigner.py:36-41)
The tool asserts what the cases are for: the fused cases collide (boxes lose their forced anchor under the default rule) where the case
table says so and never exhaust; the exhaustion cases do exhaust.

Uses tools/gen_golden.py's import shims (runs only where the reference tree is present).
Usage:  python tools/gen_golden_bipartite.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools import gen_golden   # noqa: E402,F401  (shims first: the stubbed third-party modules)

sys.path.insert(0, os.path.join(REPO, 'tests'))
import bipartite_cases as bc                         # noqa: E402
from bf.utils import box_utils as ref_box_utils      # noqa: E402
from detection import matcher as ref_matcher         # noqa: E402


def gen(out_dir):
    res = {}
    for name, make in bc.MATRIX_CASES.items():
        w = make()
        box_idx, anchor_idx = ref_matcher.match_bipartite(torch.from_numpy(w.copy()))
        left = torch.from_numpy(w.copy())
        box_idx2, anchor_idx2 = ref_matcher.match_bipartite(left, inplace=True)
        mine, mine_left = bc.match_bipartite_np(w)
        defined = mine >= 0
        assert (not defined.all()) == (name in bc.EXHAUSTED), name
        assert torch.equal(box_idx, box_idx2) and np.array_equal(anchor_idx.numpy()[defined], anchor_idx2.numpy()[defined]), name
        res[f'matrix/{name}/box_idx'] = box_idx.numpy()
        res[f'matrix/{name}/anchor_idx'] = np.where(defined, anchor_idx.numpy(), 0)   # (undefined entries: stored as 0, masked by `defined`)
        res[f'matrix/{name}/inplace'] = left.numpy()
        if name in bc.EXHAUSTED:
            res[f'matrix/{name}/defined'] = defined
    for name, case in bc.FUSED_CASES.items():
        gt_list, anchors, mt, ut = bc.fused_inputs(name)
        corners = ref_box_utils.to_corners(torch.from_numpy(anchors))
        out = torch.full((len(gt_list), anchors.shape[0]), ref_matcher.NOT_MATCHED, dtype=torch.long)
        collisions = []
        for i, gt in enumerate(gt_list):
            if not len(gt):
                continue
            iou = ref_box_utils.iou(torch.from_numpy(gt)[:, 0:4], corners)
            box_idx = ref_matcher.match_per_prediction(iou, mt, ut, force_match_for_each_target=False)
            assert (bc.force_bipartite_np(iou.numpy()) >= 0).all(), f'{name}: image {i} exhausts'
            box_idx_b, anchor_idx = ref_matcher.match_bipartite(iou)
            assert np.array_equal(anchor_idx.numpy(), bc.force_bipartite_np(iou.numpy())), (name, i)
            box_idx[anchor_idx] = box_idx_b
            out[i] = box_idx
            collisions.append(len(bc.lost_forced_anchor(iou.numpy())))
        assert not case[6] or sum(collisions) >= 1, f'{name}: no collision in any image ({collisions})'
        print(f'fused/{name}: boxes that lose their forced anchor under the default rule, per image: {collisions}')
        res[f'fused/{name}/box_idx'] = out.numpy().astype(np.int32)
    path = os.path.join(out_dir, 'bipartite.npz')
    np.savez_compressed(path, **res)
    print(f'bipartite -> {path} ({os.path.getsize(path) / 1e3:.1f} KB, {len(res)} arrays)')
    assert os.path.getsize(path) < 300e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    gen(args.out)


if __name__ == '__main__':
    main()
