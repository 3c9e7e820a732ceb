"""Cases of bipartite matching (detection/matcher.py:7-31) shared by ``tools/gen_golden_bipartite.py``, which runs them through the
reference's ``match_bipartite`` on the CPU and writes ``tests/golden/bipartite.npz``, and by ``tests/test_bipartite*.py``; and a numpy
restatement of both semantics (the matrix form with the reference's behaviour on exhaustion, the fused force stage that stops there),
which ``tests/test_bipartite.py`` pins to those goldens so that randomised GPU checks may use it.  Inputs are seeded, not stored."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _same_rows(g, a, seed):
    row = np.random.default_rng(seed).random(a, dtype=np.float32)
    return np.tile(row, (g, 1))


def _iou_like(g, a, seed):
    """Sparse matrix in [0, 1) whose values sit on a 1/16 grid in many columns (ties inside rows, between rows, duplicated maxima);
    every row has a positive entry."""
    rng = np.random.default_rng(seed)
    w = rng.random((g, a), dtype=np.float32) * (rng.random((g, a)) < 0.3)
    w[:, ::3] = np.round(w[:, ::3] * 16) / 16
    w[np.arange(g), rng.integers(0, a, g)] = np.float32(0.9375)   # the maximum of most rows, often in a column another row shares
    w[7] = w[3]
    return np.ascontiguousarray(w, dtype=np.float32)


# name -> matrix [Boxes, AnchorBoxes].  Every row has a positive entry (the reference asserts it).
MATRIX_CASES = {
    'one': lambda: np.array([[0.7]], np.float32),
    'tie_in_row': lambda: np.array([[0.2, 0.9, 0.9, 0.1], [0.5, 0.3, 0.2, 0.8]], np.float32),          # the lowest column
    'tie_between_rows': lambda: np.array([[0.3, 0.9, 0.2], [0.5, 0.9, 0.1]], np.float32),              # the lowest row
    'same_rows_3x5': lambda: _same_rows(3, 5, 31),                                                      # the longest rescan chain
    'same_rows_40x700': lambda: _same_rows(40, 700, 32),
    'exhaust_5x3': lambda: np.random.default_rng(33).random((5, 3), dtype=np.float32) + np.float32(0.01),   # Boxes > AnchorBoxes
    'exhaust_shared_column': lambda: np.array([[0, 0, 0.6, 0], [0, 0, 0.4, 0]], np.float32),           # anchors to spare
    'exhaust_shared_column_row0_kept': lambda: np.array([[0.1, 0.9, 0, 0], [0, 0, 0.6, 0], [0, 0, 0.4, 0]], np.float32),
    'random_130x700_a': lambda: _iou_like(130, 700, 34),       # beyond the 128-box chunk and one 512-anchor segment
    'random_130x700_b': lambda: _iou_like(130, 700, 35),
}
EXHAUSTED = ('exhaust_5x3', 'exhaust_shared_column', 'exhaust_shared_column_row0_kept')

# name -> (anchors of tests/golden/<config>.npz, batch, make_ground_truth keywords, emptied image or None, matched, unmatched, collisions asserted)
FUSED_CASES = {
    'mb2_g32': ('ssd_mb2_voc', 4, dict(seed=1, fixed_g=32), None, 0.5, 0.5, True),
    'mb2_g140': ('ssd_mb2_voc', 4, dict(seed=1, fixed_g=140), None, 0.5, 0.4, True),
    'retina_g32': ('retina_rn50_500_coco', 2, dict(seed=1, fixed_g=32), None, 0.5, 0.4, True),     # 47 961 anchors: several argmax segments
    'mb2_default_one_empty': ('ssd_mb2_voc', 3, dict(seed=1), 1, 0.5, 0.5, False),
}


def fused_inputs(name):
    """(gt list of [G_i, 6] fp32, anchors [A, 4] fp32, matched, unmatched)."""
    from single_shot_detection_amd import synthetic as syn
    config, batch, kw, emptied, mt, ut, _ = FUSED_CASES[name]
    cfg = syn.CONFIGS[config]
    gt = syn.make_ground_truth(batch, cfg['size'], cfg['num_classes'], **kw)
    if emptied is not None:
        gt[emptied] = np.zeros((0, 6), np.float32)
    anchors = np.load(os.path.join(GOLDEN, f'{config}.npz'))['anchors']
    return gt, anchors, mt, ut


def load_golden():
    return dict(np.load(os.path.join(GOLDEN, 'bipartite.npz')))


# ---- numpy restatement ---------------------------------------------------------------------------------------------------------------
def match_bipartite_np(weights):
    """The matrix form: (anchor_idx int64 [G] with -1 where the loop never wrote, the matrix the loop leaves).  Boxes rounds; after
    exhaustion np.argmax of the all-zero matrix is flat index 0, so anchor_idx[0] = 0."""
    w = np.array(weights, dtype=np.float32, copy=True)
    g, a = w.shape
    anchor_idx = np.full((g,), -1, np.int64)
    for _ in range(g):
        r, c = divmod(int(np.argmax(w)), a)     # first flat index on ties
        anchor_idx[r] = c
        w[:, c] = 0
        w[r] = 0
    return anchor_idx, w


def force_bipartite_np(iou):
    """The fused force stage: as above, but it stops at the first maximum that is not above 0; -1 = no forced anchor."""
    w = np.array(iou, dtype=np.float32, copy=True)
    g, a = w.shape
    w[np.isnan(w)] = 0
    anchor_idx = np.full((g,), -1, np.int64)
    for _ in range(g):
        r, c = divmod(int(np.argmax(w)), a)
        if not w[r, c] > 0:
            break
        anchor_idx[r] = c
        w[:, c] = 0
        w[r] = 0
    return anchor_idx


def encode_bipartite_np(gt_list, anchors, matched, unmatched):
    """box_idx int32 [B, A] of TargetAssigner(matched, unmatched, force_match='bipartite'): match_per_prediction without force-matching,
    then box_idx[anchor_idx] = arange(G).  The IoU matrix and the threshold stage are the oracle's (bit-exact with the reference)."""
    import oracle
    corners = oracle.to_corners(anchors)
    out = np.full((len(gt_list), anchors.shape[0]), -2, np.int32)
    for i, gt in enumerate(gt_list):
        if not len(gt):
            continue
        iou = oracle.iou(np.ascontiguousarray(gt[:, :4]), corners)
        idx = np.asarray(oracle.match_per_prediction(iou, matched, unmatched, False)).astype(np.int32)
        forced = force_bipartite_np(iou)
        idx[forced[forced >= 0]] = np.nonzero(forced >= 0)[0]
        out[i] = idx
    return out


def lost_forced_anchor(iou):
    """Boxes that share their best anchor with a box of higher index (they lose it under the default rule, matcher.py:52-54)."""
    best = np.argmax(iou, axis=1)
    return [g for g in range(len(best)) if (best[g + 1:] == best[g]).any()]


def target_from_box_idx(box_idx, gt_list):
    """target fp32 [B, A, 6] from the matcher's box_idx (target_assigner.py:39-40, 52-58)."""
    b, a = box_idx.shape
    target = np.zeros((b, a, 6), np.float32)
    target[..., 5] = 1.0
    for i, gt in enumerate(gt_list):
        pos = box_idx[i] >= 0
        target[i, pos] = gt[box_idx[i][pos], :6]
        target[i, box_idx[i] == -1, 4:6] = -1.0
    return target
