#!/usr/bin/env python3
"""Golden vectors for the torch loss options MultiboxLoss accepts by name, produced by RUNNING THE REFERENCE'S MultiboxLoss on CPU.

The reference re-exports ``torch.nn.modules.loss`` (bf/modules/losses.py:4) and builds the configured losses through get_ctor +
filter_kwargs (detection/losses/multibox_loss.py:23-30), so a config may pass CrossEntropyLoss ``label_smoothing`` / ``weight`` and pick
L1Loss, MSELoss, HuberLoss (``delta``) or SmoothL1Loss with ``beta=0`` for the box term.  One case per configuration -- smoothing, weights,
both, and each box kind under both samplers -- on the ssd_mb2_voc anchors at batch 2 with the inputs of ``losses_extra.npz``
(synthetic logits seed 2, locs seed 3, ground truth seed 1 matched at 0.5 / 0.5).

Written to tests/golden/losses_torch.npz:
  target                  the matched [B, A, 6] target handed to the loss
  target_encoded          the target after the forward (columns 0..3 encoded in place, multibox_loss.py:81-82; the same for every case)
  class_weight            the per-class weights of the weighted cases (fp32 [C], seeded)
  <tag>_values            (loss, class_loss, loc_loss)
  <tag>_sampled_bits      the sampler's mask, np.packbits along the anchors
  <tag>_dscores_rows/vals d loss / d scores, the non-zero rows only (indices [n, 2], values [n, C])
  <tag>_dlocs_rows/vals   d loss / d locs, the same way

Uses tools/gen_golden.py's import shims (runs only where the reference tree is present).
Usage:  python tools/gen_golden_losses_torch.py [--out tests/golden]
"""
import argparse
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import gen_golden as gg   # noqa: E402  (shims + the reference's modules)

NUM_CLASSES = 21


def cases(class_weight):
    """tag -> (sampler, classification_loss, localization_loss) -- the configs as a user writes them."""
    hnm = functools.partial(gg.sampler.hard_negative_mining, negative_per_positive_ratio=3, min_negative_per_image=5)
    naive = gg.sampler.naive_sampler
    ce = {'name': 'CrossEntropyLoss'}
    sl1 = {'name': 'SmoothL1Loss'}
    return {
        'ce_smooth': (hnm, {'name': 'CrossEntropyLoss', 'label_smoothing': 0.1}, sl1),
        'ce_weight': (hnm, {'name': 'CrossEntropyLoss', 'weight': class_weight}, sl1),
        'ce_smooth_weight': (hnm, {'name': 'CrossEntropyLoss', 'label_smoothing': 0.2, 'weight': class_weight}, sl1),
        'ce_smooth_weight_naive': (naive, {'name': 'CrossEntropyLoss', 'label_smoothing': 0.2, 'weight': class_weight}, sl1),
        'l1_hnm': (hnm, ce, {'name': 'L1Loss'}),
        'l1_naive': (naive, ce, {'name': 'L1Loss'}),
        'mse_hnm': (hnm, ce, {'name': 'MSELoss'}),
        'mse_naive': (naive, ce, {'name': 'MSELoss'}),
        'huber_hnm': (hnm, ce, {'name': 'HuberLoss', 'delta': 0.5}),
        'huber_naive': (naive, ce, {'name': 'HuberLoss', 'delta': 0.5}),
        'smooth_l1_beta0_hnm': (hnm, ce, {'name': 'SmoothL1Loss', 'beta': 0.0}),
        'smooth_l1_beta0_naive': (naive, ce, {'name': 'SmoothL1Loss', 'beta': 0.0}),
        'ce_smooth_l1': (hnm, {'name': 'CrossEntropyLoss', 'label_smoothing': 0.1}, {'name': 'L1Loss'}),
    }


def gen(out_dir):
    res = {}
    cfg = gg.syn.CONFIGS['ssd_mb2_voc']
    C, B = cfg['num_classes'], 2
    assert C == NUM_CLASSES
    anchors = gg.ref_anchors(cfg)
    A = anchors.shape[0]
    gt = gg.syn.make_ground_truth(B, cfg['size'], C, seed=1)
    _, target = gg.ref_match(gt, anchors, 0.5, 0.5)
    res['target'] = target.numpy()
    class_weight = np.random.default_rng(91).uniform(0.25, 2.0, C).astype(np.float32)
    res['class_weight'] = class_weight
    encoded = None
    for tag, (smp, cl, ll) in cases(torch.from_numpy(class_weight)).items():
        logits = torch.from_numpy(gg.syn.make_logits(B, A, C, seed=2)).requires_grad_(True)
        locs = torch.from_numpy(gg.syn.make_locs(B, A, seed=3, scale=0.5)).requires_grad_(True)
        crit = gg.MultiboxLoss(sampler=smp, box_coder=gg.BoxCoder(10.0, 5.0), classification_loss=cl, localization_loss=ll,
                               classification_weight=1.0, localization_weight=1.0)
        tgt = target.clone()
        mask = crit.sampler(logits.detach().view(B, A, C), tgt[..., 4].long())
        loss, cl_, ll_ = crit((logits, locs), anchors, tgt)
        loss.backward()
        if encoded is None:
            encoded = tgt.numpy().copy()
        assert np.array_equal(encoded, tgt.numpy()), tag   # every kind here mutates the target the same way
        res[tag + '_values'] = np.array([loss.item(), cl_.item(), ll_.item()], dtype=np.float64)
        res[tag + '_sampled_bits'] = np.packbits(mask.numpy().astype(np.uint8), axis=1)
        gi, gv = gg.sparse_rows(logits.grad.view(B, A, C)); res[tag + '_dscores_rows'], res[tag + '_dscores_vals'] = gi, gv
        gi, gv = gg.sparse_rows(locs.grad.view(B, A, 4)); res[tag + '_dlocs_rows'], res[tag + '_dlocs_vals'] = gi, gv
    res['target_encoded'] = encoded
    path = os.path.join(out_dir, 'losses_torch.npz')
    np.savez_compressed(path, **res)
    print(f'losses_torch -> {path} ({os.path.getsize(path) / 1e3:.1f} KB)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(gg.REPO, 'tests', 'golden'))
    gen(ap.parse_args().out)


if __name__ == '__main__':
    main()
