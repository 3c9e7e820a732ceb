"""The torch loss options of MultiboxLoss (CrossEntropyLoss label_smoothing / weight, L1Loss, MSELoss, HuberLoss, SmoothL1Loss beta=0):
the cases of tests/golden/losses_torch.npz (tools/gen_golden_losses_torch.py) and a torch-CPU restatement of
detection/losses/multibox_loss.py:59-94 built on torch's own loss modules, shared by test_loss_torch_kinds.py (CPU) and
test_loss_torch_kinds_gpu.py."""
import torch
import torch.nn as nn

WEIGHT = 'class_weight'   # stands for the golden file's per-class weights in a case's classification_loss

CASES = {   # tag: (sampler, classification_loss, localization_loss) -- as tools/gen_golden_losses_torch.py runs them
    'ce_smooth': ('hnm', {'name': 'CrossEntropyLoss', 'label_smoothing': 0.1}, {'name': 'SmoothL1Loss'}),
    'ce_weight': ('hnm', {'name': 'CrossEntropyLoss', 'weight': WEIGHT}, {'name': 'SmoothL1Loss'}),
    'ce_smooth_weight': ('hnm', {'name': 'CrossEntropyLoss', 'label_smoothing': 0.2, 'weight': WEIGHT}, {'name': 'SmoothL1Loss'}),
    'ce_smooth_weight_naive': ('naive', {'name': 'CrossEntropyLoss', 'label_smoothing': 0.2, 'weight': WEIGHT}, {'name': 'SmoothL1Loss'}),
    'l1_hnm': ('hnm', {'name': 'CrossEntropyLoss'}, {'name': 'L1Loss'}),
    'l1_naive': ('naive', {'name': 'CrossEntropyLoss'}, {'name': 'L1Loss'}),
    'mse_hnm': ('hnm', {'name': 'CrossEntropyLoss'}, {'name': 'MSELoss'}),
    'mse_naive': ('naive', {'name': 'CrossEntropyLoss'}, {'name': 'MSELoss'}),
    'huber_hnm': ('hnm', {'name': 'CrossEntropyLoss'}, {'name': 'HuberLoss', 'delta': 0.5}),
    'huber_naive': ('naive', {'name': 'CrossEntropyLoss'}, {'name': 'HuberLoss', 'delta': 0.5}),
    'smooth_l1_beta0_hnm': ('hnm', {'name': 'CrossEntropyLoss'}, {'name': 'SmoothL1Loss', 'beta': 0.0}),
    'smooth_l1_beta0_naive': ('naive', {'name': 'CrossEntropyLoss'}, {'name': 'SmoothL1Loss', 'beta': 0.0}),
    'ce_smooth_l1': ('hnm', {'name': 'CrossEntropyLoss', 'label_smoothing': 0.1}, {'name': 'L1Loss'}),
}


def with_weight(cfg, weight):
    """a case's loss config with the WEIGHT marker replaced by the tensor ``weight``"""
    return {k: (weight if v is WEIGHT else v) for k, v in cfg.items()}


def encode_target(target, anchors, xy_scale=10.0, wh_scale=5.0, eps=1e-8):
    """multibox_loss.py:81-82 on a copy: to_centroids(inplace) + encode_box(inplace), in the reference's order of operations
    (box_utils.py:33-34, box_coder.py:22-30)."""
    t = target.clone()
    b, p = t[..., :4], anchors.unsqueeze(0)
    b[..., 2:] -= b[..., :2]
    b[..., :2] += b[..., 2:] / 2
    b[..., :2] -= p[..., :2]
    b[..., :2] /= p[..., 2:]
    b[..., :2] *= xy_scale
    b[..., 2:] /= p[..., 2:]
    b[..., 2:] += eps
    b[..., 2:].log_()
    b[..., 2:] *= wh_scale
    return t


def torch_multibox_loss(scores, locs, encoded_target, mask, classification_loss, localization_loss, classification_weight=1.0,
                        localization_weight=1.0):
    """(loss, class_loss, loc_loss) of multibox_loss.py:59-94 for a given sampled mask [B, A] (bool), on CPU with torch's own
    CrossEntropyLoss / L1Loss / MSELoss / HuberLoss / SmoothL1Loss (reduction='sum' and ignore_index=-1, as :23-30 construct them).
    scores [B, A * C] and locs [B, A * 4] may require grad; encoded_target is the target after the in-place encode."""
    B, A = encoded_target.shape[:2]
    scores = scores.view(B, A, -1)
    locs = locs.view(B, A, 4)
    cls = encoded_target[..., 4].long()
    positive = (cls != 0) & (cls != -1)
    cl = {k: v for k, v in classification_loss.items() if k != 'name'}
    ll = {k: v for k, v in localization_loss.items() if k != 'name'}
    class_loss = getattr(nn, classification_loss['name'])(reduction='sum', ignore_index=-1, **cl)(scores[mask], cls[mask])
    loc_loss = getattr(nn, localization_loss['name'])(reduction='sum', **ll)(locs[positive].view(-1, 4),
                                                                             encoded_target[..., :4][positive].view(-1, 4))
    divider = positive.sum().clamp(min=1).float()
    class_loss = class_loss * classification_weight / divider
    loc_loss = loc_loss * localization_weight / divider
    return class_loss + loc_loss, class_loss, loc_loss
