"""The sampled-path loss kernels of csrc/loss.hip (loss_fwd_kernel<LK,CEX> / loss_bwd_kernel<LK,CEX>, the hard-negative-mining kernels, the
box coder): an fp64 torch-CPU restatement of detection/losses/multibox_loss.py:59-94 for a GIVEN mask, an fp64 restatement of
detection/sampler.py:12-25, a deterministic case builder, the tolerances, and the list of every run that tests/test_loss_kernels_gpu.py makes --
which tests/test_loss_reference.py evaluates in fp32 on the CPU, so that a tolerance the GPU file applies is one that plain fp32 torch meets
on the same inputs.

The box term of the SmoothL1 family is taken against a given encoded target (``encoded=``: what the kernel -- or fp32 torch -- wrote into
the target's columns 0..3), as tests/quality_loss_cases.py and tests/test_loss_torch_kinds_gpu.py do: the encode is compared with the fp64
one on its own (rtol 1e-6, atol 2e-5), and an error of that size in the target would otherwise sit in dlocs = (l - t) / beta at 1e-5."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import quality_loss_cases as qc
from loss_torch_cases import encode_target

XY_SCALE, WH_SCALE, EPS = qc.XY_SCALE, qc.WH_SCALE, qc.EPS
CLASS_W, LOC_W, GRAD_OUT = 0.7, 1.3, (2.0, 0.5)       # non-unit weights and upstream gradients of every run

# ---- tolerances (all against fp64) -----------------------------------------------------------------------------------------------------
VALUES_RTOL = 1e-5                                    # |got - ref| <= 1e-5 * (the term's fp64 sum of absolute per-row contributions)
DSCORES = dict(rtol=3e-4, atol=3e-7)
DLOCS = {'smooth_l1': dict(rtol=1e-5, atol=1e-8), 'giou': dict(rtol=3e-4, atol=3e-7)}
TARGET = dict(rtol=1e-6, atol=2e-5)
KINK = 1e-3                                           # GIoU rows with a predicted corner this close to the target's: finite only

SOFTMAX_KINDS = ('ce', 'softmax_focal', 'ce_soft')    # positives 1..C-1; the sigmoid kinds ('sigmoid_focal', 'bce_soft'): 1..C
FOCAL_KINDS = ('sigmoid_focal', 'softmax_focal')


# ---- classification / box specs ---------------------------------------------------------------------------------------------------------
def class_weights(C, zeros=False):
    """CrossEntropyLoss ``weight`` of a spec with weight=True (with zeros: every third class weighs nothing)."""
    w = np.linspace(0.5, 2.0, C, dtype=np.float32) if C > 1 else np.array([0.75], np.float32)
    if zeros:
        w = w.copy()
        w[::3] = 0.0
    return w


CLS = {
    'ce': dict(kind='ce'),
    'ce_ls': dict(kind='ce', label_smoothing=0.1),
    'ce_w': dict(kind='ce', weight='plain'),
    'ce_ls_w': dict(kind='ce', label_smoothing=0.2, weight='plain'),
    'sigmoid_focal': dict(kind='sigmoid_focal', gamma=2.0, alpha=0.25),
    'softmax_focal': dict(kind='softmax_focal', gamma=2.0, alpha=0.25),
    'softmax_focal_noalpha': dict(kind='softmax_focal', gamma=1.5, alpha=None),
    'ce_soft': dict(kind='ce_soft', epsilon=0.0),
    'ce_soft_eps': dict(kind='ce_soft', epsilon=0.1),
    'bce_soft': dict(kind='bce_soft', epsilon=0.0),
    'bce_soft_eps': dict(kind='bce_soft', epsilon=0.1),
}
BOX = {
    'smooth_l1': dict(kind='smooth_l1', beta=1.0),
    'l1': dict(kind='smooth_l1', beta=0.0),            # torch: SmoothL1Loss(beta=0) is L1Loss
    'mse': dict(kind='mse'),
    'huber': dict(kind='huber', beta=0.5),
    'giou': dict(kind='giou'),
}


def box_family(box):
    return 'giou' if box['kind'] == 'giou' else 'smooth_l1'


def hard_label(cls):
    return cls['kind'] in ('ce', 'softmax_focal')


def spec_weight(cls, C):
    w = cls.get('weight')
    if w is None or isinstance(w, np.ndarray):
        return w
    return class_weights(C, zeros=(w == 'zeros'))


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------
def _soften(t, eps):
    """bf/modules/losses.py:28-32, out of place."""
    pos = (t > 0).to(t.dtype)
    t = t + (1.0 - pos) * eps * t.sum(-1, keepdim=True) / (t.size(1) - pos.sum(-1, keepdim=True))
    return t - pos * eps * t


def restatement(target, scores, locs, anchors, mask, cls, box, classification_weight=1.0, localization_weight=1.0, reduce_mean=1,
                dtype=torch.float64, grad_out=(1.0, 1.0), encoded=None):
    """multibox_loss.py:59-94 for the sampled mask ``mask`` [B, A], everything in ``dtype`` on the CPU.  target: the RAW [B, A, 6] target;
    scores [B, A * C]; locs [B, A * 4]; anchors [A, 4]; cls / box: specs as in CLS / BOX; reduce_mean 0: sums, 1: the focal kinds' 'mean' over
    the sampled rows, 2: sums that are not divided by the positives.  Returns a dict: values [3] (loss, class_loss, loc_loss), dscores and
    dlocs (autograd of grad_out[0] * class_loss + grad_out[1] * loc_loss), target (the encoded target; the raw one under GIoU), sabs [3] (per
    term the sum of the absolute per-row contributions after the same scaling)."""
    B, A = target.shape[:2]
    target, anchors = target.detach().to(dtype), anchors.detach().to(dtype)
    s = scores.detach().to(dtype).clone().requires_grad_(True)
    l = locs.detach().to(dtype).clone().requires_grad_(True)
    x = s.view(B, A, -1)
    C = x.shape[-1]
    cls_col = target[..., 4].long()                                                       # multibox_loss.py:48
    positive = (cls_col != 0) & (cls_col != -1)
    m = torch.as_tensor(mask).bool()
    xs, cs, ts = x[m], cls_col[m], target[..., 5][m]
    n = xs.shape[0]
    kind = cls['kind']
    rows_ix = torch.arange(n)
    if kind == 'ce':
        w = spec_weight(cls, C)
        rows = F.cross_entropy(xs, cs, weight=None if w is None else torch.from_numpy(w).to(dtype), ignore_index=-1, reduction='none',
                               label_smoothing=float(cls.get('label_smoothing', 0.0))) if n else xs.sum(-1)
    elif kind == 'softmax_focal':                                                         # losses.py:63-78
        valid = cs != -1
        logpb = F.log_softmax(xs, dim=-1)[rows_ix[valid], cs[valid]]
        val = -1 * (1.0 - logpb.exp()).pow(cls['gamma']) * logpb
        if cls.get('alpha') is not None:
            val = val * torch.where(cs[valid] == 0, 1.0 - cls['alpha'], cls['alpha']).to(dtype)
        rows = torch.zeros(n, dtype=dtype).index_put((rows_ix[valid],), val)
    else:
        t = torch.zeros_like(xs)
        if kind == 'ce_soft':                                                             # multibox_loss.py:68-71
            sel = cs != -1
            t[rows_ix[sel], cs[sel]] = ts[sel]
        else:                                                                             # multibox_loss.py:64-67
            sel = (cs != 0) & (cs != -1)
            t[rows_ix[sel], cs[sel] - 1] = ts[sel]
        if kind == 'sigmoid_focal':
            rows = qc.sigmoid_focal(xs, t, cls['gamma'], cls['alpha']).sum(-1)
        else:
            if cls.get('epsilon'):
                t = _soften(t, cls['epsilon'])
            if kind == 'ce_soft':                                                         # losses.py:83-93
                rows = -1 * t.sum(-1).mean().pow(-1) * (F.log_softmax(xs, dim=-1) * t).sum(-1)
            else:                                                                         # losses.py:99-106
                sc = t.mean(-1)
                rows = (sc.sum() / (sc > 0).to(dtype).sum()).pow(-1) * qc.bce(xs, t).sum(-1)
    if kind in FOCAL_KINDS and reduce_mean == 1:
        rows = rows / n
    if box['kind'] == 'giou':                                                             # multibox_loss.py:77-79
        brows = qc.giou_loss(qc.decode_corners(l.view(B, A, 4), anchors)[positive], target[..., :4][positive])
        enc = target
    else:                                                                                 # multibox_loss.py:81-86
        enc = encode_target(target, anchors, XY_SCALE, WH_SCALE, EPS)
        e = enc if encoded is None else torch.as_tensor(encoded).to(dtype)
        a, b = l.view(B, A, 4)[positive], e[..., :4][positive]
        if box['kind'] == 'smooth_l1':
            brows = F.smooth_l1_loss(a, b, reduction='none', beta=box['beta']).sum(-1)
        elif box['kind'] == 'mse':
            brows = F.mse_loss(a, b, reduction='none').sum(-1)
        else:
            brows = F.huber_loss(a, b, reduction='none', delta=box['beta']).sum(-1)
    divider = 1.0 if reduce_mean == 2 else float(max(int(positive.sum()), 1))            # multibox_loss.py:88
    class_loss = rows.sum() * classification_weight / divider
    loc_loss = brows.sum() * localization_weight / divider
    (grad_out[0] * class_loss + grad_out[1] * loc_loss).backward()
    sabs_c = float(rows.detach().abs().sum()) * abs(classification_weight) / divider
    sabs_l = float(brows.detach().abs().sum()) * abs(localization_weight) / divider
    return dict(values=np.array([float((class_loss + loc_loss).detach()), float(class_loss.detach()), float(loc_loss.detach())]),
                dscores=(s.grad if s.grad is not None else torch.zeros_like(s)).numpy(),
                dlocs=(l.grad if l.grad is not None else torch.zeros_like(l)).numpy(),
                target=enc.numpy(), sabs=np.array([sabs_c + sabs_l, sabs_c, sabs_l]))


def giou_kink(case):
    """bool [B, A]: positives with a decoded corner coordinate within KINK of the target's (the max / min of box_utils.py:104-143 switch
    sides there: the gradient is one-sided, fp32 and fp64 may take different sides)."""
    B, A = case['B'], case['A']
    cls = case['target'][..., 4].long()
    positive = (cls != 0) & (cls != -1)
    P = qc.decode_corners(case['locs'].double().view(B, A, 4), case['anchors'].double())
    T = case['target'][..., :4].double()
    d = torch.cat([(P - T).abs(), (P[..., :2] - T[..., 2:]).abs(), (P[..., 2:] - T[..., :2]).abs()], -1)   # (the last two: the clamp at 0 overlap)
    return positive & (d.min(-1).values < KINK)


def excess(got, ref, rtol, atol):
    """max over the elements of |got - ref| / (atol + rtol * |ref|): <= 1 is inside the tolerance; inf where ``got`` is not finite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def compare(got, ref, box, kink=None, what=''):
    """got / ref: dicts with values, dscores, dlocs (ref also sabs).  Asserts section by section; returns each error as a fraction of its
    tolerance."""
    fam = box_family(box)
    frac = {}
    v = []
    for k in range(3):
        err, tol = abs(float(got['values'][k]) - ref['values'][k]), VALUES_RTOL * ref['sabs'][k]
        assert np.isfinite(got['values'][k]), (what, 'values', got['values'])
        v.append(0.0 if err == 0.0 else (math.inf if tol == 0.0 else err / tol))
    frac['values'] = max(v)
    frac['dscores'] = excess(got['dscores'], ref['dscores'], **DSCORES)
    gd, rd = np.asarray(got['dlocs']).reshape(-1, 4), np.asarray(ref['dlocs']).reshape(-1, 4)
    if fam == 'giou' and kink is not None and bool(np.asarray(kink).any()):
        k = np.asarray(kink).reshape(-1)
        assert np.isfinite(gd[k]).all(), (what, 'kink rows')
        gd, rd = gd[~k], rd[~k]
    frac['dlocs'] = excess(gd, rd, **DLOCS[fam])
    print('FRAC', what, ' '.join(f'{k}={v:.3g}' for k, v in frac.items()), 'values', np.asarray(got['values']), ref['values'])
    assert frac['values'] <= 1.0, (what, 'values', got['values'], ref['values'], ref['sabs'], frac)
    assert frac['dscores'] <= 1.0, (what, 'dscores', frac)
    assert frac['dlocs'] <= 1.0, (what, 'dlocs', frac)
    return frac


# ---- hard negative mining ---------------------------------------------------------------------------------------------------------------
def mining_losses(scores, C):
    """-log_softmax[..., 0] in fp64 (sampler.py:13): [B, A]."""
    s = torch.as_tensor(scores).double()
    return (-F.log_softmax(s.reshape(s.shape[0], -1, C), dim=-1)[..., 0]).numpy()


def mining(scores, classes, ratio, min_neg, C=None, losses=None):
    """sampler.py:12-25 in fp64: n = min(max(P * ratio, min_neg), #neg) per image, a fractional n keeps ceil(n) ranks, ties go to the lower
    index, class -1 is never taken.  scores [B, A, C] (or ``losses`` [B, A], from mining_losses), classes [B, A] -> bool [B, A]."""
    classes = np.asarray(classes)
    loss = mining_losses(scores, C if C is not None else np.asarray(scores).shape[-1]) if losses is None else losses
    out = np.zeros(classes.shape, bool)
    for i in range(classes.shape[0]):
        neg = classes[i] == 0
        pos = (classes[i] != 0) & (classes[i] != -1)
        n = min(max(float(pos.sum()) * float(ratio), float(min_neg)), float(neg.sum()))
        keep = int(math.ceil(n))
        idx = np.nonzero(neg)[0]
        order = np.argsort(-(loss[i][idx] + 0.0), kind='stable')                       # descending, equal losses in index order
        out[i] = pos
        out[i][idx[order[:keep]]] = True
    return out


def sampler_classes(B, A, seed=0):
    """The class columns of the sampler tests, one image each (as far as B = 5 and A allow): 0 without positives, 1 where every negative is
    taken (most rows positive), 2 all ignored, 3 a few positives and ignored rows, 4 (the image whose proto rows are all identical) a few
    positives: all ties."""
    rng = np.random.default_rng([5, seed, A])
    cls = np.zeros((B, A), np.float32)
    cls[0, 3::11] = -1
    u = rng.random(A)
    cls[1] = np.where(u < 0.6, 2.0, np.where(u < 0.7, -1.0, 0.0))
    cls[2] = -1
    cls[3, 1::97] = 1
    cls[3, 5::211] = -1
    cls[4, 2::1000] = 1
    return cls


# ---- the case builder -------------------------------------------------------------------------------------------------------------------
N_PROTO = 24
PROTO_SEP = 1e-3


def prototypes(C, seed):
    """N_PROTO rows [N_PROTO, C] whose background losses differ pairwise by at least PROTO_SEP in fp64 (C >= 2; with C = 1 every loss is 0),
    and that separation."""
    for k in range(50):
        rng = np.random.default_rng(seed * 1000 + k)
        p = rng.standard_normal((N_PROTO, C), dtype=np.float32)
        p[:, 0] = np.linspace(-3.0, 3.0, N_PROTO, dtype=np.float32)
        if C == 1:
            return p, 0.0
        sep = float(np.diff(np.sort(mining_losses(p[None], C)[0])).min())
        if sep >= PROTO_SEP:
            return p, sep
    raise AssertionError(f'no prototypes with separation {PROTO_SEP} for C={C}')


MINING_PAIRS = ((3, 5), (2.5, 0), (0.5, 7), (3, 10 ** 6), (0, 0))    # (negative_per_positive_ratio, min_negative_per_image)


def proto_logits(B, A, C, seed=0):
    """[B, A, C] rows dealt from the prototypes; the last image has every row identical (all ties)."""
    return _logits('proto', np.random.default_rng([11, seed, B, A, C]), B, A, C, None, seed)


def _logits(regime, rng, B, A, C, label, seed):
    if regime in ('normal', 'wide'):
        return rng.standard_normal((B, A, C), dtype=np.float32) * np.float32(1.0 if regime == 'normal' else 10.0)
    if regime == 'proto':
        x = prototypes(C, seed)[0][rng.integers(0, N_PROTO, (B, A))]
        x[-1] = 0.5                                                                       # one image with every row identical
        return x
    assert regime == 'saturated'
    x = rng.standard_normal((B, A, C), dtype=np.float32) * np.float32(0.5)
    r = np.arange(B * A).reshape(B, A) % 6
    bi, ai = np.meshgrid(np.arange(B), np.arange(A), indexing='ij')
    rest = np.ma.masked_array(x, mask=np.arange(C)[None, None, :] == label[..., None])
    hi = rest.max(-1).filled(0.0).astype(np.float32)
    lo = rest.min(-1).filled(0.0).astype(np.float32)
    lab = x[bi, ai, label]
    lab = np.where(r == 0, hi + 40.0, lab)                                                 # the label logit 40 above the rest
    lab = np.where(r == 1, lo - 40.0, lab)                                                 # ... 40 below
    lab = np.where(r == 3, 87.0, lab)                                                      # single logits at +-87
    lab = np.where(r == 4, -87.0, lab)
    x[bi, ai, label] = lab.astype(np.float32)
    x = np.where((r == 2)[..., None], (0.25 * (ai % 5))[..., None].astype(np.float32), x)  # all logits equal
    other = (label + 1) % C
    x[bi, ai, other] = np.where(r == 5, 87.0, x[bi, ai, other]).astype(np.float32)         # +87 beside the label
    return x.astype(np.float32)


@functools.lru_cache(maxsize=64)
def build(B, A, C, regime='normal', seed=0, sigmoid=False, no_positive=False):
    """A deterministic case, tensors on the CPU in fp32: anchors [A, 4] (cx, cy, w, h; sizes positive), the raw target [B, A, 6] (valid corners
    on every row; classes 0, -1 and positives 1..C-1, or 1..C with ``sigmoid``; scores 1.0 and 0.6), scores [B, A * C], locs [B, A * 4].
    Coordinates lie on a grid of 1/4, so that the differences of the encode are exact and its error is the divide's and the log's."""
    rng = np.random.default_rng([seed, B, A, C, int(sigmoid)])
    anchors = np.concatenate([rng.integers(0, 1024, (A, 2)) / 4.0, rng.integers(40, 400, (A, 2)) / 4.0], 1).astype(np.float32)
    x1 = rng.integers(0, 800, (B, A, 2)) / 4.0
    target = np.zeros((B, A, 6), np.float32)
    target[..., 0:2] = x1
    target[..., 2:4] = x1 + rng.integers(16, 400, (B, A, 2)) / 4.0
    u = rng.random((B, A))
    top = C if sigmoid else C - 1
    pos = (u < 0.15) & (top >= 1) & (not no_positive)
    if top >= 1 and not no_positive:
        pos[0, 0] = True
    cls = np.zeros((B, A), np.float32)
    cls[pos] = rng.integers(1, max(top, 1) + 1, int(pos.sum()))
    cls[(u >= 0.15) & (u < 0.25) & ~pos] = -1
    target[..., 4] = cls
    target[..., 5] = np.where(rng.random((B, A)) < 0.5, 1.0, 0.6)
    label = np.where(cls > 0, cls - 1 if sigmoid else cls, 0).astype(np.int64)
    scores = _logits(regime, rng, B, A, C, label, seed)
    t, a = torch.from_numpy(target), torch.from_numpy(anchors)
    enc = encode_target(t.double(), a.double(), XY_SCALE, WH_SCALE, EPS)[..., :4].float().numpy()
    noise = rng.standard_normal((B, A, 4), dtype=np.float32) * np.array([2.0, 2.0, 1.0, 1.0], np.float32)
    locs = np.where(pos[..., None], enc + noise, noise).astype(np.float32)
    assert np.isfinite(scores).all() and np.isfinite(locs).all() and np.isfinite(enc).all()
    return dict(B=B, A=A, C=C, regime=regime, seed=seed, anchors=a, target=t, scores=torch.from_numpy(scores.reshape(B, A * C).copy()),
                locs=torch.from_numpy(locs.reshape(B, A * 4).copy()))


def random_mask(case, seed=0):
    """bool [B, A], half of the rows: it samples some ignored rows and leaves some positives out.  Row [0, 0] -- a positive wherever the
    case has one -- is always sampled: without a sampled positive the reference's BinaryCrossEntropyWithSoftTargetsLoss is 0 / 0."""
    m = np.random.default_rng([77, seed, case['B'], case['A']]).random((case['B'], case['A'])) < 0.5
    m[0, 0] = True
    return torch.from_numpy(m)


# ---- every run of tests/test_loss_kernels_gpu.py ------------------------------------------------------------------------------------------
LDS_BYTES = 160 * 1024
C_MAX = (LDS_BYTES - 4096) // (64 * 4)                 # check_loss_common: 64 * C * 4 <= 160 KiB - 4096  (624)
SMALL = (2, 257, 21)                                   # a 64-row tile crosses the image boundary (257 = 4 * 64 + 1)
SWEEP_SHAPES = [(1, 1, 1), (2, 5, 1), (3, 21, 2), (2, 63, 3), (1, 64, 4), (1, 65, 5), (2, 70, 192), (2, 70, 193), (2, 70, C_MAX),
                (2, 262400, 2)]


def _sigmoid(cls):
    return cls['kind'] in ('sigmoid_focal', 'bce_soft')


def make_run(group, name, shape, cls, box, regime='normal', reduce_mean=1, mask='random', seed=0, no_positive=False, lse='both'):
    """One run of the GPU file.  mask: 'random' | 'ones' | 'zeros' | 'hnm' (mining at ratio 3, min 5).  lse: for the hard-label kinds, whether
    the run is made from a NaN workspace with lse_valid = 0 ('own'), after ssdk_hard_negative_mining with lse_valid = 1 ('sampler'), or both."""
    return dict(id=f'{group}-{name}', group=group, shape=tuple(shape), cls=cls, box=box, regime=regime, reduce_mean=reduce_mean, mask=mask,
                seed=seed, no_positive=no_positive, lse=lse)


def run_case(run):
    B, A, C = run['shape']
    return build(B, A, C, run['regime'], run['seed'], _sigmoid(run['cls']), run['no_positive'])


def run_mask(run, case):
    """The run's mask on the CPU ('hnm': the fp64 mining restatement's; the GPU file takes the kernel's own, which it also compares)."""
    B, A, C = run['shape']
    if run['mask'] == 'random':
        return random_mask(case, run['seed'])
    if run['mask'] == 'hnm':
        return torch.from_numpy(mining(case['scores'].view(B, A, C), case['target'][..., 4].numpy(), 3, 5))
    return torch.full((B, A), run['mask'] == 'ones', dtype=torch.bool)


def _runs():
    runs = []
    for cn, cls in CLS.items():                                                           # a. every kind, one small shape
        for bn, box in BOX.items():
            runs.append(make_run('a', f'{cn}-{bn}', SMALL, cls, box, seed=1))
    for shape in SWEEP_SHAPES:                                                            # b. the shape sweep
        combos = [(cn, 'smooth_l1') for cn in CLS] + [('ce', bn) for bn in BOX if bn != 'smooth_l1']
        for cn, bn in combos:
            if shape[2] == 1 and CLS[cn].get('epsilon'):
                continue                                                                   # losses.py:30 divides by C - 1
            runs.append(make_run('b', f'{shape[0]}x{shape[1]}x{shape[2]}-{cn}-{bn}', shape, CLS[cn], BOX[bn], seed=2))
    for cn in ('ce', 'ce_ls', 'ce_w', 'ce_ls_w', 'softmax_focal'):                        # d. lse_valid 1 against 0 on the mining mask
        runs.append(make_run('d', cn, SMALL, CLS[cn], BOX['smooth_l1'], mask='hnm', seed=3))
    for regime in ('wide', 'saturated'):                                                  # e. exponents and saturation
        for gamma in (0.0, 1.0, 2.0, 3.5):
            for alpha in (0.25, 0.5):
                runs.append(make_run('e', f'sigmoid_focal-g{gamma}-a{alpha}-{regime}', SMALL,
                                     dict(kind='sigmoid_focal', gamma=gamma, alpha=alpha), BOX['smooth_l1'], regime=regime, seed=4))
            for alpha in (0.25, 0.5, None):
                runs.append(make_run('e', f'softmax_focal-g{gamma}-a{alpha}-{regime}', SMALL,
                                     dict(kind='softmax_focal', gamma=gamma, alpha=alpha), BOX['smooth_l1'], regime=regime, seed=4))
        others = {'ce': CLS['ce'], 'ce_ls0.1': dict(kind='ce', label_smoothing=0.1), 'ce_ls1.0': dict(kind='ce', label_smoothing=1.0),
                  'ce_wz': dict(kind='ce', weight='zeros'), 'ce_ls0.1_wz': dict(kind='ce', label_smoothing=0.1, weight='zeros'),
                  'ce_soft': CLS['ce_soft'], 'ce_soft_eps': CLS['ce_soft_eps'], 'bce_soft': CLS['bce_soft'], 'bce_soft_eps': CLS['bce_soft_eps']}
        for cn, cls in others.items():
            runs.append(make_run('e', f'{cn}-{regime}', SMALL, cls, BOX['smooth_l1'], regime=regime, seed=4))
    for alpha in (0.25, 0.5):                                                             # gamma < 1: normal logits only
        runs.append(make_run('e', f'sigmoid_focal-g0.5-a{alpha}-normal', SMALL, dict(kind='sigmoid_focal', gamma=0.5, alpha=alpha),
                             BOX['smooth_l1'], seed=4))
    for alpha in (0.25, 0.5, None):
        runs.append(make_run('e', f'softmax_focal-g0.5-a{alpha}-normal', SMALL, dict(kind='softmax_focal', gamma=0.5, alpha=alpha),
                             BOX['smooth_l1'], seed=4))
    for cn in ('sigmoid_focal', 'softmax_focal', 'ce'):                                   # f. bookkeeping
        for rm in (0, 1, 2):
            runs.append(make_run('f', f'reduce_mean{rm}-{cn}', SMALL, CLS[cn], BOX['smooth_l1'], reduce_mean=rm, seed=5))
    for cn in ('ce', 'sigmoid_focal', 'ce_soft'):
        runs.append(make_run('f', f'ones-{cn}', SMALL, CLS[cn], BOX['smooth_l1'], mask='ones', seed=5))
    runs.append(make_run('f', 'zeros-ce', SMALL, CLS['ce'], BOX['smooth_l1'], mask='zeros', seed=5))
    for cn, bn in (('ce', 'smooth_l1'), ('sigmoid_focal', 'giou'), ('softmax_focal', 'smooth_l1')):
        runs.append(make_run('f', f'no_positive-{cn}-{bn}', SMALL, CLS[cn], BOX[bn], seed=5, no_positive=True))
    return runs


RUNS = _runs()
RUNS_BY_ID = {r['id']: r for r in RUNS}
assert len(RUNS_BY_ID) == len(RUNS)


def group(g):
    return [r['id'] for r in RUNS if r['group'] == g]


def reference_run(run, mask=None, dtype=torch.float64, encoded=None, case=None):
    """The restatement on a run (CLASS_W, LOC_W, GRAD_OUT) with the run's CPU mask unless one is given."""
    case = run_case(run) if case is None else case
    mask = run_mask(run, case) if mask is None else mask
    return restatement(case['target'], case['scores'], case['locs'], case['anchors'], mask, run['cls'], run['box'], CLASS_W, LOC_W,
                       run['reduce_mean'], dtype, GRAD_OUT, encoded)


# ---- box coder --------------------------------------------------------------------------------------------------------------------------
def encode_box(boxes, priors, inplace_semantics, dtype=torch.float64):
    """box_coder.py:22-30 (inplace: eps after the divide) / :32-34 (eps before it); boxes [B, A, 4] centroids, priors [A, 4]."""
    b, p = torch.as_tensor(boxes).to(dtype), torch.as_tensor(priors).to(dtype).unsqueeze(0)
    xy = (b[..., :2] - p[..., :2]) / p[..., 2:] * XY_SCALE
    wh = torch.log(b[..., 2:] / p[..., 2:] + EPS) if inplace_semantics else torch.log((b[..., 2:] + EPS) / p[..., 2:])
    return torch.cat([xy, wh * WH_SCALE], -1)


def decode_box(locs, priors, inplace_semantics, dtype=torch.float64):
    """box_coder.py:45-53 (inplace) / :55-57."""
    t, p = torch.as_tensor(locs).to(dtype), torch.as_tensor(priors).to(dtype).unsqueeze(0)
    if inplace_semantics:
        return torch.cat([t[..., :2] / XY_SCALE * p[..., 2:] + p[..., :2], torch.exp(t[..., 2:] / WH_SCALE) * p[..., 2:]], -1)
    return torch.cat([p[..., :2] + p[..., 2:] * t[..., :2] / XY_SCALE, p[..., 2:] * torch.exp(t[..., 2:] / WH_SCALE)], -1)


def coder_case(B, A, seed=0):
    """centroid boxes [B, A, 4] and priors [A, 4] of arbitrary (positive-size) magnitudes, locs [B, A, 4]."""
    rng = np.random.default_rng([seed, B, A])
    priors = np.concatenate([rng.uniform(0, 300, (A, 2)), rng.uniform(4, 200, (A, 2))], 1).astype(np.float32)
    boxes = np.concatenate([rng.uniform(0, 300, (B, A, 2)), rng.uniform(2, 250, (B, A, 2))], 2).astype(np.float32)
    locs = (rng.standard_normal((B, A, 4)) * np.array([3.0, 3.0, 2.0, 2.0])).astype(np.float32)
    return torch.from_numpy(boxes), torch.from_numpy(priors), torch.from_numpy(locs)


def coder_tolerance(ref64, torch32):
    """Per element: 4 x the case's largest fp32-torch error against fp64, at least 2 fp32 ulp of the reference value.  Returns (tolerance
    array, the measured maximum)."""
    ref = np.asarray(ref64, np.float64)
    measured = float(np.abs(np.asarray(torch32, np.float64) - ref).max())
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.maximum(4.0 * measured, 2.0 * ulp), measured
