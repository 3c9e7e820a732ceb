"""The IoU-based box terms (SSDK_LOC_IOU / _DIOU / _CIOU / _EIOU beside SSDK_LOC_GIOU; csrc/iou_loss.h): the definitions of
include/ssdk.h as executable torch -- any dtype, with autograd, so that torch.max / torch.min / clamp(min=0) supply the gradient rules (the
selected argument, half each at an exact tie, the clamp passes where its argument is >= 0) and ``alpha`` is taken under no_grad -- their
closed-form gradients away from a kink, the hand-built rows, the random row builder, and the references and run list that
tests/test_iou_loss.py (CPU, fp64 and fp32 torch) and tests/test_iou_loss_gpu.py (the kernels) share.  The reference has none of the four
losses, so there are no goldens: the yardstick is this restatement in fp64 on the CPU.

P is the predicted corner box and T the target corner box.  area, inter, uni and iou = inter / uni are quality_loss_cases.giou_loss's, no
epsilon; EPS = 1e-7 stands only where the new terms add a denominator:
    cw = max(P.x2, T.x2) - min(P.x1, T.x1), ch likewise, c2 = cw^2 + ch^2 + EPS
    rho2 = ((P.x1 + P.x2 - T.x1 - T.x2) / 2)^2 + ((P.y1 + P.y2 - T.y1 - T.y2) / 2)^2
    w, h of P and wg, hg of T: plain differences
    iou    1 - iou
    diou   1 - iou + rho2 / c2
    ciou   diou + alpha v,   v = 4 / pi^2 (atan(wg / hg) - atan(w / h))^2,   alpha = v / (1 - iou + v + EPS), a constant of the step
    eiou   diou + (w - wg)^2 / (cw^2 + EPS) + (h - hg)^2 / (ch^2 + EPS)"""
import functools
import math

import numpy as np
import torch

import loss_reference as lr
import quality_loss_cases as qc

EPS = 1e-7
KINDS = ('iou', 'giou', 'diou', 'ciou', 'eiou')
NEW_KINDS = ('iou', 'diou', 'ciou', 'eiou')
LOC_KIND = {'giou': 1, 'iou': 8, 'diou': 9, 'ciou': 10, 'eiou': 11}                       # include/ssdk.h
CLASS_NAME = {'giou': 'GeneralizedIoULoss', 'iou': 'IoULoss', 'diou': 'DistanceIoULoss', 'ciou': 'CompleteIoULoss', 'eiou': 'EfficientIoULoss'}
GRAD = dict(rtol=3e-4, atol=3e-7)                                                          # the project's GIoU figures (loss_reference.DLOCS['giou'])
KINK = lr.KINK


# ---- the definitions ---------------------------------------------------------------------------------------------------------------------
def _area(b):
    return (b[..., 2] - b[..., 0]).clamp(min=0) * (b[..., 3] - b[..., 1]).clamp(min=0)


def iou_loss(p, t, kind):
    """Per-box value [...] of corner boxes p against t [..., 4]; autograd towards p follows the rules above."""
    if kind == 'giou':
        return qc.giou_loss(p, t)
    inter = _area(torch.cat([torch.max(p[..., :2], t[..., :2]), torch.min(p[..., 2:], t[..., 2:])], -1))
    union = _area(p) + _area(t) - inter
    iou = inter / union
    if kind == 'iou':
        return 1.0 - iou
    cw = torch.max(p[..., 2], t[..., 2]) - torch.min(p[..., 0], t[..., 0])
    ch = torch.max(p[..., 3], t[..., 3]) - torch.min(p[..., 1], t[..., 1])
    c2 = cw * cw + ch * ch + EPS
    dx = (p[..., 0] + p[..., 2] - t[..., 0] - t[..., 2]) / 2
    dy = (p[..., 1] + p[..., 3] - t[..., 1] - t[..., 3]) / 2
    diou = 1.0 - iou + (dx * dx + dy * dy) / c2
    if kind == 'diou':
        return diou
    w, h = p[..., 2] - p[..., 0], p[..., 3] - p[..., 1]
    wg, hg = t[..., 2] - t[..., 0], t[..., 3] - t[..., 1]
    if kind == 'ciou':
        a = torch.atan(wg / hg) - torch.atan(w / h)
        v = (4.0 / math.pi ** 2) * (a * a)
        with torch.no_grad():
            alpha = v / (1.0 - iou + v + EPS)
        return diou + alpha * v
    assert kind == 'eiou', kind
    dw, dh = w - wg, h - hg
    return diou + dw * dw / (cw * cw + EPS) + dh * dh / (ch * ch + EPS)


def closed_form_grad(p, t, kind):
    """d iou_loss / dp [..., 4] written out (fp64), for rows AWAY from every kink: no tie, no clamp argument at 0.  1[.] are indicators."""
    p, t = p.double(), t.double()
    x1, y1, x2, y2 = p.unbind(-1)
    tx1, ty1, tx2, ty2 = t.unbind(-1)
    one = lambda c: c.double()                                                             # noqa: E731
    w, h, wg, hg = x2 - x1, y2 - y1, tx2 - tx1, ty2 - ty1
    iw = torch.min(x2, tx2) - torch.max(x1, tx1)
    ih = torch.min(y2, ty2) - torch.max(y1, ty1)
    ov = one((iw > 0) & (ih > 0))
    inter = iw.clamp(min=0) * ih.clamp(min=0)
    uni = w * h + wg * hg - inter
    # value = 1 - inter / uni (+ ...): coefficient of d area_p and of d inter
    c_area = inter / uni ** 2
    c_inter = -1.0 / uni - c_area
    g = torch.zeros_like(p)
    g[..., 0] = -c_area * h - c_inter * ih * ov * one(x1 > tx1)
    g[..., 2] = c_area * h + c_inter * ih * ov * one(x2 < tx2)
    g[..., 1] = -c_area * w - c_inter * iw * ov * one(y1 > ty1)
    g[..., 3] = c_area * w + c_inter * iw * ov * one(y2 < ty2)
    cw, ch = torch.max(x2, tx2) - torch.min(x1, tx1), torch.max(y2, ty2) - torch.min(y1, ty1)
    if kind == 'giou':                                                                     # ... - uni / enc
        enc = cw * ch
        d_uni, d_enc = -1.0 / enc, uni / enc ** 2
        for k, (side, sgn, coef) in enumerate(((one(x1 < tx1), -1, ch), (one(y1 < ty1), -1, cw), (one(x2 > tx2), 1, ch), (one(y2 > ty2), 1, cw))):
            g[..., k] += sgn * d_enc * coef * side
        # d uni = d area_p - d inter
        g[..., 0] += d_uni * (-h + ih * ov * one(x1 > tx1))
        g[..., 2] += d_uni * (h - ih * ov * one(x2 < tx2))
        g[..., 1] += d_uni * (-w + iw * ov * one(y1 > ty1))
        g[..., 3] += d_uni * (w - iw * ov * one(y2 < ty2))
        return g
    if kind == 'iou':
        return g
    c2 = cw * cw + ch * ch + EPS
    dx, dy = (x1 + x2 - tx1 - tx2) / 2, (y1 + y2 - ty1 - ty2) / 2
    rho2 = dx * dx + dy * dy
    kx, ky = -rho2 / c2 ** 2 * 2 * cw, -rho2 / c2 ** 2 * 2 * ch                            # coefficients of d cw, d ch
    gw = gh = torch.zeros_like(w)
    if kind == 'ciou':
        a = torch.atan(wg / hg) - torch.atan(w / h)
        v = (4.0 / math.pi ** 2) * a * a
        alpha = v / (1.0 - inter / uni + v + EPS)
        k = alpha * (8.0 / math.pi ** 2) * a / (w * w + h * h)
        gw, gh = -k * h, k * w
    elif kind == 'eiou':
        dw, dh = w - wg, h - hg
        cw2, ch2 = cw * cw + EPS, ch * ch + EPS
        gw, gh = 2 * dw / cw2, 2 * dh / ch2
        kx = kx - dw * dw / cw2 ** 2 * 2 * cw
        ky = ky - dh * dh / ch2 ** 2 * 2 * ch
    g[..., 0] += dx / c2 - gw - kx * one(x1 < tx1)
    g[..., 2] += dx / c2 + gw + kx * one(x2 > tx2)
    g[..., 1] += dy / c2 - gh - ky * one(y1 < ty1)
    g[..., 3] += dy / c2 + gh + ky * one(y2 > ty2)
    return g


def rows_reference(p, t, kind, grad_rows, dtype=torch.float64):
    """(values [n], dp [n, 4] = grad_rows[i] * d value_i / dp_i) of the restatement in ``dtype`` on the CPU, as numpy."""
    pp = torch.as_tensor(p).to(dtype).clone().requires_grad_(True)
    val = iou_loss(pp, torch.as_tensor(t).to(dtype), kind)
    (val * torch.as_tensor(grad_rows).to(dtype)).sum().backward()
    return val.detach().numpy(), pp.grad.numpy()


# ---- the hand-built rows: (P, T), every coordinate exactly representable in fp32 ----------------------------------------------------------
HAND_ROWS = [
    ('identical', (10, 20, 50, 80), (10, 20, 50, 80)),
    ('shared_left_edge', (10, 22, 40, 70), (10, 20, 50, 80)),
    ('touching', (10, 20, 30, 60), (30, 25, 60, 70)),                                      # ix2 - ix1 == 0
    ('disjoint', (0, 0, 16, 16), (32, 40, 64, 100)),
    ('p_inside_t', (20, 30, 40, 60), (10, 20, 50, 80)),
    ('t_inside_p', (10, 20, 50, 80), (20, 30, 40, 60)),
    ('same_aspect', (4, 8, 36, 72), (20, 40, 52, 104)),                                    # w / h == wg / hg == 0.5: v == 0
    ('same_centre', (10, 10, 50, 30), (20, 5, 40, 35)),                                    # rho2 == 0
    ('tiny_prediction', (16, 16, 16.125, 16.25), (15.875, 15.75, 16.5, 16.75)),            # 0.125 x 0.25
    ('wide_prediction', (-10000, 10, 10000, 50), (100, 0, 200, 80)),                       # 2e4 wide
]


def hand_rows():
    """(P [10, 4], T [10, 4]) fp32 tensors."""
    p = torch.tensor([r[1] for r in HAND_ROWS], dtype=torch.float32)
    t = torch.tensor([r[2] for r in HAND_ROWS], dtype=torch.float32)
    assert torch.equal(p.double().float(), p) and (p[:, 2:] > p[:, :2]).all() and (t[:, 2:] > t[:, :2]).all()
    return p, t


# ---- random rows ---------------------------------------------------------------------------------------------------------------------------
def at_kink(p, t, margin=KINK):
    """bool [n]: a predicted corner coordinate within ``margin`` of the target's same or opposite coordinate on its axis (where a max / min
    switches sides or a clamp argument crosses 0)."""
    p, t = torch.as_tensor(p).double(), torch.as_tensor(t).double()
    d = torch.cat([(p - t).abs(), (p[..., :2] - t[..., 2:]).abs(), (p[..., 2:] - t[..., :2]).abs()], -1)
    return d.min(-1).values < margin


@functools.lru_cache(maxsize=None)
def random_rows(n, seed=0):
    """(P [n, 4], T [n, 4], grad_rows [n]) fp32 on the CPU.  Targets as synthetic.make_ground_truth draws them for a 300-pixel image (sides
    of 8 % to 60 % of it, inside it); two rows in three are the target moved and resized by up to half its size (IoU spread over (0, 1)),
    the third is a box of the same law drawn on its own (mostly disjoint).  A row is redrawn while it sits at a kink; none does at the end."""
    rng = np.random.default_rng([4242, seed, n])
    size = 300.0

    def boxes(k):
        wh = rng.uniform(0.08 * size, 0.6 * size, (k, 2))
        xy = rng.uniform(0.0, 1.0, (k, 2)) * (size - wh)
        return np.concatenate([xy, xy + wh], 1)

    def predictions(t):
        k = len(t)
        wh = t[:, 2:] - t[:, :2]
        c = (t[:, :2] + t[:, 2:]) / 2 + rng.uniform(-0.5, 0.5, (k, 2)) * wh
        pwh = wh * np.exp(rng.uniform(-0.7, 0.7, (k, 2)))
        near = np.concatenate([c - pwh / 2, c + pwh / 2], 1)
        return np.where((rng.random(k) < 2.0 / 3.0)[:, None], near, boxes(k))

    t = boxes(n).astype(np.float32)
    p = predictions(t.astype(np.float64)).astype(np.float32)
    for _ in range(100):
        bad = at_kink(p, t).numpy() | ~(p[:, 2:] - p[:, :2] >= 1.0).all(1)
        if not bad.any():
            break
        p[bad] = predictions(t[bad].astype(np.float64)).astype(np.float32)
    p, t = torch.from_numpy(p), torch.from_numpy(t)
    assert not at_kink(p, t).any() and (p[:, 2:] - p[:, :2] >= 1.0).all()
    g = torch.from_numpy(rng.uniform(0.25, 2.0, n).astype(np.float32) * np.where(rng.random(n) < 0.3, -1.0, 1.0).astype(np.float32))
    return p, t, g


ROW_SIZES = (1, 255, 256, 257, 2048 * 256 + 1)         # one workgroup -+ 1; one row more than the grid's 2048 * 256 threads: the second round


def values_tolerance(ref64, torch32):
    """The box coder's rule (loss_reference.coder_tolerance): 4 x the largest fp32-torch error on the same rows, at least 2 fp32 ulp of the
    reference value.  Returns (tolerance array, the measured maximum)."""
    return lr.coder_tolerance(ref64, torch32)


# ---- the fused sampled kernels: run list and reference --------------------------------------------------------------------------------------
BOX = {k: dict(kind=k) for k in KINDS}
BIG = (2, 262400, 2)                                                                       # the forward's second grid-stride round


def _runs():
    runs = []
    for k in NEW_KINDS:                                                                    # a. every kind with three classification kernels
        for cn in ('ce', 'sigmoid_focal', 'ce_ls'):                                       # (ce_ls: the CEX instantiation)
            runs.append(lr.make_run('a', f'{k}-{cn}', lr.SMALL, lr.CLS[cn], BOX[k], seed=0))
    for shape in ((3, 21, 2), (2, 63, 3), (1, 64, 4), (1, 65, 5)):                        # b. tile edges
        for k in NEW_KINDS:
            runs.append(lr.make_run('b', f'{shape[0]}x{shape[1]}x{shape[2]}-{k}', shape, lr.CLS['ce'], BOX[k], seed=1))
    for shape in ((2, 5, 1), (1, 1, 1)):                                                   # c. no positive (C = 1: CrossEntropy has no positive class)
        for k in NEW_KINDS:
            runs.append(lr.make_run('c', f'{shape[0]}x{shape[1]}x{shape[2]}-{k}', shape, lr.CLS['ce'], BOX[k], seed=1))
    runs.append(lr.make_run('d', f'{BIG[0]}x{BIG[1]}x{BIG[2]}-iou', BIG, lr.CLS['ce'], BOX['iou'], seed=0))   # d. IoULoss only
    return runs


RUNS = _runs()
RUNS_BY_ID = {r['id']: r for r in RUNS}
assert len(RUNS_BY_ID) == len(RUNS)


def group(g):
    return [r['id'] for r in RUNS if r['group'] == g]


def box_term(case_locs, anchors, target, kind, dtype, weight, divider, grad):
    """The box term of MultiboxLoss for an IoU kind: decoded corners of every positive against its RAW target.  Returns (loc_loss,
    dlocs [B, A * 4] of grad * loc_loss, the sum of the absolute row contributions after the same scaling), as float / numpy."""
    B, A = target.shape[:2]
    target, anchors = target.detach().to(dtype), anchors.detach().to(dtype)
    cls = target[..., 4].long()
    positive = (cls != 0) & (cls != -1)
    l = case_locs.detach().to(dtype).clone().requires_grad_(True)
    rows = iou_loss(qc.decode_corners(l.view(B, A, 4), anchors)[positive], target[..., :4][positive], kind)
    loc_loss = rows.sum() * weight / divider
    (grad * loc_loss).backward()
    return float(loc_loss.detach()), l.grad.numpy(), float(rows.detach().abs().sum()) * abs(weight) / divider


def reference_run(run, mask=None, dtype=torch.float64, case=None):
    """loss_reference.reference_run's dict for a run of this list: the classification term is its own (with GIoU in the box slot, which
    leaves the target alone too), the box term is this module's."""
    case = lr.run_case(run) if case is None else case
    mask = lr.run_mask(run, case) if mask is None else mask
    ref = lr.reference_run(dict(run, box=lr.BOX['giou']), mask, dtype, case=case)
    cls = case['target'][..., 4].long()
    npos = int(((cls != 0) & (cls != -1)).sum())
    divider = 1.0 if run['reduce_mean'] == 2 else float(max(npos, 1))
    loc, dlocs, sabs = box_term(case['locs'], case['anchors'], case['target'], run['box']['kind'], dtype, lr.LOC_W, divider, lr.GRAD_OUT[1])
    values = np.array([ref['values'][1] + loc, ref['values'][1], loc])
    return dict(ref, values=values, dlocs=dlocs, sabs=np.array([ref['sabs'][1] + sabs, ref['sabs'][1], sabs]))


def compare(got, ref, kink, what=''):
    """loss_reference.compare with the GIoU family's dlocs tolerance (rtol 3e-4 / atol 3e-7; kink rows finite only)."""
    return lr.compare(got, ref, lr.BOX['giou'], kink, what)


# ---- the dense kernels: quality_loss_cases.restatement with the new box terms ----------------------------------------------------------------
def dense_reference(case, mask, kind, box, dtype=torch.float64, scores=None, locs=None, **kw):
    """quality_loss_cases.reference_run for an IoU box kind: (values [3], dscores, dlocs, q [B, A]) with the gradients of
    2 * class_loss + 0.5 * loc_loss.  The class term (and q, detached) is quality_loss_cases.restatement's."""
    s = (case['scores'] if scores is None else scores).to(dtype).clone().requires_grad_(True)
    l = (case['locs'] if locs is None else locs).to(dtype).clone().requires_grad_(True)
    loss, class_loss, loc_loss = dense_restatement(s, l, case['anchors'], case['target'], mask, kind, box, **kw)
    (2.0 * class_loss + 0.5 * loc_loss).backward()
    B, A = case['target'].shape[:2]
    q = qc.qualities(l.detach().view(B, A, 4), case['anchors'].to(dtype), case['target'].to(dtype))
    return np.array([float(v.detach()) for v in (loss, class_loss, loc_loss)]), s.grad.numpy(), l.grad.numpy(), q.numpy()


def dense_restatement(scores, locs, anchors, target, mask, kind, box, localization_weight=1.0, **kw):
    """(loss, class_loss, loc_loss) in the dtype of ``scores``, with autograd."""
    dt = scores.dtype
    B, A = target.shape[:2]
    _, class_loss, _ = qc.restatement(scores, locs, anchors, target, mask, kind, loc='giou', **kw)
    target, anchors = target.to(dt), anchors.to(dt)
    cls = target[..., 4].long()
    positive = (cls != 0) & (cls != -1)
    rows = iou_loss(qc.decode_corners(locs.view(B, A, 4), anchors)[positive], target[..., :4][positive], box)
    loc_loss = rows.sum() * localization_weight / positive.sum().clamp(min=1).to(dt)
    return class_loss + loc_loss, class_loss, loc_loss


DENSE_CASES = ('b3_c20', 'b2_c81_a257')
