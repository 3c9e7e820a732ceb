"""The integral box head and the Distribution Focal Loss (include/ssdk.h: ssdk_integral_fwd / ssdk_integral_bwd): the rule
as executable fp64 torch -- integral, DFL, their composition with the restatement of tests/quality_loss_cases.py for the class and box terms,
the closed-form gradients -- and the case builder that tests/test_dfl_gpu.py and tests/dfl_graph_worker.py share.  The reference has neither
the head nor the loss, so there are no goldens: the yardstick is this restatement on the CPU, with autograd."""
import functools

import numpy as np
import torch

import quality_loss_cases as qc

XY_LIMIT = WH_LIMIT = 8.0


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def grid(bins, xy_limit=XY_LIMIT, wh_limit=WH_LIMIT, dtype=torch.float64):
    """v [4, bins]: v_k[i] = -L_k + i * (2 L_k / reg_max), L = xy_limit for tx, ty and wh_limit for tw, th."""
    L = torch.tensor([xy_limit, xy_limit, wh_limit, wh_limit], dtype=dtype).view(4, 1)
    return -L + torch.arange(bins, dtype=dtype).view(1, bins) * (2.0 * L / (bins - 1))


def integral(z, xy_limit=XY_LIMIT, wh_limit=WH_LIMIT):
    """z [..., 4, bins] -> the expectation [..., 4] under softmax(z) (row maximum subtracted first: torch.softmax)."""
    return (torch.softmax(z, -1) * grid(z.shape[-1], xy_limit, wh_limit, z.dtype)).sum(-1)


def positions(encoded, bins, xy_limit=XY_LIMIT, wh_limit=WH_LIMIT):
    """y [..., 4] in bin units of encoded targets [..., 4]: clamp((t_k + L_k) / step_k, 0, reg_max)."""
    L = torch.tensor([xy_limit, xy_limit, wh_limit, wh_limit], dtype=encoded.dtype)
    return ((encoded + L) / (2.0 * L / (bins - 1))).clamp(0.0, float(bins - 1))


def brackets(y, bins):
    """(yl as long, weight of yl, weight of yr = yl + 1)."""
    yl = y.floor().clamp(max=bins - 2)
    return yl.long(), yl + 1.0 - y, y - yl


def dfl_terms(z, y):
    """The side terms [...]: lse(z) - ((yr - y) z[yl] + (y - yl) z[yr]); z [..., bins], y [...]."""
    yl, wl, wr = brackets(y, z.shape[-1])
    zl = z.gather(-1, yl.unsqueeze(-1)).squeeze(-1)
    zr = z.gather(-1, (yl + 1).unsqueeze(-1)).squeeze(-1)
    return torch.logsumexp(z, -1) - (wl * zl + wr * zr)


def closed_form_dz(z, y, v, g_side, dloc):
    """include/ssdk.h's gradient of one distribution: g_side * (p - wl [i == yl] - wr [i == yr]) + dloc * p * (v - loc); z [n, bins],
    y, g_side, dloc [n], v [bins] (g_side = g_dfl * distribution_weight / (4 max(1, #pos)))."""
    p = torch.softmax(z, -1)
    yl, wl, wr = brackets(y, z.shape[-1])
    hot = torch.zeros_like(z).scatter_(-1, yl.unsqueeze(-1), wl.unsqueeze(-1)).scatter_add_(-1, (yl + 1).unsqueeze(-1), wr.unsqueeze(-1))
    loc = (p * v).sum(-1, keepdim=True)
    return g_side.unsqueeze(-1) * (p - hot) + dloc.unsqueeze(-1) * p * (v - loc)


def target_positions(target, anchors, bins, xy_limit=XY_LIMIT, wh_limit=WH_LIMIT):
    """y [B, A, 4] of the RAW target rows (meaningful on the positives), through this suite's own encode."""
    return positions(qc.encode_target(target, anchors)[..., :4], bins, xy_limit, wh_limit)


def dfl_value(z, target, anchors, distribution_weight=0.25, xy_limit=XY_LIMIT, wh_limit=WH_LIMIT):
    """distribution_weight * sum over the positives of the mean of the four side terms / max(1, #positives); z [B, A, 4, bins]."""
    dt = z.dtype
    target, anchors = target.to(dt), anchors.to(dt)
    cls = target[..., 4].long()
    positive = (cls != 0) & (cls != -1)
    y = target_positions(target, anchors, z.shape[-1], xy_limit, wh_limit)
    terms = dfl_terms(z[positive], y[positive]).mean(-1)
    return distribution_weight * terms.sum() / positive.sum().clamp(min=1).to(dt)


def restatement(scores, logits, anchors, target, mask, kind, bins, loc='giou', distribution_weight=0.25, xy_limit=XY_LIMIT, wh_limit=WH_LIMIT,
                **kw):
    """(loss, class_loss, loc_loss, dfl, locs) of MultiboxLoss with an IntegralBoxCoder: the integral, then quality_loss_cases.restatement on
    the integrated locs, with the DFL value added to loc_loss and loss."""
    B, A = target.shape[:2]
    z = logits.view(B, A, 4, bins)
    locs = integral(z, xy_limit, wh_limit).view(B, A * 4)
    loss, class_loss, loc_loss = qc.restatement(scores, locs, anchors, target, mask, kind, loc=loc, **kw)
    dfl = dfl_value(z, target, anchors, distribution_weight, xy_limit, wh_limit) if distribution_weight else torch.zeros((), dtype=z.dtype)
    return loss + dfl, class_loss, loc_loss + dfl, dfl, locs


def reference_run(case, logits, mask, kind, bins, **kw):
    """The restatement with the gradients of 2 * class_loss + 0.5 * loc_loss (which holds the DFL value): values [4] (loss, class, loc,
    dfl), dscores, dlogits, locs as numpy."""
    s = case['scores'].double().requires_grad_(True)
    z = logits.double().requires_grad_(True)
    out = restatement(s, z, case['anchors'], case['target'], mask, kind, bins, **kw)
    (2.0 * out[1] + 0.5 * out[2]).backward()
    return np.array([float(v) for v in out[:4]]), s.grad.numpy(), z.grad.numpy(), out[4].detach().numpy()


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logits_for(name, bins, xy_limit=XY_LIMIT, wh_limit=WH_LIMIT, peak=4.0, seed=0):
    """Seeded noise around a one-hot at each row's target bin (the nearest node of its clamped y; rows that are not positive: a random bin):
    [B, A * 4 * bins] fp32 on the CPU for the case ``name`` of tests/quality_loss_cases.py."""
    c = qc.case(name)
    B, A = c['B'], c['A']
    rng = np.random.default_rng(7000 + 31 * bins + seed)
    y = target_positions(c['target'].double(), c['anchors'].double(), bins, xy_limit, wh_limit)
    node = torch.where(c['positive'].unsqueeze(-1), y.round().long(), torch.from_numpy(rng.integers(0, bins, (B, A, 4))))
    z = torch.from_numpy(rng.standard_normal((B, A, 4, bins)).astype(np.float32))
    z.scatter_add_(-1, node.unsqueeze(-1), torch.full((B, A, 4, 1), float(peak)))
    return z.reshape(B, A * 4 * bins).contiguous()
