"""GPU: the integral box head and the Distribution Focal Loss (csrc/integral.hip: ssdk_integral_fwd / ssdk_integral_bwd) against the fp64
torch-CPU restatement of tests/dfl_cases.py -- through the C ABI, through MultiboxLoss with an IntegralBoxCoder, through the loc heads built
with ``reg_max`` and through the Postprocessor.  Tolerances are the project's for this family (tests/test_quality_loss_gpu.py)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dfl_cases as dc
import quality_loss_cases as qc
from single_shot_detection_amd import _lib
from single_shot_detection_amd.detection import detector_builder, sampler
from single_shot_detection_amd.detection.box_coder import BoxCoder, IntegralBoxCoder
from single_shot_detection_amd.detection.losses.multibox_loss import MultiboxLoss
from single_shot_detection_amd.detection.modules.heads import multi_level_heads
from single_shot_detection_amd.detection.postprocessor import Postprocessor

pytestmark = pytest.mark.gpu

VALUES = dict(rtol=1e-5, atol=1e-4)
DLOGITS = dict(rtol=3e-4, atol=3e-7)
LOCS = dict(rtol=1e-5, atol=1e-5)
CLS = {'qfl': 'QualityFocalLoss', 'vfl': 'VarifocalLoss'}
LOC = {'giou': 'GeneralizedIoULoss', 'smooth_l1': 'SmoothL1Loss'}


def params(bins, weight=0.25, xy_limit=dc.XY_LIMIT, wh_limit=dc.WH_LIMIT, xy_scale=qc.XY_SCALE, wh_scale=qc.WH_SCALE, eps=qc.EPS):
    return _lib.IntegralParams(bins, xy_limit, wh_limit, xy_scale, wh_scale, eps, weight)


def abi_run(z, anchors, target, p, dlocs=None, g=None, with_target=True, backward=True):
    """ssdk_integral_fwd (+ _bwd) on CPU tensors z [B, A, 4, bins], anchors [A, 4], target [B, A, 6] (raw), dlocs [B, A, 4] or None, g: the
    upstream DFL gradient or None.  Outputs are pre-filled with 7 so that anything left unwritten shows."""
    lib = _lib.lib()
    dev = torch.device('cuda:0')
    B, A = z.shape[:2]
    zg, ag, tg = z.contiguous().cuda(), anchors.contiguous().cuda(), target.clone().cuda()
    locs = torch.full((B, A, 4), 7.0, device=dev)
    out2 = torch.full((2,), 7.0, device=dev)
    ws = torch.empty((lib.ssdk_integral_workspace_bytes(B, A),), dtype=torch.uint8, device=dev)
    stream = _lib.current_stream()
    rc = lib.ssdk_integral_fwd(ctypes.byref(p), _lib.ptr(zg), _lib.ptr(ag), _lib.ptr(tg) if with_target else None, B, A, _lib.ptr(locs),
                               _lib.ptr(out2), _lib.ptr(ws), ws.numel(), stream)
    assert rc == 0, rc
    res = dict(locs=locs, out2=out2)
    if backward:
        dz = torch.full_like(zg, 7.0)
        dl = None if dlocs is None else dlocs.contiguous().cuda()
        gg = None if g is None else torch.tensor([g], dtype=torch.float32, device=dev)
        # the multibox loss has run in between: the backward must not need the raw corners
        tg[..., :4] = float('nan')
        rc = lib.ssdk_integral_bwd(ctypes.byref(p), _lib.ptr(zg), _lib.ptr(dl), tg[..., 4].data_ptr() if with_target else None, 6, _lib.ptr(gg), B, A,
                                   _lib.ptr(dz), _lib.ptr(ws) if with_target else None, ws.numel() if with_target else 0, stream)
        assert rc == 0, rc
        res['dlogits'] = dz
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def abi_reference(z, anchors, target, p, dlocs=None, g=None):
    """fp64: locs, (value, #positives), dlogits of g * value + sum(dlocs * locs) with the rows that are not positive given no gradient."""
    zd = z.double().requires_grad_(True)
    locs = dc.integral(zd, p.xy_limit, p.wh_limit)
    cls = target[..., 4].long()
    positive = (cls != 0) & (cls != -1)
    w = p.distribution_weight
    value = dc.dfl_value(zd, target, anchors, w, p.xy_limit, p.wh_limit) if w else torch.zeros((), dtype=torch.float64)
    total = (g or 0.0) * value
    if dlocs is not None:
        total = total + (dlocs.double() * locs * positive.unsqueeze(-1)).sum()
    if total.requires_grad:
        total.backward()
    dz = zd.grad if zd.grad is not None else torch.zeros_like(zd)
    return locs.detach().numpy(), np.array([float(value.detach()), float(positive.sum())]), dz.numpy()


def case_inputs(name, bins, **limits):
    c = qc.case(name)
    B, A = c['B'], c['A']
    z = dc.logits_for(name, bins, **limits).view(B, A, 4, bins)
    dlocs = torch.from_numpy(np.random.default_rng(bins + A).standard_normal((B, A, 4)).astype(np.float32))
    return c, z, dlocs


def check_abi(name, bins, weight=0.25, **limits):
    c, z, dlocs = case_inputs(name, bins, **limits)
    p = params(bins, weight, **limits)
    got = abi_run(z, c['anchors'], c['target'], p, dlocs, 1.5)
    locs, out2, dz = abi_reference(z, c['anchors'], c['target'], p, dlocs, 1.5)
    print(name, bins, 'out', got['out2'].tolist(), out2.tolist(), 'max |dlocs|', np.abs(got['locs'].numpy() - locs).max(),
          'max |ddlogits|', np.abs(got['dlogits'].numpy() - dz).max())
    np.testing.assert_allclose(got['locs'].numpy(), locs, **LOCS)
    np.testing.assert_allclose(got['out2'].numpy(), out2, **VALUES)
    assert got['out2'][1].item() == out2[1]                      # the positive count is exact
    np.testing.assert_allclose(got['dlogits'].numpy(), dz, **DLOGITS)
    rows = ~c['positive']
    assert (got['dlogits'][rows] == 0).all()                     # rows that are not positive: exact zeros
    return got


@pytest.mark.parametrize('name', ['b1_c3_a5', 'b1_c81_a257', 'b2_c81_a257', 'b3_c20', 'no_positive'])
@pytest.mark.parametrize('bins', [17, 8, 2, 33, 64])
def test_abi_against_the_restatement(bins, name):
    """bins: 17 (odd: the LDS image is a straight copy), 8 and 2 (even: padded pitch; 2: a 16-byte vector covers two distributions), 33 (odd,
    32-row tiles), 64 (the limit).  Anchors: 5 (less than a tile), 257 (64-row tiles: four full ones and one of a single row; at B = 2 a
    tile crosses the image boundary), ssd_mb2_voc's 2 268 at B = 3 with an emptied image, and a batch without a positive."""
    got = check_abi(name, bins)
    c = qc.case(name)
    if name == 'no_positive':
        assert got['out2'].tolist() == [0.0, 0.0] and (got['dlogits'] == 0).all()     # value 0, divider 1, gradient all zeros
    if name == 'b3_c20':
        assert not c['positive'][1].any() and c['positive'][0].any()                    # the emptied image


@pytest.mark.parametrize('bins', [17, 8])
def test_targets_outside_the_grid_on_each_side(bins):
    """Limits of 1.0 / 0.5 put most encoded targets outside the grid, on both ends and for both kinds of side: y clamps to 0 and reg_max."""
    c = qc.case('b3_c20')
    y = dc.target_positions(c['target'].double(), c['anchors'].double(), bins, 1.0, 0.5)[c['positive']]
    for sides in (slice(0, 2), slice(2, 4)):
        assert (y[:, sides] == 0).any() and (y[:, sides] == bins - 1).any() and ((y[:, sides] > 0) & (y[:, sides] < bins - 1)).any()
    check_abi('b3_c20', bins, xy_limit=1.0, wh_limit=0.5)


def hand_rows():
    """B = 1, A = 5 on unit anchors at (0.5, 0.5), xy_scale = wh_scale = 1: row 0 a box of width and height 1 centred 3 right of and 3 above the
    anchor (tx = 3, ty = -3: y exactly on a node; tw = th = log(1) = 0); row 1 the same box 20 away (outside the grid on either end); row 2
    background; row 3 ignored; row 4 a positive whose logits are +-80."""
    anchors = torch.tensor([[0.5, 0.5, 1.0, 1.0]] * 5)
    target = torch.zeros((1, 5, 6))
    target[0, 0] = torch.tensor([3.0, -3.0, 4.0, -2.0, 2.0, 1.0])
    target[0, 1] = torch.tensor([20.0, -22.0, 21.0, -21.0, 1.0, 1.0])
    target[0, 2, 4], target[0, 3, 4] = 0.0, -1.0
    target[0, 4] = torch.tensor([0.75, 0.25, 1.5, 1.25, 3.0, 0.5])
    return anchors, target


@pytest.mark.parametrize('bins', [17, 8])
def test_a_target_exactly_on_a_node_and_logits_of_80(bins):
    anchors, target = hand_rows()
    rng = np.random.default_rng(5)
    z = torch.from_numpy(rng.standard_normal((1, 5, 4, bins)).astype(np.float32))
    z[0, 4] = torch.where(torch.from_numpy(rng.random((4, bins))) < 0.5, torch.tensor(80.0), torch.tensor(-80.0))
    z[0, 4, 0, 0], z[0, 4, 0, 1] = 80.0, -80.0
    p = params(bins, 0.25, xy_scale=1.0, wh_scale=1.0) if bins == 17 else params(bins, 0.25, 7.0, 7.0, 1.0, 1.0)   # (step 1 or 2: nodes stay exact)
    y = dc.positions(qc_encode(target, anchors, 1.0, 1.0), bins, p.xy_limit, p.wh_limit)
    assert (y[0, 0, :2] == y[0, 0, :2].round()).all() and y[0, 1, :2].tolist() == [float(bins - 1), 0.0]
    assert (y[0, :2, 2:] - (bins - 1) / 2).abs().max() < 1e-7          # (log(1 + eps): the middle of the grid, a node at 17 bins)
    dlocs = torch.from_numpy(rng.standard_normal((1, 5, 4)).astype(np.float32))
    got = abi_run(z, anchors, target, p, dlocs, 2.0)
    ref = hand_reference(z, anchors, target, p, dlocs, 2.0)
    assert torch.isfinite(got['locs']).all() and torch.isfinite(got['dlogits']).all() and torch.isfinite(got['out2']).all()
    np.testing.assert_allclose(got['locs'].numpy(), ref[0], **LOCS)
    np.testing.assert_allclose(got['out2'].numpy(), ref[1], **VALUES)
    np.testing.assert_allclose(got['dlogits'].numpy(), ref[2], **DLOGITS)
    assert (got['dlogits'][0, 2:4] == 0).all() and got['out2'][1].item() == 3.0


def qc_encode(target, anchors, xy_scale, wh_scale):
    """quality_loss_cases.encode_target with other scales (its own are module constants), fp64."""
    t = target.double().clone()
    b, pr = t[..., :4], anchors.double().unsqueeze(0)
    b[..., 2:] -= b[..., :2]
    b[..., :2] += b[..., 2:] / 2
    b[..., :2] -= pr[..., :2]
    b[..., :2] /= pr[..., 2:]
    b[..., :2] *= xy_scale
    b[..., 2:] /= pr[..., 2:]
    b[..., 2:] += qc.EPS
    b[..., 2:].log_()
    b[..., 2:] *= wh_scale
    return b


def hand_reference(z, anchors, target, p, dlocs, g):
    zd = z.double().requires_grad_(True)
    locs = dc.integral(zd, p.xy_limit, p.wh_limit)
    cls = target[..., 4].long()
    positive = (cls != 0) & (cls != -1)
    y = dc.positions(qc_encode(target, anchors, p.xy_scale, p.wh_scale), z.shape[-1], p.xy_limit, p.wh_limit)
    value = p.distribution_weight * dc.dfl_terms(zd[positive], y[positive]).mean(-1).sum() / positive.sum().clamp(min=1)
    (g * value + (dlocs.double() * locs * positive.unsqueeze(-1)).sum()).backward()
    return locs.detach().numpy(), np.array([float(value), float(positive.sum())]), zd.grad.numpy()


def test_without_a_target_it_is_the_integral_alone():
    """target = NULL (postprocess, evaluation): the same locs bit for bit, out and the workspace untouched; its backward (no class column)
    treats every row as live and has no DFL term."""
    c, z, dlocs = case_inputs('b2_c81_a257', 17)
    p = params(17)
    with_t = abi_run(z, c['anchors'], c['target'], p, backward=False)
    alone = abi_run(z, c['anchors'], c['target'], p, dlocs, None, with_target=False)
    assert torch.equal(with_t['locs'], alone['locs']) and alone['out2'].tolist() == [7.0, 7.0]
    zd = z.double().requires_grad_(True)
    (dlocs.double() * dc.integral(zd)).sum().backward()
    np.testing.assert_allclose(alone['dlogits'].numpy(), zd.grad.numpy(), **DLOGITS)


def test_dlocs_null_means_zeros():
    c, z, dlocs = case_inputs('b3_c20', 17)
    p = params(17)
    null = abi_run(z, c['anchors'], c['target'], p, None, 1.5)
    zeros = abi_run(z, c['anchors'], c['target'], p, torch.zeros_like(dlocs), 1.5)
    assert torch.equal(null['dlogits'], zeros['dlogits'])
    np.testing.assert_allclose(null['dlogits'].numpy(), abi_reference(z, c['anchors'], c['target'], p, None, 1.5)[2], **DLOGITS)
    none = abi_run(z, c['anchors'], c['target'], p, None, None)          # neither gradient: all zeros
    assert (none['dlogits'] == 0).all()


def test_weight_zero_skips_the_term_but_counts():
    c, z, dlocs = case_inputs('b3_c20', 17)
    got = abi_run(z, c['anchors'], c['target'], params(17, 0.0), dlocs, 1.5)
    assert got['out2'].tolist() == [0.0, float(c['positive'].sum())]
    np.testing.assert_allclose(got['dlogits'].numpy(), abi_reference(z, c['anchors'], c['target'], params(17, 0.0), dlocs, None)[2], **DLOGITS)


@pytest.mark.parametrize('bins', [17, 8])
def test_two_runs_give_identical_bits(bins):
    c, z, dlocs = case_inputs('b3_c20', bins)
    a, b = (abi_run(z, c['anchors'], c['target'], params(bins), dlocs, 1.5) for _ in range(2))
    for k in ('locs', 'out2', 'dlogits'):
        assert torch.equal(a[k], b[k]), k


def test_c_abi_refusals():
    """By return code, before any launch, with the outputs untouched."""
    lib = _lib.lib()
    dev = torch.device('cuda:0')
    B, A, bins = 1, 8, 17
    z = torch.zeros((B, A, 4, bins), device=dev)
    anchors = torch.ones((A, 4), device=dev)
    target = torch.zeros((B, A, 6), device=dev)
    locs, out2, dz = torch.full((B, A, 4), 7.0, device=dev), torch.full((2,), 7.0, device=dev), torch.full_like(z, 7.0)
    g = torch.ones((1,), device=dev)
    ws = torch.empty((lib.ssdk_integral_workspace_bytes(B, A),), dtype=torch.uint8, device=dev)
    s = _lib.current_stream()

    def fwd(p, z_=z, a_=anchors, t_=target, l_=locs, ws_=ws):
        return lib.ssdk_integral_fwd(ctypes.byref(p), _lib.ptr(z_), _lib.ptr(a_), _lib.ptr(t_), B, A, _lib.ptr(l_), _lib.ptr(out2), _lib.ptr(ws_),
                                     0 if ws_ is None else ws_.numel(), s)

    def bwd(p, z_=z, dz_=dz, cls=target, g_=g, ws_=ws):
        return lib.ssdk_integral_bwd(ctypes.byref(p), _lib.ptr(z_), None, None if cls is None else cls[..., 4].data_ptr(), 6, _lib.ptr(g_), B, A,
                                     _lib.ptr(dz_), _lib.ptr(ws_), 0 if ws_ is None else ws_.numel(), s)

    for bad in (params(1), params(65), params(0), params(17, xy_limit=0.0), params(17, wh_limit=-1.0), params(17, xy_scale=0.0),
                params(17, wh_scale=-5.0)):
        assert fwd(bad) == -1 and bwd(bad) == -1
    ok = params(17)
    assert fwd(ok, z_=None) == -1 and fwd(ok, l_=None) == -1 and fwd(ok, a_=None) == -1        # NULL logits / locs; a target without anchors
    assert bwd(ok, z_=None) == -1 and bwd(ok, dz_=None) == -1 and bwd(ok, cls=None) == -1      # ... a DFL gradient without the class column
    assert fwd(ok, ws_=None) == -2 and bwd(ok, ws_=None) == -2
    torch.cuda.synchronize()
    assert (locs == 7).all() and (out2 == 7).all() and (dz == 7).all()
    assert fwd(ok) == 0 and bwd(ok) == 0 and fwd(params(2)) == 0 and fwd(params(64), z_=torch.zeros((B, A, 4, 64), device=dev)) == 0
    assert fwd(ok, a_=None, t_=None, ws_=None) == 0 and bwd(ok, cls=None, g_=None, ws_=None) == 0   # the integral alone
    torch.cuda.synchronize()
    assert (locs == 0).all() and out2.tolist() == [0.0, 0.0]


# ---- through MultiboxLoss ----------------------------------------------------------------------------------------------------------------
def run_loss(case, logits, bins, kind, loc, dist=True, weight=0.25):
    coder = IntegralBoxCoder(qc.XY_SCALE, qc.WH_SCALE, reg_max=bins - 1)
    kw = {'distribution_loss': {'name': 'DistributionFocalLoss'}, 'distribution_weight': weight} if dist else {}
    crit = MultiboxLoss(sampler=sampler.valid_sampler, box_coder=coder, classification_loss={'name': CLS[kind]},
                        localization_loss={'name': LOC[loc]}, **kw)
    s, _, anchors, target = qc.fresh(case)
    z = logits.clone().cuda().requires_grad_(True)
    loss, class_loss, loc_loss = crit((s, z), anchors, target)
    (2.0 * class_loss + 0.5 * loc_loss).backward()
    locs = coder.integrate(z.detach(), case['A'])
    return dict(values=np.array([loss.item(), class_loss.item(), loc_loss.item(), crit.last_distribution_loss.item()]), dscores=s.grad.cpu().numpy(),
                dlogits=z.grad.cpu().numpy(), target=target.cpu(), locs=locs.cpu().numpy(),
                bits=[t.detach().cpu() for t in (loss, class_loss, loc_loss, s.grad, z.grad)])


def check_loss(name, bins, kind, loc, dist=True):
    case = qc.case(name)
    logits = dc.logits_for(name, bins, peak=6.0)
    got = run_loss(case, logits, bins, kind, loc, dist)
    encoded = got['target'] if loc == 'smooth_l1' else None
    vals, ds, dz, locs = dc.reference_run(case, logits, None, kind, bins, loc=loc, encoded=encoded, distribution_weight=0.25 if dist else 0.0)
    B, A = case['B'], case['A']
    if loc == 'giou':   # §22's kink rule, on the integrated locs: rows within 1e-3 pixel of a GIoU kink are only required to be finite
        P = qc.decode_corners(torch.from_numpy(locs).view(B, A, 4), case['anchors'].double())
        kink = ((P - case['target'].double()[..., :4]).abs().min(-1).values < 1e-3) & case['positive']
        k = kink.numpy().repeat(4 * bins, axis=1)
        assert np.isfinite(got['dlogits'][k]).all() and int(kink.sum()) <= 2
        got = dict(got, dlogits=np.where(k, 0.0, got['dlogits']))
        dz = np.where(k, 0.0, dz)
    print(name, bins, kind, loc, 'values', got['values'], vals, 'max |dlocs|', np.abs(got['locs'] - locs).max(),
          'max |ddscores|', np.abs(got['dscores'] - ds).max(), 'max |ddlogits|', np.abs(got['dlogits'] - dz).max())
    np.testing.assert_allclose(got['locs'], locs, **LOCS)
    np.testing.assert_allclose(got['values'], vals, **VALUES)
    np.testing.assert_allclose(got['dscores'], ds, rtol=3e-4, atol=3e-7)
    np.testing.assert_allclose(got['dlogits'], dz, **DLOGITS)
    return got, case


def test_qfl_giou_dfl_on_atss_targets():
    """The full GFL configuration on RetinaNet-500 geometry (47 961 anchors), B = 2, ATSS targets."""
    got, case = check_loss('retina_b2_c80_atss', 17, 'qfl', 'giou')
    assert got['values'][3] > 0 and torch.equal(got['target'], case['target'])


def test_varifocal_smooth_l1_dfl_sees_the_raw_target_first():
    """TargetAssigner(0.5, 0.4) targets; the SmoothL1 family encodes the target in place AFTER the integral node has read the raw corners:
    the target comes back encoded and the DFL value and gradient still match the restatement on the raw target."""
    got, case = check_loss('b3_c20', 17, 'vfl', 'smooth_l1')
    enc = qc.encode_target(case['target'].double(), case['anchors'].double())
    np.testing.assert_allclose(got['target'].numpy(), enc.numpy(), rtol=1e-6, atol=2e-5)
    assert not torch.equal(got['target'], case['target']) and got['values'][3] > 0
    again = run_loss(case, dc.logits_for('b3_c20', 17, peak=6.0), 17, 'vfl', 'smooth_l1')
    for a, b in zip(got['bits'], again['bits']):
        assert torch.equal(a, b)


@pytest.mark.parametrize('bins', [17, 8])
def test_integral_coder_without_a_distribution_loss(bins):
    got, _ = check_loss('b2_c81_a257', bins, 'qfl', 'giou', dist=False)
    assert got['values'][3] == 0.0


def test_wrong_logit_width_is_refused():
    case = qc.case('b1_c3_a5')
    crit = MultiboxLoss(sampler=sampler.valid_sampler, box_coder=IntegralBoxCoder(qc.XY_SCALE, qc.WH_SCALE), classification_loss={'name': 'QualityFocalLoss'},
                        localization_loss={'name': 'GeneralizedIoULoss'})
    s, l, anchors, target = qc.fresh(case)
    with pytest.raises(ValueError):
        crit((s, l), anchors, target)                              # four numbers per anchor


# ---- the loc heads of the reg_max route ---------------------------------------------------------------------------------------------------
def test_loc_heads_on_the_reg_max_route():
    """Two tiny levels (5 x 5 with one anchor type, 2 x 2 with two; Cin 16, 3 classes, bins 17): scores and logits, and the gradients of
    the maps and of every parameter, against torch.nn.functional.conv2d in fp64.  Tolerance: the GEMMs are exact fp32 with at most
    9 * 16 = 144 (forward), 50 (weights) and 9 * 142 (maps) products per sum, operands below ~4 and ~0.4: a worst case of ~1e-4 absolute."""
    F = torch.nn.functional
    torch.manual_seed(3)
    heads = detector_builder.get_heads([16, 16], [1, 2], 3, initializer={'name': 'normal_', 'args': {'mean': 0, 'std': 0.1}}, reg_max=16).cuda()
    for h in heads:
        torch.nn.init.normal_(h['loc'].bias, std=0.1)
    rng = np.random.default_rng(8)
    xs_np = [rng.standard_normal((2, 16, 5, 5)).astype(np.float32), rng.standard_normal((2, 16, 2, 2)).astype(np.float32)]
    xs = [torch.from_numpy(x).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for x in xs_np]
    scores, logits = multi_level_heads(xs, xs, heads)
    A = 25 + 8
    assert tuple(scores.shape) == (2, A * 3) and tuple(logits.shape) == (2, A * 4 * 17)
    ws_, wl_ = (torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)) for t in (scores, logits))
    ((scores * ws_.cuda()).sum() + (logits * wl_.cuda()).sum()).backward()

    xr = [torch.from_numpy(x).double().requires_grad_(True) for x in xs_np]
    pr = [{k: {n: getattr(h[k], n).detach().cpu().double().contiguous().requires_grad_(True) for n in ('weight', 'bias')} for k in ('score', 'loc')}
          for h in heads]
    flat = lambda k: torch.cat([F.conv2d(x, q[k]['weight'], q[k]['bias'], padding=1).permute(0, 2, 3, 1).reshape(2, -1) for x, q in zip(xr, pr)], 1)
    rs, rl = flat('score'), flat('loc')
    ((rs * ws_.double()).sum() + (rl * wl_.double()).sum()).backward()
    tol = dict(rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(scores.detach().cpu().numpy(), rs.detach().numpy(), **tol)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), rl.detach().numpy(), **tol)
    for x, r in zip(xs, xr):
        np.testing.assert_allclose(x.grad.cpu().numpy(), r.grad.numpy(), **tol)
    for h, q in zip(heads, pr):
        for k in ('score', 'loc'):
            for n in ('weight', 'bias'):
                np.testing.assert_allclose(getattr(h[k], n).grad.cpu().numpy(), q[k][n].grad.numpy(), **tol)


def test_postprocessor_integrates_first():
    """Postprocessor with the integral coder on the logits equals Postprocessor with a plain coder fed integrate(logits), bit for bit."""
    case = qc.case('b3_c20')
    logits = dc.logits_for('b3_c20', 17).cuda()
    scores, anchors = case['scores'].cuda(), case['anchors'].cuda()
    coder = IntegralBoxCoder(qc.XY_SCALE, qc.WH_SCALE)
    args = (0.3, {'max_per_class': 50, 'overlap_threshold': 0.45}, 'SIGMOID', 100)
    out_a, n_a = Postprocessor(coder, *args).postprocess_padded((scores, logits), anchors)
    locs = coder.integrate(logits, case['A'])
    assert tuple(locs.shape) == (case['B'], case['A'] * 4)
    out_b, n_b = Postprocessor(BoxCoder(qc.XY_SCALE, qc.WH_SCALE), *args).postprocess_padded((scores, locs), anchors)
    assert torch.equal(n_a, n_b) and int(n_a.sum()) > 0
    for i, n in enumerate(n_a.tolist()):
        assert torch.equal(out_a[i, :n], out_b[i, :n])


def test_integrate_has_autograd():
    coder = IntegralBoxCoder(qc.XY_SCALE, qc.WH_SCALE, reg_max=7)
    rng = np.random.default_rng(12)
    z_np = rng.standard_normal((2, 70 * 4 * 8)).astype(np.float32)
    w_np = rng.standard_normal((2, 70 * 4)).astype(np.float32)
    z = torch.from_numpy(z_np).cuda().requires_grad_(True)
    (coder.integrate(z, 70) * torch.from_numpy(w_np).cuda()).sum().backward()
    zd = torch.from_numpy(z_np).double().requires_grad_(True)
    (dc.integral(zd.view(2, 70, 4, 8)).view(2, -1) * torch.from_numpy(w_np).double()).sum().backward()
    np.testing.assert_allclose(z.grad.cpu().numpy(), zd.grad.numpy(), **DLOGITS)


def test_captured_graph_and_detection_init_in_a_child_process():
    """tests/dfl_graph_worker.py, in a process of its own (see there): ssdk_integral_fwd / _bwd captured in a HIP graph and replayed on two
    batches equal the eager results bit for bit; a training step through detection.init with the full GFL configuration, eager and with
    graph_hot_path=True, gives the same loss, which is the restatement's on the assigner's target."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, 'tests', 'dfl_graph_worker.py')], cwd=repo, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert res['timeouts'] == 0
    assert res['eager_loss'] == res['graphed_loss'] and np.isfinite(res['eager_loss']) and res['dfl'] > 0, res
