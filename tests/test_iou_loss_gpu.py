"""GPU: the IoU, DIoU, CIoU and EIoU box terms (csrc/iou_loss.h) against the fp64 restatement of tests/iou_loss_cases.py -- row by row through
ssdk_box_iou_loss_fwd / _bwd (csrc/boxes.hip; GIoU beside them), inside the fused sampled and dense loss kernels through the C ABI
(csrc/loss.hip), through MultiboxLoss (hard-negative mining, valid_sampler, the integral box head) and the standalone modules.

Every input of the C-ABI tests lies inside a larger allocation whose bytes are 0xFF (NaN) on both sides; every output lies between such
guards, which must keep their bits, and is itself 0xFF before the call, as is the workspace.  Tolerances: row values by the
box coder's rule (4 x the largest fp32-torch error on the same rows, at least 2 fp32 ulp of the reference); every gradient towards boxes or
locs rtol 3e-4 / atol 3e-7 (the project's GIoU figures); loss values 1e-5 of the term's fp64 sum of absolute row contributions; dscores rtol
3e-4 / atol 3e-7; the stored quality by the box coder's rule.  tests/test_iou_loss.py shows on the CPU that plain fp32 torch meets them."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dfl_cases as dc
import iou_loss_cases as ic
import loss_reference as lr
import quality_loss_cases as qc
from single_shot_detection_amd import _lib
from single_shot_detection_amd.bf.modules import losses
from single_shot_detection_amd.bf.utils import box_utils
from single_shot_detection_amd.detection import sampler
from single_shot_detection_amd.detection.box_coder import BoxCoder, IntegralBoxCoder
from single_shot_detection_amd.detection.losses.multibox_loss import MultiboxLoss

pytestmark = pytest.mark.gpu

PAD = 256                                             # guard bytes on either side (keeps the 16-byte alignment of the interior)
CLS_KIND = {'ce': 0, 'sigmoid_focal': 1, 'qfl': 5, 'vfl': 6}
SSDK_E_INVALID, SSDK_E_UNSUPPORTED = -1, -3
HNM = functools.partial(sampler.hard_negative_mining, negative_per_positive_ratio=3, min_negative_per_image=5)


class Buf:
    """``nbytes`` of device memory between two guards of PAD bytes, all 0xFF; ``data``: the interior's initial content."""

    def __init__(self, data=None, nbytes=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            nbytes = data.nbytes
        self.nbytes = nbytes
        self.t = torch.full((PAD + nbytes + PAD,), 0xFF, dtype=torch.uint8, device='cuda')
        assert self.t.data_ptr() % 256 == 0
        if data is not None and nbytes:
            self.t[PAD:PAD + nbytes] = torch.from_numpy(data.reshape(-1).view(np.uint8)).cuda()
        self.ptr = self.t.data_ptr() + PAD

    def get(self, dtype, shape=(-1,)):
        return self.t[PAD:PAD + self.nbytes].cpu().numpy().view(dtype).reshape(shape).copy()

    def intact(self):
        return bool((self.t[:PAD] == 0xFF).all()) and bool((self.t[PAD + self.nbytes:] == 0xFF).all())

    def untouched(self):
        return bool((self.t == 0xFF).all())


def stream():
    return _lib.current_stream()


# ---- 1. the row-wise kernels ----------------------------------------------------------------------------------------------------------------
def rows_run(kind, p, t, g):
    """ssdk_box_iou_loss_fwd + _bwd on guarded buffers: (values [n], dpred [n, 4])."""
    lib = _lib.lib()
    n = p.shape[0]
    inputs = dict(p=p.numpy(), t=t.numpy(), g=g.numpy())
    b = {k: Buf(v) for k, v in inputs.items()}
    b.update(out=Buf(nbytes=n * 4), dp=Buf(nbytes=n * 16))
    code = ic.LOC_KIND[kind]
    rc = lib.ssdk_box_iou_loss_fwd(code, b['p'].ptr, b['t'].ptr, n, b['out'].ptr, stream())
    assert rc == 0, (rc, lib.ssdk_last_error_string())
    rc = lib.ssdk_box_iou_loss_bwd(code, b['p'].ptr, b['t'].ptr, b['g'].ptr, n, b['dp'].ptr, stream())
    assert rc == 0, (rc, lib.ssdk_last_error_string())
    torch.cuda.synchronize()
    for k, v in b.items():
        assert v.intact(), ('guard of', k)
    for k, v in inputs.items():
        assert np.array_equal(b[k].get(np.uint8), np.ascontiguousarray(v).reshape(-1).view(np.uint8)), ('input', k)
    return b['out'].get(np.float32), b['dp'].get(np.float32, (n, 4))


def check_rows(kind, p, t, g, what):
    v64, g64 = ic.rows_reference(p, t, kind, g)
    v32, _ = ic.rows_reference(p, t, kind, g, torch.float32)
    got_v, got_g = rows_run(kind, p, t, g)
    tol, measured = ic.values_tolerance(v64, v32)
    err = np.abs(got_v.astype(np.float64) - v64)
    fv, fg = float((err / tol).max()), lr.excess(got_g, g64, **ic.GRAD)
    print('FRAC', what, f'values={fv:.3g} dpred={fg:.3g}', 'fp32 torch max', measured)
    assert np.isfinite(got_v).all() and (err <= tol).all(), (what, 'values', fv, measured)
    assert fg <= 1.0, (what, 'dpred', fg)
    return got_v, got_g


@pytest.mark.parametrize('kind', ic.KINDS)
def test_rows_hand_built(kind):
    """Identical boxes, a shared edge, touching, disjoint, nested either way, v == 0, rho2 == 0, a 0.125 x 0.25 and a 2e4-wide prediction:
    the rows where max / min / clamp tie."""
    p, t = ic.hand_rows()
    g = torch.linspace(0.5, 1.4, len(p))
    got_v, _ = check_rows(kind, p, t, g, f'rows-hand-{kind}')
    if kind != 'giou':
        assert got_v[0] == 0.0                                                             # identical boxes


@pytest.mark.parametrize('kind', ic.KINDS)
@pytest.mark.parametrize('n', ic.ROW_SIZES)
def test_rows_random(n, kind):
    """n = 1, one workgroup -+ 1 row, and one row more than the grid's 2048 * 256 threads (the grid-stride loop's second round)."""
    p, t, g = ic.random_rows(n)
    assert not (g == 1.0).all()
    a = check_rows(kind, p, t, g, f'rows-{n}-{kind}')
    if n == 257:
        b = rows_run(kind, p, t, g)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_rows_refusals():
    lib = _lib.lib()
    n = 64
    p, t, g = ic.random_rows(255)
    bp, bt, bg = Buf(p[:n + 1].numpy()), Buf(t[:n + 1].numpy()), Buf(g[:n].numpy())
    out, dp = Buf(nbytes=n * 4), Buf(nbytes=(n + 1) * 16)
    for kind in (0, 5, 12, 2, 7, -1):
        assert lib.ssdk_box_iou_loss_fwd(kind, bp.ptr, bt.ptr, n, out.ptr, stream()) == SSDK_E_INVALID
        assert lib.ssdk_box_iou_loss_bwd(kind, bp.ptr, bt.ptr, bg.ptr, n, dp.ptr, stream()) == SSDK_E_INVALID
    assert b'kind=' in lib.ssdk_last_error_string()
    for kind in (1, 8, 9, 10, 11):
        assert lib.ssdk_box_iou_loss_fwd(kind, bp.ptr + 4, bt.ptr, n, out.ptr, stream()) == SSDK_E_UNSUPPORTED
        assert lib.ssdk_box_iou_loss_fwd(kind, bp.ptr, bt.ptr + 8, n, out.ptr, stream()) == SSDK_E_UNSUPPORTED
        assert lib.ssdk_box_iou_loss_bwd(kind, bp.ptr + 4, bt.ptr, bg.ptr, n, dp.ptr, stream()) == SSDK_E_UNSUPPORTED
        assert lib.ssdk_box_iou_loss_bwd(kind, bp.ptr, bt.ptr, bg.ptr, n, dp.ptr + 4, stream()) == SSDK_E_UNSUPPORTED
        assert lib.ssdk_box_iou_loss_fwd(kind, None, bt.ptr, n, out.ptr, stream()) == SSDK_E_INVALID
        assert lib.ssdk_box_iou_loss_bwd(kind, bp.ptr, bt.ptr, None, n, dp.ptr, stream()) == SSDK_E_INVALID
        assert lib.ssdk_box_iou_loss_fwd(kind, bp.ptr, bt.ptr, -1, out.ptr, stream()) == SSDK_E_INVALID
        assert lib.ssdk_box_iou_loss_fwd(kind, None, None, 0, None, stream()) == 0        # no rows: nothing to do
    torch.cuda.synchronize()
    assert out.untouched() and dp.untouched()


# ---- 2. the fused sampled kernels through the C ABI -----------------------------------------------------------------------------------------
def loss_params(cls_kind, box, gamma=2.0, alpha=0.25, reduce_mean=1, ls=0.0, quality=0, class_w=lr.CLASS_W, loc_w=lr.LOC_W):
    return _lib.LossParams(cls_kind, ic.LOC_KIND[box], float(gamma), float(alpha), reduce_mean, 0.0, class_w, loc_w, lr.XY_SCALE, lr.WH_SCALE, lr.EPS,
                           1.0, float(ls), None, quality)


def abi_run(case, p, mask, grad_out, lse_valid=0, ws=None, what=''):
    """ssdk_multibox_loss_fwd + ssdk_multibox_loss_bwd_ex on guarded buffers from a workspace of NaN bytes (or the one a sampler call
    filled): a dict of numpy outputs.  mask None: sampled = NULL (the dense kernels)."""
    lib = _lib.lib()
    B, A, C = case['B'], case['A'], case['C']
    inputs = dict(scores=case['scores'].numpy(), locs=case['locs'].numpy(), anchors=case['anchors'].numpy(), grad=np.asarray(grad_out, np.float32))
    if mask is not None:
        inputs['mask'] = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
    b = {k: Buf(v) for k, v in inputs.items()}
    b.update(target=Buf(case['target'].numpy()), out3=Buf(nbytes=12), dscores=Buf(nbytes=B * A * C * 4), dlocs=Buf(nbytes=B * A * 16),
             row_mask=Buf(nbytes=B * A))
    b['ws'] = Buf(nbytes=lib.ssdk_multibox_loss_workspace_bytes(B, A, C)) if ws is None else ws
    mptr = b['mask'].ptr if mask is not None else None
    rc = lib.ssdk_multibox_loss_fwd(ctypes.byref(p), b['scores'].ptr, b['locs'].ptr, b['anchors'].ptr, b['target'].ptr, mptr, B, A, C, lse_valid,
                                    b['out3'].ptr, b['ws'].ptr, b['ws'].nbytes, stream())
    assert rc == 0, (what, 'fwd', rc, lib.ssdk_last_error_string())
    rc = lib.ssdk_multibox_loss_bwd_ex(ctypes.byref(p), b['scores'].ptr, b['locs'].ptr, b['anchors'].ptr, b['target'].ptr, mptr, b['grad'].ptr, 0,
                                       B, A, C, b['dscores'].ptr, b['dlocs'].ptr, b['row_mask'].ptr, b['ws'].ptr, b['ws'].nbytes, stream())
    assert rc == 0, (what, 'bwd', rc, lib.ssdk_last_error_string())
    torch.cuda.synchronize()
    for k, v in b.items():
        assert v.intact(), (what, 'guard of', k)
    for k, v in inputs.items():                                                            # inputs keep their bits
        assert np.array_equal(b[k].get(np.uint8), np.ascontiguousarray(v).reshape(-1).view(np.uint8)), (what, 'input', k)
    # the target is left alone: bit-identical after the call
    assert np.array_equal(b['target'].get(np.uint32), case['target'].numpy().reshape(-1).view(np.uint32)), (what, 'target')
    return dict(values=b['out3'].get(np.float32).astype(np.float64), dscores=b['dscores'].get(np.float32, (B, A * C)),
                dlocs=b['dlocs'].get(np.float32, (B, A * 4)), row_mask=b['row_mask'].get(np.uint8, (B, A)),
                quality=b['ws'].get(np.uint8)[:B * A * 4].view(np.float32).reshape(B, A))   # (the workspace's first array: lse / the dense kernels' q)


def check_row_mask(case, want, got, what):
    """row_mask == want | positive; rows outside it are +0 bits in both gradients; rows that are not wanted have no classification gradient."""
    B, A, C = case['B'], case['A'], case['C']
    c = case['target'].numpy()[..., 4].astype(np.int64)
    positive = (c != 0) & (c != -1)
    assert np.array_equal(got['row_mask'], (want | positive).astype(np.uint8)), (what, 'row_mask')
    off = got['row_mask'] == 0
    assert not got['dscores'].reshape(B, A, C).view(np.uint32)[off].any(), (what, 'dscores rows outside row_mask')
    assert not got['dlocs'].reshape(B, A, 4).view(np.uint32)[off].any(), (what, 'dlocs rows outside row_mask')
    assert not got['dscores'].reshape(B, A, C).view(np.uint32)[~want].any(), (what, 'dscores rows that are not sampled')
    assert not got['dlocs'].reshape(B, A, 4).view(np.uint32)[~positive].any(), (what, 'dlocs rows that are not positive')


def mine(case):
    """ssdk_hard_negative_mining on a case (class_stride 6 into its target): (mask uint8 [B, A], the workspace it filled)."""
    B, A, C = case['B'], case['A'], case['C']
    scores, target, out = Buf(case['scores'].numpy()), Buf(case['target'].numpy()), Buf(nbytes=B * A)
    ws = Buf(nbytes=_lib.lib().ssdk_multibox_loss_workspace_bytes(B, A, C))
    rc = _lib.lib().ssdk_hard_negative_mining(scores.ptr, target.ptr + 16, 6, B, A, C, 3.0, 5, out.ptr, ws.ptr, ws.nbytes, stream())
    assert rc == 0, (rc, _lib.lib().ssdk_last_error_string())
    torch.cuda.synchronize()
    assert scores.intact() and target.intact() and out.intact() and ws.intact()
    return out.get(np.uint8, (B, A)), ws


def check_fused(run, mask=None, lse_valid=0, ws=None):
    case = lr.run_case(run)
    mask = lr.run_mask(run, case).numpy() if mask is None else mask
    what = f"{run['id']} lse_valid={lse_valid}"
    cls = run['cls']
    p = loss_params(CLS_KIND[cls['kind']], run['box']['kind'], cls.get('gamma', 2.0), cls.get('alpha', 0.25), run['reduce_mean'],
                    cls.get('label_smoothing', 0.0))
    got = abi_run(case, p, mask, lr.GRAD_OUT, lse_valid, ws, what)
    m = np.asarray(mask).astype(bool)
    c = case['target'].numpy()[..., 4]
    check_row_mask(case, (m & (c != -1)) if lr.hard_label(cls) else m, got, what)
    ref = ic.reference_run(run, torch.from_numpy(m), case=case)
    ic.compare(got, ref, lr.giou_kink(case).numpy(), what)
    return got


@pytest.mark.parametrize('rid', ic.group('a'))
def test_fused_every_kind_with_three_classification_kernels(rid):
    """(2, 257, 21): a 64-row tile crosses the image boundary.  ce and sigmoid_focal: the plain instantiation; ce_ls: CEX.  The hard-label
    runs are made twice: from a NaN workspace and after ssdk_hard_negative_mining left every row's log-sum-exp (lse_valid = 1)."""
    run = ic.RUNS_BY_ID[rid]
    check_fused(run)
    if lr.hard_label(run['cls']):
        _, ws = mine(lr.run_case(run))
        check_fused(run, lse_valid=1, ws=ws)


@pytest.mark.parametrize('rid', ic.group('b'))
def test_fused_tile_edges(rid):
    check_fused(ic.RUNS_BY_ID[rid])


@pytest.mark.parametrize('rid', ic.group('c'))
def test_fused_without_a_positive(rid):
    got = check_fused(ic.RUNS_BY_ID[rid])
    assert got['values'][2] == 0.0 and not got['dlocs'].view(np.uint32).any()


@pytest.mark.parametrize('rid', ic.group('d'))
def test_fused_second_grid_stride_round(rid):
    """(2, 262 400, 2): 524 800 rows against the forward's 2048 * 256 threads, so its grid-stride loop makes a second round.  IoULoss only:
    the loop is the one every kind shares.  The few of its ~40 000 positives that sit at a kink are left out of the dlocs
    comparison, finite, as DESIGN.md §22 does."""
    check_fused(ic.RUNS_BY_ID[rid])


@pytest.mark.parametrize('box', ic.NEW_KINDS)
def test_fused_two_runs_give_identical_bits(box):
    run = lr.make_run('a', f'twice-{box}', lr.SMALL, lr.CLS['ce_ls'], ic.BOX[box], seed=3)
    case = lr.run_case(run)
    mask = lr.run_mask(run, case).numpy()
    p = loss_params(0, box, ls=0.1)
    a, b = (abi_run(case, p, mask, lr.GRAD_OUT) for _ in range(2))
    for k in ('values', 'dscores', 'dlocs', 'row_mask'):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert np.abs(a['dlocs']).max() > 0


def test_loc_kinds_5_6_7_and_12_stay_refused():
    lib = _lib.lib()
    run = ic.RUNS_BY_ID[ic.group('b')[0]]
    case = lr.run_case(run)
    B, A, C = case['B'], case['A'], case['C']
    bufs = [Buf(case[k].numpy()) for k in ('scores', 'locs', 'anchors', 'target')]
    mask, grad = Buf(np.ones((B, A), np.uint8)), Buf(np.ones(2, np.float32))
    outs = [Buf(nbytes=12), Buf(nbytes=B * A * C * 4), Buf(nbytes=B * A * 16), Buf(nbytes=lib.ssdk_multibox_loss_workspace_bytes(B, A, C))]
    for kind in (5, 6, 7, 12, -1):
        p = _lib.LossParams(0, kind, 2.0, 0.25, 0, 0.0, 1.0, 1.0, lr.XY_SCALE, lr.WH_SCALE, lr.EPS, 1.0, 0.0, None, 0)
        assert lib.ssdk_multibox_loss_fwd(ctypes.byref(p), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, mask.ptr, B, A, C, 0, outs[0].ptr,
                                          outs[3].ptr, outs[3].nbytes, stream()) == SSDK_E_INVALID
        assert lib.ssdk_multibox_loss_bwd(ctypes.byref(p), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, mask.ptr, grad.ptr, B, A, C,
                                          outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[3].nbytes, stream()) == SSDK_E_INVALID
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# ---- 3. the dense kernels -------------------------------------------------------------------------------------------------------------------
def check_dense(name, kind, box, use_iou):
    case = qc.case(name)
    what = f"dense-{name}-{kind}-{box}-use_iou{int(use_iou)}"
    kink = lr.giou_kink(case)
    # the one positive the builder places exactly on its box: left out of the dlocs comparison, finite.  At least 10 positives are compared
    # (b2_c81_a257, a slice of 257 anchors, has 4 positives in all: there every one but that row)
    npos = int(case['positive'].sum())
    assert int(kink.sum()) <= 1 and int((case['positive'] & ~kink).sum()) >= min(10, npos - 1) >= 3, (what, int(kink.sum()), npos)
    alpha = 0.75 if kind == 'vfl' else 0.25
    p = loss_params(CLS_KIND[kind], box, 2.0, alpha, 0, quality=int(use_iou), class_w=1.0, loc_w=1.0)
    got = abi_run(case, p, None, (2.0, 0.5), what=what)
    c = case['target'].numpy()[..., 4]
    check_row_mask(case, c != -1, got, what)
    vals, ds, dl, q = ic.dense_reference(case, None, kind, box, use_iou=use_iou)
    v32, _, _, q32 = ic.dense_reference(case, None, kind, box, torch.float32, use_iou=use_iou)
    frac = {}
    fv = []
    for k in range(3):   # every row contribution of these terms is >= 0: the sum of their absolute values is the term itself
        err, tol = abs(got['values'][k] - vals[k]), lr.VALUES_RTOL * abs(vals[k])
        fv.append(0.0 if err == 0.0 else (np.inf if tol == 0.0 else err / tol))
    frac['values'] = max(fv)
    frac['dscores'] = lr.excess(got['dscores'], ds, **lr.DSCORES)
    k = kink.numpy().reshape(-1)
    gd, rd = got['dlocs'].reshape(-1, 4), dl.reshape(-1, 4)
    assert np.isfinite(gd[k]).all()
    frac['dlocs'] = lr.excess(gd[~k], rd[~k], **ic.GRAD)
    pos = case['positive'].numpy()
    if use_iou:
        tol, measured = ic.values_tolerance(q[pos], q32[pos])
        frac['q'] = float((np.abs(got['quality'][pos].astype(np.float64) - q[pos]) / tol).max())
    else:
        assert (got['quality'] == 1.0).all()
    print('FRAC', what, ' '.join(f'{a}={b:.3g}' for a, b in frac.items()), 'values', got['values'], vals)
    assert max(frac.values()) <= 1.0, (what, frac)
    return got


@pytest.mark.parametrize('use_iou', [True, False])
@pytest.mark.parametrize('box', ic.NEW_KINDS)
@pytest.mark.parametrize('kind', ['qfl', 'vfl'])
@pytest.mark.parametrize('name', ic.DENSE_CASES)
def test_dense(name, kind, box, use_iou):
    """Quality Focal / Varifocal with sampled = NULL: the row phase decodes P once for the box term and for q."""
    check_dense(name, kind, box, use_iou)


def test_dense_retina_500_atss():
    """RetinaNet-500 geometry (47 961 anchors, 80 classes), B = 2, ATSS targets: the tiles stride."""
    assert qc.case('retina_b2_c80_atss')['A'] == 47961
    check_dense('retina_b2_c80_atss', 'qfl', 'ciou', True)


def test_dense_two_runs_give_identical_bits():
    case = qc.case('b3_c20')
    p = loss_params(5, 'ciou', 2.0, 0.25, 0, quality=1)
    a, b = (abi_run(case, p, None, (2.0, 0.5)) for _ in range(2))
    for k in ('values', 'dscores', 'dlocs', 'row_mask', 'quality'):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ---- 4. the modules -------------------------------------------------------------------------------------------------------------------------
def module_run(case, scores, smp, cl, box, coder=None, logits=None, **kw):
    crit = MultiboxLoss(sampler=smp, box_coder=coder or BoxCoder(qc.XY_SCALE, qc.WH_SCALE), classification_loss=cl,
                        localization_loss={'name': ic.CLASS_NAME[box]}, **kw)
    assert crit.loc_kind == ic.LOC_KIND[box]
    s = scores.clone().cuda().requires_grad_(True)
    l = (case['locs'] if logits is None else logits).clone().cuda().requires_grad_(True)
    target = case['target'].clone().cuda()
    loss, class_loss, loc_loss = crit((s, l), case['anchors'].cuda(), target)
    (2.0 * class_loss + 0.5 * loc_loss).backward()
    assert torch.equal(target.cpu(), case['target'])                                       # left alone
    return dict(values=np.array([loss.item(), class_loss.item(), loc_loss.item()], np.float64), dscores=s.grad.cpu().numpy(),
                dlocs=l.grad.cpu().numpy(), mask=crit.last_sampled_mask.cpu().bool(), crit=crit)


@pytest.mark.parametrize('box', ic.NEW_KINDS)
def test_multibox_loss_hard_negative_mining_cross_entropy(box):
    case = qc.case('b3_c20')
    B, A, C = case['B'], case['A'], 21
    scores = torch.from_numpy(np.random.default_rng(3).standard_normal((B, A * C), dtype=np.float32))
    got = module_run(case, scores, HNM, {'name': 'CrossEntropyLoss'}, box)
    ref = lr.restatement(case['target'], scores, case['locs'], case['anchors'], got['mask'], lr.CLS['ce'], lr.BOX['giou'], grad_out=(2.0, 0.5))
    npos = float(max(int(case['positive'].sum()), 1))
    loc, dlocs, sabs = ic.box_term(case['locs'], case['anchors'], case['target'], box, torch.float64, 1.0, npos, 0.5)
    ref = dict(ref, values=np.array([ref['values'][1] + loc, ref['values'][1], loc]), dlocs=dlocs,
               sabs=np.array([ref['sabs'][1] + sabs, ref['sabs'][1], sabs]))
    ic.compare(got, ref, lr.giou_kink(case).numpy(), f'module-hnm-ce-{box}')


@pytest.mark.parametrize('box', ic.NEW_KINDS)
def test_multibox_loss_valid_sampler_quality_focal(box):
    case = qc.case('b3_c20')
    got = module_run(case, case['scores'], sampler.valid_sampler, {'name': 'QualityFocalLoss'}, box)
    assert torch.equal(got['mask'], case['target'][..., 4] != -1)
    vals, ds, dl, _ = ic.dense_reference(case, None, 'qfl', box)
    ref = dict(values=vals, dscores=ds, dlocs=dl, sabs=np.abs(vals))
    ic.compare(got, ref, lr.giou_kink(case).numpy(), f'module-valid-qfl-{box}')


def test_multibox_loss_integral_head_dfl_and_ciou():
    """IntegralBoxCoder(reg_max=16) + DistributionFocalLoss + CompleteIoULoss: the loss and the gradient on the distribution logits against
    the restatement chained through tests/dfl_cases.py's integral (integrate, ordinary locs, dlocs back through ssdk_integral_bwd)."""
    bins = 17
    case = qc.case('b3_c20')
    B, A = case['B'], case['A']
    logits = dc.logits_for('b3_c20', bins, peak=6.0)
    got = module_run(case, case['scores'], sampler.valid_sampler, {'name': 'QualityFocalLoss'}, 'ciou',
                     coder=IntegralBoxCoder(qc.XY_SCALE, qc.WH_SCALE, reg_max=bins - 1), logits=logits,
                     distribution_loss={'name': 'DistributionFocalLoss'}, distribution_weight=0.25)
    dfl_got = got['crit'].last_distribution_loss.item()
    s = case['scores'].double().requires_grad_(True)
    z = logits.double().requires_grad_(True)
    locs = dc.integral(z.view(B, A, 4, bins)).view(B, A * 4)
    loss, class_loss, loc_loss = ic.dense_restatement(s, locs, case['anchors'], case['target'], None, 'qfl', 'ciou')
    dfl = dc.dfl_value(z.view(B, A, 4, bins), case['target'], case['anchors'], 0.25)
    (2.0 * class_loss + 0.5 * (loc_loss + dfl)).backward()
    vals = np.array([float(loss + dfl), float(class_loss), float(loc_loss + dfl)])
    # §22's kink rule on the integrated locs
    P = qc.decode_corners(locs.detach().view(B, A, 4), case['anchors'].double())
    kink = ic.at_kink(P, case['target'].double()[..., :4]) & case['positive']
    k = kink.numpy().repeat(4 * bins, axis=1)
    assert np.isfinite(got['dlocs'][k]).all() and int(kink.sum()) <= 2
    fz = lr.excess(np.where(k, 0.0, got['dlocs']), np.where(k, 0.0, z.grad.numpy()), **ic.GRAD)
    fs = lr.excess(got['dscores'], s.grad.numpy(), **lr.DSCORES)
    fv = float(np.max(np.abs(got['values'] - vals) / (lr.VALUES_RTOL * np.abs(vals))))
    print('FRAC module-integral-dfl-ciou', f'values={fv:.3g} dscores={fs:.3g} dlogits={fz:.3g}', got['values'], vals, dfl_got, float(dfl))
    assert fv <= 1.0 and fs <= 1.0 and fz <= 1.0 and abs(dfl_got - float(dfl)) <= lr.VALUES_RTOL * float(dfl) and float(dfl) > 0


@pytest.mark.parametrize('reduction', ['none', 'mean', 'sum'])
@pytest.mark.parametrize('n', [1000, 7])
@pytest.mark.parametrize('kind', ic.NEW_KINDS)
def test_standalone_modules(kind, n, reduction):
    p, t, _ = ic.random_rows(n, seed=1)
    module = getattr(losses, ic.CLASS_NAME[kind])(reduction=reduction)
    x = p.clone().cuda().requires_grad_(True)
    out = module(x, t.cuda())
    up = torch.linspace(0.5, 2.0, n) if reduction == 'none' else torch.tensor(3.0)
    (out * up.cuda()).sum().backward()
    scale = 1.0 / n if reduction == 'mean' else 1.0
    g = (up.expand(n) if reduction != 'none' else up) * scale
    v64, g64 = ic.rows_reference(p, t, kind, g)
    v32, _ = ic.rows_reference(p, t, kind, g, torch.float32)
    if reduction == 'none':
        tol, _ = ic.values_tolerance(v64, v32)
        assert out.shape == (n,) and (np.abs(out.detach().cpu().numpy().astype(np.float64) - v64) <= tol).all()
    else:
        assert out.dim() == 0 and abs(out.item() - v64.sum() * scale) <= lr.VALUES_RTOL * np.abs(v64).sum() * scale
    assert lr.excess(x.grad.cpu().numpy(), g64, **ic.GRAD) <= 1.0


def test_box_utils_iou_loss_giou_is_one_minus_generalized_iou():
    p, t, _ = ic.random_rows(257)
    a = box_utils.iou_loss(p.cuda(), t.cuda(), 'giou')
    b = 1.0 - box_utils.generalized_iou(p.cuda(), t.cuda(), cartesian=False)
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=2.4e-7)       # (1 - (a - b) against 1 - giou: 2 ulp of 1)
    with pytest.raises(ValueError):
        box_utils.iou_loss(p.cuda(), t[:5].cuda(), 'iou')


# ---- 5. graphs and detection.init -----------------------------------------------------------------------------------------------------------
def test_captured_graph_and_detection_init_in_a_child_process():
    """tests/iou_loss_graph_worker.py, in a process of its own (see there): forward and backward with the new box kinds captured in a HIP
    graph and replayed on two batches equal the eager results bit for bit; a training step through detection.init with TaskAlignedAssigner,
    valid_sampler, QualityFocalLoss(use_iou=False) and CompleteIoULoss, eager and with graph_hot_path=True, gives the same loss, which is
    the restatement's on the assigner's target."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, 'tests', 'iou_loss_graph_worker.py')], cwd=repo, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    print('iou_loss_graph_worker', res)
    assert res['timeouts'] == 0
    assert res['eager_loss'] == res['graphed_loss'] and np.isfinite(res['eager_loss']), res
    assert abs(res['eager_loss'] - res['restatement_loss']) <= 1e-4 + 1e-5 * abs(res['restatement_loss'])
