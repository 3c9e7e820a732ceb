"""GPU: COCO-style evaluation on libssdk (csrc/metrics.hip, ssdk_coco_eval_ex) against the numpy restatement of tests/coco_eval_reference.py,
on the hand-built cases, random cases and edge shapes of tests/coco_eval_cases.py.

Every input lies inside a larger allocation whose bytes are 0xFF on both sides; every output lies between such guards, which must keep
their bits, and is itself 0xFF before the call, as is the workspace.  Each case runs twice and must give the same bits.
What must agree: ranks, orders, flag bytes and npig exactly; precision, recall and the statistics within 1e-12 absolute --
they are fp64 quotients and means of integers below 2^31, a different but valid summation order moves them by a few 1e-16, and the smallest
real difference (one detection changing outcome) is above 1e-9 at these sizes."""
import ctypes

import numpy as np
import pytest
import torch

import coco_eval_cases as cases
import coco_eval_reference as ref
from single_shot_detection_amd import _lib
from single_shot_detection_amd.detection.metrics import coco_average_precision, coco_evaluation
from single_shot_detection_amd.detection.metrics.coco_evaluation import STAT_NAMES

pytestmark = pytest.mark.gpu

PAD = 256
TOL = 1e-12
SSDK_E_INVALID = -1


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
            self.t[PAD:PAD + nbytes] = torch.from_numpy(data.reshape(-1).view(np.uint8).copy()).cuda()
        self.ptr = ctypes.c_void_p(self.t.data_ptr() + PAD)

    def get(self, dtype, shape=(-1,)):
        return self.t[PAD:PAD + self.nbytes].cpu().numpy().view(dtype).reshape(shape).copy()

    def intact(self):
        return bool((self.t[:PAD] == 0xFF).all()) and bool((self.t[PAD + self.nbytes:] == 0xFF).all())


def tables_of(c):
    d = ref.default_tables()
    iou = np.ascontiguousarray(d[0] if c['iou_thrs'] is None else c['iou_thrs'], np.float64)
    rec = np.ascontiguousarray(d[1] if c['rec_thrs'] is None else c['rec_thrs'], np.float64)
    area = np.ascontiguousarray(d[2] if c['area_rngs'] is None else c['area_rngs'], np.float64).reshape(-1, 2)
    md = np.ascontiguousarray(d[3] if c['max_dets'] is None else c['max_dets'], np.int32)
    return iou, rec, area, md


def abi_run(c, what=''):
    """ssdk_coco_eval_ex on guarded buffers from a workspace of 0xFF bytes: a dict of numpy outputs."""
    lib = _lib.lib()
    pred, gts, K = c['pred'], c['gts'], c['num_classes']
    iou, rec, area, md = tables_of(c)
    T, R, A, M = iou.size, rec.size, area.shape[0], md.size
    stride = gts[0].shape[1] if len(gts) else 6
    counts = [g.shape[0] for g in gts]
    total, n = int(sum(counts)), pred.shape[0]
    rows = np.concatenate([g.reshape(-1, stride) for g in gts], 0).astype(np.float32) if total else np.zeros((0, stride), np.float32)
    inputs = dict(pred=pred, rows=rows, offs=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), iou=iou, rec=rec, area=area)
    if c['gt_areas'] is not None:
        inputs['gt_area'] = np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in c['gt_areas']]) if total else np.zeros(0, np.float64)
    if c['image_area_scale'] is not None:
        inputs['scale'] = np.asarray(c['image_area_scale'], np.float64)
    b = {k: Buf(v) for k, v in inputs.items()}
    ws_bytes = lib.ssdk_coco_eval_workspace_bytes(n, total, K, T, A)
    assert ws_bytes > 0
    sizes = dict(precision=8 * T * R * K * A * M, recall=8 * T * K * A * M, stats=8 * 12, rank=4 * n, flags=n * T * A, order=4 * n, npig=4 * K * A, ws=ws_bytes)
    b.update({k: Buf(nbytes=v) for k, v in sizes.items()})
    null = ctypes.c_void_p(None)
    rc = lib.ssdk_coco_eval_ex(b['pred'].ptr, n, b['rows'].ptr, stride, b['offs'].ptr, len(gts), total, K, b['gt_area'].ptr if 'gt_area' in b else null,
                               b['scale'].ptr if 'scale' in b else null, b['iou'].ptr, T, b['rec'].ptr, R, b['area'].ptr, A, ctypes.c_void_p(md.ctypes.data), M,
                               b['precision'].ptr, b['recall'].ptr, b['stats'].ptr, b['rank'].ptr, b['flags'].ptr, b['order'].ptr, b['npig'].ptr, b['ws'].ptr,
                               ws_bytes, _lib.current_stream())
    assert rc == 0, (what, rc, lib.ssdk_last_error_string())
    torch.cuda.synchronize()
    for k, v in b.items():
        assert v.intact(), (what, 'guard of', k)
    for k, v in inputs.items():
        assert np.array_equal(b[k].get(np.uint8), np.ascontiguousarray(v).reshape(-1).view(np.uint8)), (what, 'input', k)
    return dict(precision=b['precision'].get(np.float64, (T, R, K, A, M)), recall=b['recall'].get(np.float64, (T, K, A, M)), stats=b['stats'].get(np.float64),
                rank=b['rank'].get(np.int32), flags=b['flags'].get(np.uint8, (n, T * A)), order=b['order'].get(np.uint32).astype(np.int64),
                npig=b['npig'].get(np.int32, (K, A)))


_REF = {}


def reference(name):
    if name not in _REF:
        c = cases.gpu_cases()[name]
        _REF[name] = ref.evaluate(c['pred'], c['gts'], c['num_classes'], **cases.reference_kwargs(c))
    return _REF[name]


def compare(got, want, what):
    assert np.array_equal(got['npig'], want['npig']), (what, 'npig')
    assert np.array_equal(got['rank'], want['rank']), (what, 'rank', np.nonzero(got['rank'] != want['rank'])[0][:8])
    assert np.array_equal(got['order'], want['order']), (what, 'order')
    bad = np.nonzero((got['flags'] != want['flags']).any(1))[0]
    assert bad.size == 0, (what, 'flags of rows', bad[:8], got['flags'][bad[:2]], want['flags'][bad[:2]])
    for k in ('precision', 'recall'):
        assert got[k].shape == want[k].shape and np.isfinite(got[k]).all(), (what, k)
        err = float(np.abs(got[k] - want[k]).max()) if got[k].size else 0.0
        print(f'{what}: {k} max abs error {err:.3e}, bit-equal {np.array_equal(got[k], want[k])}')
        assert err <= TOL, (what, k, err)
    for i, k in enumerate(STAT_NAMES):
        print(f'{what}: {k} = {got["stats"][i]!r} (reference {want["stats"][k]!r})')
        assert abs(got['stats'][i] - want['stats'][k]) <= TOL, (what, k, got['stats'][i], want['stats'][k])


@pytest.mark.parametrize('name', sorted(cases.gpu_cases()))
def test_coco_eval_vs_reference(name):
    c = cases.gpu_cases()[name]
    got = abi_run(c, name)
    compare(got, reference(name), name)
    again = abi_run(c, name + ' (second run)')
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), (name, 'run to run', k)


@pytest.mark.parametrize('name', sorted(cases.hand_cases()))
def test_hand_cases_give_the_hand_worked_statistics(name):
    c, want = cases.hand_cases()[name]
    got = abi_run(c, name)['stats']
    for i, k in enumerate(STAT_NAMES):
        assert abs(got[i] - want[k]) <= TOL, (name, k, got[i], want[k])


def test_no_ground_truth_gives_minus_one_everywhere():
    got = abi_run(cases.gpu_cases()['special_no_ground_truth'])
    assert (got['stats'] == -1.0).all() and (got['precision'] == -1.0).all() and (got['recall'] == -1.0).all()


def test_both_matched_state_paths_are_reached():
    """64 gts of the class: the register mask; 65 and 130: the workspace bytes (csrc/metrics.hip kCocoMaskGts) -- and the matches there are real"""
    for n_det, n_gt in [(101, 64), (257, 65), (40, 130)]:
        want = reference(f'group_{n_det}_dets_{n_gt}_gts')
        assert (want['flags'] & 1).any() and (want['flags'] == 3).any() and (want['flags'] == 0).any(), (n_det, n_gt)


def test_refusals():
    lib = _lib.lib()
    c = cases.gpu_cases()['hand_iou_078']
    for kw in (dict(iou_thrs=np.linspace(.3, .95, 13), area_rngs=np.tile([[0.0, 1e10]], (5, 1))), dict(max_dets=np.array([100, 10, 1], np.int32)),
               dict(rec_thrs=np.zeros(0))):
        cc = dict(c, **kw)
        iou, rec, area, md = tables_of(cc)
        out = {k: Buf(nbytes=4096) for k in ('precision', 'recall', 'stats', 'ws')}
        inp = {k: Buf(v) for k, v in dict(pred=c['pred'], rows=c['gts'][0], offs=np.array([0, 1], np.int32), iou=iou, rec=np.zeros(1) if rec.size == 0 else rec,
                                          area=area).items()}
        rc = lib.ssdk_coco_eval(inp['pred'].ptr, 1, inp['rows'].ptr, 6, inp['offs'].ptr, 1, 1, 2, None, None, inp['iou'].ptr, iou.size, inp['rec'].ptr, rec.size,
                                inp['area'].ptr, area.shape[0], ctypes.c_void_p(md.ctypes.data), md.size, out['precision'].ptr, out['recall'].ptr,
                                out['stats'].ptr, out['ws'].ptr, 4096, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == SSDK_E_INVALID, (kw, rc)
        assert all(bool((v.t == 0xFF).all()) for v in out.values()), 'a refused call wrote something'
    # a workspace that is too small is refused as such
    iou, rec, area, md = tables_of(c)
    inp = {k: Buf(v) for k, v in dict(pred=c['pred'], rows=c['gts'][0], offs=np.array([0, 1], np.int32), iou=iou, rec=rec, area=area).items()}
    out = {k: Buf(nbytes=1 << 16) for k in ('precision', 'recall', 'stats')}
    ws = Buf(nbytes=256)
    rc = lib.ssdk_coco_eval(inp['pred'].ptr, 1, inp['rows'].ptr, 6, inp['offs'].ptr, 1, 1, 2, None, None, inp['iou'].ptr, 10, inp['rec'].ptr, 101, inp['area'].ptr, 4,
                            ctypes.c_void_p(md.ctypes.data), 3, out['precision'].ptr, out['recall'].ptr, out['stats'].ptr, ws.ptr, 256, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((ws.t == 0xFF).all()) and all(bool((v.t == 0xFF).all()) for v in out.values())


def _api(c, device, **kw):
    conv = (lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device))
    labels = {k: f'c{k}' for k in range(c['num_classes'])}
    return coco_evaluation(conv(c['pred']), [conv(g) for g in c['gts']], labels,
                           gt_areas=None if c['gt_areas'] is None else [conv(x) for x in c['gt_areas']],
                           image_area_scale=None if c['image_area_scale'] is None else conv(c['image_area_scale']), iou_thresholds=c['iou_thrs'],
                           recall_thresholds=c['rec_thrs'], area_ranges=c['area_rngs'], max_detections=c['max_dets'], **kw)


def test_python_api_host_and_device_inputs():
    name = 'random_small_crowd'
    c, want = cases.gpu_cases()[name], reference(name)
    host = _api(c, 'cpu', verbose=False, details=True)
    dev = _api(c, 'cuda', verbose=False, details=True)
    for k in STAT_NAMES:
        assert isinstance(host[k], float) and host[k] == dev[k] and abs(host[k] - want['stats'][k]) <= TOL, k
    for k in ('precision', 'recall', 'rank', 'flags', 'order', 'npig'):
        assert not host[k].is_cuda and torch.equal(host[k], dev[k]), k
    assert host['precision'].dtype == torch.float64 and np.abs(host['precision'].numpy() - want['precision']).max() <= TOL
    assert np.array_equal(host['flags'].numpy(), want['flags']) and np.array_equal(host['rank'].numpy(), want['rank'])
    assert np.array_equal(host['order'].numpy(), want['order']) and np.array_equal(host['npig'].numpy(), want['npig'])
    plain = _api(c, 'cuda', verbose=False)
    assert set(plain) == set(STAT_NAMES) | {'precision', 'recall'} and plain['AP'] == host['AP']
    labels = {k: f'c{k}' for k in range(c['num_classes'])}
    ap = coco_average_precision(torch.from_numpy(c['pred']), [torch.from_numpy(g) for g in c['gts']], labels, gt_areas=c['gt_areas'],
                                image_area_scale=c['image_area_scale'])
    assert isinstance(ap, float) and ap == host['AP']


def test_python_api_logs_the_twelve_lines(caplog):
    import logging
    c = cases.gpu_cases()['hand_iou_078']
    with caplog.at_level(logging.INFO):
        out = _api(c, 'cpu', verbose=True)
    lines = [r.getMessage() for r in caplog.records if 'Average' in r.getMessage()]
    assert len(lines) == 12 and lines[0].endswith('maxDets=100 ] = 0.600') and out['AP'] == pytest.approx(0.6, abs=TOL)
