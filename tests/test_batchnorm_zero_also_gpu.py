"""The zero-fill of a strided convolution's dx rides on the consumer norm's backward apply launch (ssdk_batchnorm_bwd_chained_ex,
ssdk_conv_desc::dx_is_zero, ops._DxLink).

(a) the entry point: zero_also ranges of 0, 1, 3, 4, 5, 1021 and 1 400 000 floats at a 4-byte-aligned, not 16-byte-aligned start, prefilled
    with NaN between NaN guard words: afterwards the range is all +0.0, the guards are untouched, and dx / dgamma / dbeta have the bits of
    the call without the side job; the same through three replays of a captured graph with the range poisoned again between replays.
(b) the block: conv2d_batch_norm, 3 x 3 / 2, 32 -> 64 channels, 2 x 9 x 9 input (tests/zero_also_cases.py): gradients against torch CPU at the
    bar test_conv_bn_gpu.py uses for the composition; the library's zero-fill counter shows that the backward zero-filled no dx.
(c) deterministic mode takes the path it took before, bit for bit: tests/golden/zero_also_det.npz, written by the build of the parent
    commit (tools/gen_golden_zero_also.py)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import zero_also_cases as cases
from conftest import GOLDEN
from single_shot_detection_amd import _lib, ops

pytestmark = pytest.mark.gpu

OK = 0
ROWS, CH = 300, 132        # (one of the composed shapes of test_batchnorm_kernels_gpu.py: C / 4 = 33, per-float4 constants in the apply kernel)
RANGES = [0, 1, 3, 4, 5, 1021, 1400000]
GUARD = 8                  # NaN guard words on either side


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope='module')
def norm_case():
    """Inputs of one backward call on the device, its sums buffers, and the outputs of the call WITHOUT the side job."""
    rng = np.random.default_rng(5)
    d = dict(x=torch.from_numpy(rng.standard_normal((ROWS, CH), dtype=np.float32)).cuda(),
             dy=torch.from_numpy(rng.standard_normal((ROWS, CH), dtype=np.float32)).cuda(),
             gamma=torch.from_numpy(rng.uniform(0.5, 1.5, CH).astype(np.float32)).cuda())
    d['y'] = torch.from_numpy(rng.standard_normal((ROWS, CH), dtype=np.float32)).cuda()
    d['mean'] = d['x'].mean(dim=0).contiguous()
    d['rstd'] = (1.0 / torch.sqrt(d['x'].var(dim=0, unbiased=False) + 1e-5)).contiguous()
    d['plain'] = _backward(d, None, 0)
    return d


def _backward(d, zero_also, n, sums=None, partner=None, out=None):
    """ssdk_batchnorm_bwd_chained_ex with ReLU mask; `sums` must hold zeros.  Returns (dx, dgamma, dbeta) tensors."""
    lib, st = _lib.lib(), _lib.current_stream()
    sums = torch.zeros(2 * CH + 2, dtype=torch.float64, device='cuda') if sums is None else sums
    partner = torch.zeros(2 * CH + 2, dtype=torch.float64, device='cuda') if partner is None else partner
    dx, dgamma, dbeta = out if out is not None else (torch.empty((ROWS, CH), device='cuda'), torch.empty(CH, device='cuda'), torch.empty(CH, device='cuda'))
    rc = lib.ssdk_batchnorm_bwd_chained_ex(_p(d['x']), _p(d['y']), _p(d['dy']), ROWS, CH, _p(d['gamma']), _p(d['mean']), _p(d['rstd']), 1, _p(dx),
                                           _p(dgamma), _p(dbeta), _p(sums), _p(partner), zero_also, n, st)
    assert rc == OK, _lib.lib().ssdk_last_error_string()
    torch.cuda.current_stream().synchronize()
    return dx, dgamma, dbeta


def _poisoned(n):
    """[GUARD NaN | pad | n NaN | GUARD NaN] with the range starting 4 bytes past a 16-byte boundary."""
    buf = torch.full((GUARD + 4 + n + GUARD,), float('nan'), device='cuda')
    start = GUARD + next(k for k in range(4) if (buf.data_ptr() + 4 * (GUARD + k)) % 16 == 4)
    assert (buf.data_ptr() + 4 * start) % 16 == 4
    return buf, start


def _check_range(buf, start, n):
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[start:start + n] == 0).all(), ('not +0.0 everywhere', n, int(np.flatnonzero(got[start:start + n])[0]))
    assert np.isnan(buf.cpu().numpy()[:start]).all() and np.isnan(buf.cpu().numpy()[start + n:]).all(), ('a guard word was written', n)


def _same_bits(a, b):
    return all(np.array_equal(u.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32)) for u, v in zip(a, b))


@pytest.mark.parametrize('n', RANGES)
def test_zero_also_fills_exactly_its_range_and_changes_no_output(norm_case, n):
    buf, start = _poisoned(n)
    got = _backward(norm_case, C.c_void_p(buf.data_ptr() + 4 * start), n)
    _check_range(buf, start, n)
    assert _same_bits(got, norm_case['plain']), 'dx / dgamma / dbeta differ from the call without the side job'


def test_null_pointer_or_zero_count_is_the_plain_call_and_bad_ranges_are_refused(norm_case):
    lib = _lib.lib()
    buf, start = _poisoned(16)
    assert _same_bits(_backward(norm_case, None, 0), norm_case['plain'])
    assert _same_bits(_backward(norm_case, C.c_void_p(buf.data_ptr() + 4 * start), 0), norm_case['plain'])
    assert _same_bits(_backward(norm_case, None, 4), norm_case['plain'])
    assert np.isnan(buf.cpu().numpy()).all()
    d, z = norm_case, torch.zeros(2 * CH + 2, dtype=torch.float64, device='cuda')
    dx = torch.full((ROWS, CH), 7.0, device='cuda')
    for also, n in ((C.c_void_p(buf.data_ptr() + 2), 4), (C.c_void_p(buf.data_ptr()), -1)):
        assert lib.ssdk_batchnorm_bwd_chained_ex(_p(d['x']), _p(d['y']), _p(d['dy']), ROWS, CH, _p(d['gamma']), _p(d['mean']), _p(d['rstd']), 1, _p(dx), _p(dx),
                                                 _p(dx), _p(z), _p(z.clone()), also, n, _lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert (dx == 7.0).all() and (z == 0).all()   # refused before the first launch


@pytest.mark.parametrize('n', [5, 1400000])
def test_three_replays_of_a_captured_graph_zero_the_range_again(norm_case, n):
    buf, start = _poisoned(n)
    sums, partner = torch.zeros(2 * CH + 2, dtype=torch.float64, device='cuda'), torch.zeros(2 * CH + 2, dtype=torch.float64, device='cuda')
    out = (torch.empty((ROWS, CH), device='cuda'), torch.empty(CH, device='cuda'), torch.empty(CH, device='cuda'))
    lib = _lib.lib()
    d = norm_case
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            rc = lib.ssdk_batchnorm_bwd_chained_ex(_p(d['x']), _p(d['y']), _p(d['dy']), ROWS, CH, _p(d['gamma']), _p(d['mean']), _p(d['rstd']), 1, _p(out[0]),
                                                   _p(out[1]), _p(out[2]), _p(sums), _p(partner), C.c_void_p(buf.data_ptr() + 4 * start), n,
                                                   _lib.current_stream())
    assert rc == OK
    for replay in range(3):
        buf.fill_(float('nan'))
        sums.zero_()            # (the layer's forward would have had its apply launch do this)
        for t in out:
            t.fill_(float('nan'))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _check_range(buf, start, n)
        assert _same_bits(out, norm_case['plain']), replay


# ---- (b), (c) the block -----------------------------------------------------------------------------------------------------------------

def _close(got, want, bar=1e-4, err_msg=''):
    """The bar of tests/test_conv_bn_gpu.py for this composition: |got - want| <= 1e-4 * (|want| + max|want|) for every element."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (err_msg, got.shape, want.shape)
    tol = bar * (np.abs(want) + float(np.abs(want).max())) + 1e-12
    err = np.abs(got - want)
    assert not (err > tol).any(), (err_msg, int((err > tol).sum()), float((err / tol).max()))


@pytest.fixture(scope='module')
def block_case():
    m, x, g = cases.block_and_input()
    ref = nn.Sequential(copy.deepcopy(m.conv), copy.deepcopy(m.bn), nn.ReLU()).train()
    xr = torch.from_numpy(x).requires_grad_(True)
    (ref(xr) * torch.from_numpy(g)).sum().backward()
    want = dict(x=xr.grad.numpy(), weight=ref[0].weight.grad.numpy(), gamma=ref[1].weight.grad.numpy(), beta=ref[1].bias.grad.numpy())
    return m, x, g, want


def _zero_fill_counts():
    out = (C.c_ulonglong * 2)()
    assert _lib.lib().ssdk_debug_zero_fill_counts(out) == OK
    return int(out[0]), int(out[1])


def _forward_then_counted_backward(m, x, g):
    """(gradients, zero-fill launches, floats they covered) of the block's backward pass alone."""
    m = m.cuda().train()
    for p in m.parameters():
        p.grad = None
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    loss = (m(xd) * torch.from_numpy(g).cuda()).sum()
    torch.cuda.synchronize()
    l0, f0 = _zero_fill_counts()
    loss.backward()
    torch.cuda.synchronize()
    l1, f1 = _zero_fill_counts()
    grads = dict(x=xd.grad.cpu().numpy(), weight=m.conv.weight.grad.cpu().numpy(), gamma=m.bn.weight.grad.cpu().numpy(), beta=m.bn.bias.grad.cpu().numpy())
    return grads, l1 - l0, f1 - f0


def test_block_gradients_and_no_zero_fill_of_dx(block_case, monkeypatch):
    m, x, g, want = block_case
    desc = _lib.ConvDesc()
    desc.stride = cases.STRIDE
    assert _lib.lib().ssdk_conv2d_dx_form(C.byref(desc)) == 1     # the scatter form: the case is about what the issue is about
    got, launches, floats = _forward_then_counted_backward(copy.deepcopy(m), x, g)
    for k in ('x', 'weight', 'gamma', 'beta'):
        _close(got[k], want[k], err_msg=k)
    # what the backward zero-fills without the hand-over, measured on the same build: the same block with the link switched off
    monkeypatch.setattr(ops, '_NO_DX_ZERO_BY_NORM', True)
    old, launches_old, floats_old = _forward_then_counted_backward(copy.deepcopy(m), x, g)
    print('zero-fill launches / floats in the backward: with the hand-over', launches, floats, 'without', launches_old, floats_old)
    assert floats_old - floats == x.size, 'the backward still zero-filled dx (or something else changed)'
    assert floats == m.conv.weight.numel()            # what is left: the weight gradient's accumulator
    for k in ('x', 'weight', 'gamma', 'beta'):        # the scatter's atomics add in any order: equal to rounding, not to the bit
        _close(got[k], old[k], err_msg=k + ' against the separate zero-fill')


def test_deterministic_mode_takes_the_path_it_took_before(block_case):
    m, x, g, want = block_case
    golden = np.load(os.path.join(GOLDEN, 'zero_also_det.npz'))
    with ops.deterministic():
        desc = _lib.ConvDesc()
        desc.stride = cases.STRIDE
        assert _lib.lib().ssdk_conv2d_dx_form(C.byref(desc)) == 2
        got, launches, floats = _forward_then_counted_backward(copy.deepcopy(m), x, g)
    assert floats == 0, 'deterministic mode zero-fills nothing in this backward'
    for k in ('x', 'weight', 'gamma', 'beta'):
        assert np.array_equal(got[k].view(np.uint32), golden[k].view(np.uint32)), k
        _close(got[k], want[k], err_msg=k)
