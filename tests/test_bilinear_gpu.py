"""GPU: the bilinear top-down step (ssdk_upsample_bilinear_add_fwd / _bwd, ops.upsample_add / ops.upsample with mode='bilinear') and the
necks that use it -- bit for bit against torch on the CPU where the arithmetic is exact, within derived bounds against a float64 model
(tests/bilinear_reference.py) for every pair of sizes, as an adjoint pair, run to run, against the REFERENCE's own modules
(tests/golden/necks_bilinear.npz, tools/gen_golden_bilinear.py), under a dispatch recorder, and with the default mode untouched."""
import contextlib
import logging
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bilinear_cases
import bilinear_reference as br
from conftest import GOLDEN
from single_shot_detection_amd import _lib, ops
from single_shot_detection_amd.bf.modules import conv, features

pytestmark = pytest.mark.gpu

MODS = types.SimpleNamespace(FeaturePyramid=features.FeaturePyramid, ThinnedUshapeModule=features.ThinnedUshapeModule,
                             MultilevelFeaturePyramid=features.MultilevelFeaturePyramid)
BAR = 2e-5   # the reference-golden bar of test_blocks_golden_gpu.py
OK = 0


def _cl(a):
    """A [B, C, H, W] numpy array as a channels_last fp32 tensor on the GPU."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().contiguous(memory_format=torch.channels_last)


def _p(t):
    return _lib.ptr(t)


def _raw(entry, *tensors_and_sizes):
    return getattr(_lib.lib(), entry)(*tensors_and_sizes, _lib.current_stream())


def _fwd_raw(coarse, hf, wf, fine=None):
    """The entry point itself on NCHW numpy arrays; the output buffer is pre-filled, so an element the kernel does not write shows."""
    B, C, hc, wc = coarse.shape
    cd, fd = _cl(coarse), (None if fine is None else _cl(fine))
    out = torch.full((B, C, hf, wf), 5.0, device='cuda').contiguous(memory_format=torch.channels_last)
    assert _raw('ssdk_upsample_bilinear_add_fwd', _p(fd), _p(cd), B, hf, wf, hc, wc, C, _p(out)) == OK
    return out.cpu().numpy()


def _bwd_raw(dout, hc, wc):
    B, C, hf, wf = dout.shape
    gd = _cl(dout)
    dc = torch.full((B, C, hc, wc), 5.0, device='cuda').contiguous(memory_format=torch.channels_last)
    assert _raw('ssdk_upsample_bilinear_add_bwd', _p(gd), B, hf, wf, hc, wc, C, _p(dc)) == OK
    return dc.cpu().numpy()


# ---- 1. exact ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [4, 12])
@pytest.mark.parametrize('hc,wc,hf,wf', [(1, 1, 2, 2), (2, 3, 4, 6), (5, 7, 10, 14), (16, 16, 32, 32)])
def test_exact_2x_equals_torch_cpu_bit_for_bit(hc, wc, hf, wf, C):
    """At exact 2 x the weights are 1/4 and 3/4: on integer operands in [-64, 64] every product and sum is exact in fp32, in any order."""
    rng = np.random.default_rng(100 * hc + C)
    B = 2
    x = rng.integers(-64, 65, (B, C, hc, wc)).astype(np.float32)
    f = rng.integers(-64, 65, (B, C, hf, wf)).astype(np.float32)
    g = rng.integers(-64, 65, (B, C, hf, wf)).astype(np.float32)
    xt = torch.from_numpy(x).requires_grad_(True)
    up = F.interpolate(xt, size=(hf, wf), mode='bilinear')
    up.backward(torch.from_numpy(g))
    assert np.array_equal(_fwd_raw(x, hf, wf), up.detach().numpy())
    assert np.array_equal(_fwd_raw(x, hf, wf, f), (torch.from_numpy(f) + up.detach()).numpy())
    assert np.array_equal(_bwd_raw(g, hc, wc), xt.grad.numpy())
    # and through ops / autograd
    xg, fg = _cl(x).requires_grad_(True), _cl(f).requires_grad_(True)
    y = ops.upsample_add(fg, xg, 'bilinear')
    y.backward(_cl(g))
    assert np.array_equal(y.detach().cpu().numpy(), (torch.from_numpy(f) + up.detach()).numpy())
    assert np.array_equal(xg.grad.cpu().numpy(), xt.grad.numpy()) and np.array_equal(fg.grad.cpu().numpy(), g)
    xg = _cl(x).requires_grad_(True)
    y = ops.upsample(xg, (hf, wf), 'bilinear')
    y.backward(_cl(g))
    assert np.array_equal(y.detach().cpu().numpy(), up.detach().numpy()) and np.array_equal(xg.grad.cpu().numpy(), xt.grad.numpy())


@pytest.mark.parametrize('h,w', [(1, 1), (5, 7), (16, 16)])
def test_equal_sizes_are_the_identity_bit_for_bit(h, w):
    rng = np.random.default_rng(h)
    x = rng.standard_normal((2, 12, h, w), dtype=np.float32)
    f = rng.standard_normal((2, 12, h, w), dtype=np.float32)
    assert np.array_equal(_fwd_raw(x, h, w), x)
    assert np.array_equal(_fwd_raw(x, h, w, f), f + x)
    assert np.array_equal(_bwd_raw(x, h, w), x)


# ---- 2. every pair of sizes against the float64 model ---------------------------------------------------------------------------------

def _pairs(axis):
    """hc, wc, hf, wf: every 1 <= in, out <= 24 along `axis` (up, equal, down), the other axis fixed at 4 -> 7."""
    for n_in in range(1, 25):
        for n_out in range(1, 25):
            yield (n_in, 4, n_out, 7) if axis == 'h' else (4, n_in, 7, n_out)


@pytest.mark.parametrize('axis', ['h', 'w'])
def test_forward_and_backward_within_the_bounds_for_every_size_pair(axis):
    rng = np.random.default_rng(21)
    B, C = 2, 8
    worst_f = worst_b = 0.0
    for hc, wc, hf, wf in _pairs(axis):
        x = rng.standard_normal((B, C, hc, wc), dtype=np.float32)
        f = rng.standard_normal((B, C, hf, wf), dtype=np.float32)
        g = rng.standard_normal((B, C, hf, wf), dtype=np.float32)
        up = br.forward(x, hf, wf)
        mx = np.abs(x).max()
        e0 = np.abs(_fwd_raw(x, hf, wf) - up) / br.forward_bound(hc, wc, mx)
        e1 = np.abs(_fwd_raw(x, hf, wf, f) - (f.astype(np.float64) + up)) / br.forward_bound(hc, wc, mx, f.astype(np.float64) + up)
        eb = np.abs(_bwd_raw(g, hc, wc) - br.backward(g, hc, wc)) / br.backward_bound(hc, wc, hf, wf, np.abs(g).max())
        worst_f, worst_b = max(worst_f, e0.max(), e1.max()), max(worst_b, eb.max())
        assert e0.max() <= 1.0 and e1.max() <= 1.0 and eb.max() <= 1.0, (hc, wc, hf, wf, e0.max(), e1.max(), eb.max())
    print(f'axis {axis}: worst forward {worst_f:.3f}, worst backward {worst_b:.3f} of the bound')


# ---- 3. adjoint ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('hc,wc,hf,wf', [(3, 3, 7, 7), (10, 10, 19, 19), (19, 19, 10, 10), (1, 1, 5, 5), (3, 10, 7, 19), (19, 1, 10, 5)])
def test_backward_is_the_adjoint_of_the_forward(hc, wc, hf, wf):
    """<up(x), g> == <x, up^T(g)>: a gather window that misses a contributor breaks it by a whole term.  Both sides summed in float64; the
    tolerance is the backward bound (per element of dcoarse) times the number of elements of dcoarse."""
    rng = np.random.default_rng(hc * 31 + hf)
    x = rng.standard_normal((2, 8, hc, wc), dtype=np.float32)
    g = rng.standard_normal((2, 8, hf, wf), dtype=np.float32)
    lhs = (_fwd_raw(x, hf, wf).astype(np.float64) * g).sum()
    rhs = (x.astype(np.float64) * _bwd_raw(g, hc, wc)).sum()
    tol = br.backward_bound(hc, wc, hf, wf, np.abs(g).max()) * x.size
    print(f'{hc}x{wc} -> {hf}x{wf}: |lhs - rhs| = {abs(lhs - rhs):.3e}, tolerance {tol:.3e}')
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


# ---- 4. run to run ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('deterministic', [False, True])
def test_two_runs_give_identical_bits(deterministic):
    rng = np.random.default_rng(5)
    B, C, hc, wc, hf, wf = 4, 32, 10, 7, 19, 13
    x = rng.standard_normal((B, C, hc, wc), dtype=np.float32)
    f = rng.standard_normal((B, C, hf, wf), dtype=np.float32)
    g = rng.standard_normal((B, C, hf, wf), dtype=np.float32)
    runs = []
    with (ops.deterministic() if deterministic else contextlib.nullcontext()):
        for _ in range(2):
            xg, fg = _cl(x).requires_grad_(True), _cl(f).requires_grad_(True)
            y = ops.upsample_add(fg, xg, 'bilinear')
            y.backward(_cl(g))
            runs.append((y.detach().clone(), xg.grad, fg.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert np.abs(runs[0][1].cpu().numpy() - br.backward(g, hc, wc)).max() <= br.backward_bound(hc, wc, hf, wf, np.abs(g).max())


# ---- 5. against the reference's own modules ------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def golden_necks():
    return np.load(os.path.join(GOLDEN, 'necks_bilinear.npz'))


@pytest.mark.parametrize('case', sorted(bilinear_cases.CASES))
def test_neck_vs_reference_golden(case, golden_necks):
    """test_blocks_golden_gpu.py's comparison: |diff| <= 2e-5 * (|ref| + max|ref|) for every stored element, checksums as there."""
    got = bilinear_cases.run_case(case, MODS, torch.device('cuda'))
    want_keys = sorted(k for k in golden_necks.files if k.startswith(case + '/'))
    assert sorted(got) == want_keys, (sorted(set(want_keys) ^ set(got))[:10])
    worst = 0.0
    for key in want_keys:
        ref, val = golden_necks[key], got[key]
        if key.endswith('__shape'):
            assert np.array_equal(ref, val), key
        elif '/buffers/' in key and key.endswith('num_batches_tracked'):
            assert np.array_equal(ref, val), (key, ref, val)
        elif key.endswith('__sum_l2'):
            l2 = float(ref[1])
            assert abs(val[1] - ref[1]) <= BAR * l2 + 1e-12, (key, val, ref)
            assert abs(val[0] - ref[0]) <= 10 * BAR * l2 + 1e-12, (key, val, ref)
        else:
            scale = float(np.abs(ref).max()) if ref.size else 0.0
            err = np.abs(val.astype(np.float64) - ref.astype(np.float64))
            tol = BAR * (np.abs(ref) + scale) + 1e-12
            bad = err > tol
            worst = max(worst, float((err / tol).max()) if err.size else 0.0)
            assert not bad.any(), (key, int(bad.sum()), float((err / tol).max()), scale)
    print(f'{case}: worst element at {worst:.3f} of the bar')


# ---- 6. no stock kernel in the top-down path ---------------------------------------------------------------------------------------------

BANNED = ('aten.upsample_bilinear2d', 'aten.upsample_nearest2d', 'aten._upsample')   # (the backward ops' names start the same way)


def _recorder():
    from torch.utils._python_dispatch import TorchDispatchMode

    class _Rec(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))
    return _Rec()


def _record(case, mode):
    """Forward and backward op names of the case's module in train(), built with `mode`."""
    module = bilinear_cases.build(case, MODS).cuda().train()
    for m in module.modules():
        if hasattr(m, 'interpolation_mode'):
            m.interpolation_mode = mode
    shape = bilinear_cases.CASES[case][1]
    x = torch.from_numpy(np.random.default_rng(3).standard_normal(shape, dtype=np.float32)).cuda().requires_grad_(True)
    fwd, bwd = _recorder(), _recorder()
    with fwd:
        outs = bilinear_cases.CASES[case][2](module, x)
    with bwd:
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
    assert x.grad is not None and fwd.names and bwd.names
    return fwd.names, bwd.names


@pytest.mark.parametrize('case', ['fpn_bilinear', 'mlfp_bilinear'])
def test_no_stock_kernel_in_the_top_down_path(case, caplog):
    """No torch interpolation, forward or backward, no tensor add from the top-down step -- the forward has exactly as many aten.add.Tensor
    calls as the same module in 'nearest' mode, whose step is one libssdk launch -- and no fall-back warning."""
    conv._warned.discard(('interpolate', "interpolation_mode='bilinear'"))
    near_f, _ = _record(case, 'nearest')
    with caplog.at_level(logging.WARNING):
        bil_f, bil_b = _record(case, 'bilinear')
    bad = [n for n in bil_f + bil_b if n.startswith(BANNED)]
    assert not bad, bad
    assert bil_f.count('aten.add.Tensor') == near_f.count('aten.add.Tensor'), (bil_f.count('aten.add.Tensor'), near_f.count('aten.add.Tensor'))
    assert not [r for r in caplog.records if 'interpolat' in r.getMessage()], [r.getMessage() for r in caplog.records]


# ---- 7. the default mode is untouched ----------------------------------------------------------------------------------------------------

def test_default_mode_is_the_nearest_entry_point_bit_for_bit():
    rng = np.random.default_rng(13)
    B, C, hc, wc, hf, wf = 2, 8, 7, 7, 13, 13
    c, f = _cl(rng.standard_normal((B, C, hc, wc), dtype=np.float32)), _cl(rng.standard_normal((B, C, hf, wf), dtype=np.float32))
    want_add, want_up = torch.empty_like(f), torch.empty_like(f)
    assert _raw('ssdk_upsample_nearest_add_fwd', _p(f), _p(c), B, hf, wf, hc, wc, C, _p(want_add)) == OK
    assert _raw('ssdk_upsample_nearest_add_fwd', None, _p(c), B, hf, wf, hc, wc, C, _p(want_up)) == OK
    assert torch.equal(ops.upsample_add(f, c), want_add) and torch.equal(ops.upsample_add(f, c, 'nearest'), want_add)
    assert torch.equal(ops.upsample_nearest(c, (hf, wf)), want_up) and torch.equal(ops.upsample(c, (hf, wf)), want_up)
    assert torch.equal(want_up.cpu(), F.interpolate(c.cpu(), size=(hf, wf), mode='nearest'))
    assert not torch.equal(ops.upsample(c, (hf, wf), 'bilinear'), want_up)
