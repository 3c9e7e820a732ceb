"""CPU: the numpy model of the grouped depthwise convolution (tests/dwgroup_reference.py) against torch's own F.conv2d(groups=C) and its
autograd, and the host-side argument checks of ssdk_depthwise_conv2d_group_* (they refuse before any launch, so no GPU is needed)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dwgroup_reference as ref
from single_shot_detection_amd import _lib


def _torch_all(xs, dys, weight, bias, stride, pad):
    w = torch.from_numpy(weight.astype(np.float64))[:, None].requires_grad_(True)
    b = torch.from_numpy(bias.astype(np.float64)).requires_grad_(True)
    xt = [torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True) for x in xs]
    ys = [F.conv2d(x, w, b, stride=stride, padding=pad, groups=w.shape[0]) for x in xt]
    grads = torch.autograd.grad(ys, xt + [w, b], [torch.from_numpy(d.astype(np.float64)).permute(0, 3, 1, 2) for d in dys])
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).numpy()   # noqa: E731
    return [nhwc(y) for y in ys], [nhwc(g) for g in grads[:len(xs)]], grads[-2][:, 0].numpy(), grads[-1].numpy()


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_model_is_torch_exactly_on_integer_operands(name):
    _, _, levels, k, stride, pad = ref.CASES[name]
    xs, dys, weight, bias = ref.integer_operands(name)
    ys, dxs, dw, db = _torch_all(xs, dys, weight, bias, stride, pad)
    for got, want in zip(ref.forward(xs, weight, bias, stride, pad, np.int64), ys):
        assert got.shape == want.shape and np.array_equal(got, want)
    for got, want in zip(ref.data_grad(dys, weight, levels, stride, pad, np.int64), dxs):
        assert got.shape == want.shape and np.array_equal(got, want)
    mdw, mdb = ref.weight_grad(xs, dys, k, stride, pad, np.int64)
    assert np.array_equal(mdw, dw) and np.array_equal(mdb, db)
    assert max(np.abs(a).max() for a in ys + dxs + [dw, db]) < 2 ** 24   # (what makes the fp32 kernels exact on these operands)


@pytest.mark.parametrize('name', ['c8_k3', 'c8_k5_shrinks', 'c8_k3_stride2', 'c32_8levels'])
def test_model_is_torch_on_normal_operands(name):
    _, _, levels, k, stride, pad = ref.CASES[name]
    xs, dys, weight, bias = ref.normal_operands(name)
    ys, dxs, dw, db = _torch_all(xs, dys, weight, bias, stride, pad)
    close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-12)   # noqa: E731  (two float64 sums of at most ~1500 terms of size ~1)
    assert all(close(a, b) for a, b in zip(ref.forward(xs, weight, bias, stride, pad), ys))
    assert all(close(a, b) for a, b in zip(ref.forward(xs, weight, None, stride, pad), [y - bias.astype(np.float64) for y in ys]))
    assert all(close(a, b) for a, b in zip(ref.data_grad(dys, weight, levels, stride, pad), dxs))
    mdw, mdb = ref.weight_grad(xs, dys, k, stride, pad)
    assert close(mdw, dw) and close(mdb, db)
    n_w, abs_w, n_b, abs_b = ref.weight_grad_terms(xs, dys, k, stride, pad)
    assert n_b == sum(d[..., 0].size for d in dys) and n_w.max() <= n_b and n_w.min() > 0
    assert (abs_w >= np.abs(mdw) - 1e-9).all() and (abs_b >= np.abs(mdb) - 1e-9).all()


# ---- the entry points' argument checks ---------------------------------------------------------------------------------------------

FAKE = 0x10000   # an aligned non-null "device pointer": a refused call never reaches a launch, so it is never read


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _ptrs(v):
    return (ctypes.c_void_p * len(v))(*v)


def _call(which, hs, ws, n, channels=8, ksize=3, xs=None, workspace_bytes=None):
    lib = _lib.lib()
    B, stride, pad = 2, 1, 1
    hs_a, ws_a = _ints(hs), _ints(ws)
    ptrs = _ptrs(xs if xs is not None else [FAKE] * len(hs))
    if which == 'workspace_bytes':
        return lib.ssdk_depthwise_conv2d_group_workspace_bytes(hs_a, ws_a, n, B, channels, ksize, stride, pad)
    if which == 'fwd':
        return lib.ssdk_depthwise_conv2d_group_fwd(ptrs, hs_a, ws_a, n, FAKE, FAKE, B, channels, ksize, stride, pad, _ptrs([FAKE] * len(hs)), None)
    need = lib.ssdk_depthwise_conv2d_group_workspace_bytes(hs_a, ws_a, n, B, channels, ksize, stride, pad)
    return lib.ssdk_depthwise_conv2d_group_bwd(ptrs, hs_a, ws_a, n, FAKE, _ptrs([FAKE] * len(hs)), B, channels, ksize, stride, pad,
                                               _ptrs([FAKE] * len(hs)), FAKE, FAKE, FAKE, need if workspace_bytes is None else workspace_bytes, None)


def _refused(status, which, *words):
    msg = _lib.lib().ssdk_last_error_string().decode()
    assert status < 0, (which, status)
    assert 'ssdk_depthwise_conv2d_group_' + which in msg, msg
    for word in words:
        assert word in msg, msg


@pytest.mark.parametrize('which', ['workspace_bytes', 'fwd', 'bwd'])
def test_entry_points_refuse_bad_arguments_before_any_launch(which):
    hs, ws = [7, 4, 2], [5, 3, 2]
    _refused(_call(which, hs, ws, 0), which, 'n_levels=0')
    _refused(_call(which, [3] * 9, [3] * 9, 9), which, 'n_levels=9')
    _refused(_call(which, hs, ws, 3, channels=6), which, 'level 0', 'C=6')
    _refused(_call(which, [7, 4, 2], [5, 3, 2], 3, ksize=5), which, 'level 2', 'k=5')   # 2 + 2 * 1 < 5: a level smaller than the kernel
    if which != 'workspace_bytes':
        _refused(_call(which, hs, ws, 3, xs=[FAKE, None, FAKE]), which, 'level 1')
    if which == 'bwd':
        need = _call('workspace_bytes', hs, ws, 3)
        _refused(_call(which, hs, ws, 3, workspace_bytes=need - 1), which, 'workspace')
        _refused(_call(which, hs, ws, 3, workspace_bytes=0), which, 'workspace')


def test_workspace_bytes_is_positive_and_independent_of_the_mode():
    lib = _lib.lib()
    before = lib.ssdk_get_deterministic()
    try:
        for name, (B, C, levels, k, stride, pad) in ref.CASES.items():
            hs, ws = _ints([h for h, _ in levels]), _ints([w for _, w in levels])
            sizes = []
            for mode in (0, 1, 0):
                lib.ssdk_set_deterministic(mode)
                sizes.append(lib.ssdk_depthwise_conv2d_group_workspace_bytes(hs, ws, len(levels), B, C, k, stride, pad))
            assert sizes[0] > 0 and sizes[0] == sizes[1] == sizes[2], (name, sizes)
            assert sizes[0] % ((k * k + 1) * C * 4) == 0, (name, sizes)   # whole chunks of (k*k + 1) rows of C floats (include/ssdk.h)
    finally:
        lib.ssdk_set_deterministic(before)
