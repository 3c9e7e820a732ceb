"""GPU: ssdk_depthwise_conv2d_group_* through the ctypes binding, on the smallest shapes that reach every branch (tests/dwgroup_reference.py
holds the cases and the numpy model).

* integer operands: forward, dx, dw and db equal the int64 model EXACTLY (every sum is an integer far below 2^24, so no summation order
  can change it);
* every level's y and dx are the bits of the single-level entry points;
* float operands: each element of dw / db is within 1.01 * n * 2^-24 * sum |terms| of the float64 model -- the bound of ANY order of
  adding n fp32 terms, with n and the sum taken from the model;
* dw / db are the same bits run after run and in both modes of ssdk_set_deterministic;
* forward + backward through ops, captured in one HIP graph and replayed twice, are the eager bits (child process).

The workgroup of the weight gradient splits its 256 threads by the channel count: 16 quads x 16 phases up to 64 channels (the cases with
8, 16, 32 and 64 channels), 32 x 8 up to 128 (c128_chunks), 64 x 4 beyond (c260_k3, whose second channel block holds one quad)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dwgroup_reference as ref
from conftest import REPO, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _workspace_bytes(name):
    from single_shot_detection_amd import _lib
    B, C, levels, k, stride, pad = ref.CASES[name]
    return _lib.lib().ssdk_depthwise_conv2d_group_workspace_bytes(_ints([h for h, _ in levels]), _ints([w for _, w in levels]), len(levels), B, C, k,
                                                                  stride, pad)


def run_group(name, xs, dys, weight, bias, want_dx=True, want_db=True, levels=None):
    """-> ys, dxs (None where not asked for), dw, db as numpy arrays.  ``want_dx``: True, None (dxs == NULL) or a per-level mask."""
    import torch
    from single_shot_detection_amd import _lib
    lib = _lib.lib()
    B, C, case_levels, k, stride, pad = ref.CASES[name]
    levels = case_levels if levels is None else levels
    n = len(levels)
    hs, ws = _ints([h for h, _ in levels]), _ints([w for _, w in levels])
    stream = _lib.current_stream()
    x_d, dy_d, w_d, b_d = [_dev(x) for x in xs], [_dev(d) for d in dys], _dev(weight), _dev(bias)
    y_d = [torch.full(d.shape, float('nan'), device='cuda') for d in dy_d]
    _lib.check(lib.ssdk_depthwise_conv2d_group_fwd(_ptrs(x_d), hs, ws, n, w_d.data_ptr(), None if b_d is None else b_d.data_ptr(), B, C, k, stride, pad,
                                                   _ptrs(y_d), stream), 'ssdk_depthwise_conv2d_group_fwd')
    mask = [bool(want_dx)] * n if want_dx is None or isinstance(want_dx, bool) else list(want_dx)
    dx_d = [torch.full(x.shape, float('nan'), device='cuda') if m else None for x, m in zip(x_d, mask)]
    dw_d = torch.full((C, k, k), float('nan'), device='cuda')
    db_d = torch.full((C,), float('nan'), device='cuda') if want_db else None
    nbytes = lib.ssdk_depthwise_conv2d_group_workspace_bytes(hs, ws, n, B, C, k, stride, pad)
    assert nbytes > 0
    work = torch.full((nbytes // 4,), float('nan'), device='cuda')
    _lib.check(lib.ssdk_depthwise_conv2d_group_bwd(_ptrs(x_d), hs, ws, n, w_d.data_ptr(), _ptrs(dy_d), B, C, k, stride, pad,
                                                   None if want_dx is None else _ptrs(dx_d), dw_d.data_ptr(), None if db_d is None else db_d.data_ptr(),
                                                   work.data_ptr(), nbytes, stream), 'ssdk_depthwise_conv2d_group_bwd')
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()   # noqa: E731
    return [host(y) for y in y_d], [host(d) for d in dx_d], host(dw_d), host(db_d)


_model_cache = {}


def model(name):
    """The int64 model of a case's integer operands, computed once."""
    if name not in _model_cache:
        _, _, levels, k, stride, pad = ref.CASES[name]
        xs, dys, weight, bias = ref.integer_operands(name)
        _model_cache[name] = (ref.forward(xs, weight, bias, stride, pad, np.int64), ref.forward(xs, weight, None, stride, pad, np.int64),
                              ref.data_grad(dys, weight, levels, stride, pad, np.int64)) + ref.weight_grad(xs, dys, k, stride, pad, np.int64)
    return _model_cache[name]


def _exact(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, got.astype(np.int64)), what


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_integer_operands_equal_the_int64_model_exactly(name):
    xs, dys, weight, bias = ref.integer_operands(name)
    ys, dxs, dw, db = run_group(name, xs, dys, weight, bias)
    want_y, _, want_dx, want_dw, want_db = model(name)
    for l in range(len(xs)):
        _exact(ys[l], want_y[l], f'y of level {l}')
        _exact(dxs[l], want_dx[l], f'dx of level {l}')
    _exact(dw, want_dw, 'dw')
    _exact(db, want_db, 'db')


def test_without_bias_and_without_db():
    name = 'c32_8levels'
    xs, dys, weight, _ = ref.integer_operands(name)
    ys, dxs, dw, db = run_group(name, xs, dys, weight, None, want_db=False)
    _, want_y, want_dx, want_dw, _ = model(name)
    assert db is None
    for l in range(len(xs)):
        _exact(ys[l], want_y[l], f'y of level {l}')
        _exact(dxs[l], want_dx[l], f'dx of level {l}')
    _exact(dw, want_dw, 'dw')


@pytest.mark.parametrize('want_dx', [None, (True, False, True, True)], ids=['dxs_null', 'one_null_entry'])
def test_levels_without_a_data_gradient(want_dx):
    name = 'c8_k3'
    xs, dys, weight, bias = ref.integer_operands(name)
    _, dxs, dw, db = run_group(name, xs, dys, weight, bias, want_dx=want_dx)
    _, _, want_dx_model, want_dw, want_db = model(name)
    for l, dx in enumerate(dxs):
        if want_dx is not None and want_dx[l]:
            _exact(dx, want_dx_model[l], f'dx of level {l}')
        else:
            assert dx is None
    _exact(dw, want_dw, 'dw')
    _exact(db, want_db, 'db')


@pytest.mark.parametrize('name', ['c64_chunks', 'c128_chunks', 'c16_chunks'])
def test_chunk_boundaries_fall_inside_levels(name):
    """What makes test_integer_operands_equal_the_int64_model_exactly[*_chunks] a test of the chunked reduction: several chunks, cut where
    the levels are not (the layout include/ssdk.h states: chunks of ceil(P / clamp(P / 256, 1, 512)) pixels)."""
    B, C, levels, k, stride, pad = ref.CASES[name]
    chunks, rest = divmod(_workspace_bytes(name), (k * k + 1) * C * 4)
    assert rest == 0 and chunks >= 4
    level_ends = np.cumsum([B * ref.out_dim(h, k, stride, pad) * ref.out_dim(w, k, stride, pad) for h, w in levels])
    P = int(level_ends[-1])
    assert P == 1316
    ppb = -(-P // min(max(P // 256, 1), 512))
    assert -(-P // ppb) == chunks
    cuts = set(range(ppb, P, ppb))
    assert not set(level_ends[:-1].tolist()) <= cuts           # no chunk boundary coincides with every level boundary ...
    assert all(c not in level_ends for c in cuts), cuts          # ... (in fact with none: every cut is inside a level)


def _single_level(x, dy, weight, bias, B, C, k, stride, pad):
    import torch
    from single_shot_detection_amd import _lib
    lib = _lib.lib()
    x_d, dy_d, w_d, b_d = _dev(x), _dev(dy), _dev(weight), _dev(bias)
    H, W = x.shape[1:3]
    y_d, dx_d = torch.empty_like(dy_d), torch.empty_like(x_d)
    dw_d, db_d = torch.empty_like(w_d), torch.empty_like(b_d)
    stream = _lib.current_stream()
    _lib.check(lib.ssdk_depthwise_conv2d_fwd(x_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), B, H, W, C, k, stride, pad, y_d.data_ptr(), stream), 'fwd')
    _lib.check(lib.ssdk_depthwise_conv2d_bwd(x_d.data_ptr(), w_d.data_ptr(), dy_d.data_ptr(), B, H, W, C, k, stride, pad, dx_d.data_ptr(), dw_d.data_ptr(),
                                             db_d.data_ptr(), 0, stream), 'bwd')
    torch.cuda.synchronize()
    return y_d.cpu().numpy(), dx_d.cpu().numpy()


@pytest.mark.parametrize('name,n_levels', [('c8_k3', 4), ('c260_k3', 4), ('c8_k3', 1)])
def test_every_level_is_the_single_level_entry_points_bits(name, n_levels):
    B, C, levels, k, stride, pad = ref.CASES[name]
    xs, dys, weight, bias = ref.normal_operands(name)
    xs, dys, levels = xs[:n_levels], dys[:n_levels], levels[:n_levels]
    ys, dxs, _, _ = run_group(name, xs, dys, weight, bias, levels=levels)
    for l in range(n_levels):
        y, dx = _single_level(xs[l], dys[l], weight, bias, B, C, k, stride, pad)
        assert np.array_equal(ys[l].view(np.uint32), y.view(np.uint32)), f'y of level {l}'
        assert np.array_equal(dxs[l].view(np.uint32), dx.view(np.uint32)), f'dx of level {l}'


@pytest.mark.parametrize('name', ['c8_k3', 'c260_k3', 'c8_k5_shrinks', 'c8_k3_stride2', 'c64_chunks', 'c128_chunks'])
def test_float_weight_gradient_within_the_bound_of_any_summation_order(name):
    _, _, levels, k, stride, pad = ref.CASES[name]
    xs, dys, weight, bias = ref.normal_operands(name)
    _, _, dw, db = run_group(name, xs, dys, weight, bias, want_dx=None)
    want_dw, want_db = ref.weight_grad(xs, dys, k, stride, pad)
    n_w, abs_w, n_b, abs_b = ref.weight_grad_terms(xs, dys, k, stride, pad)
    # each product dy * x is itself rounded once into the fmaf chain's running sum: that rounding is one of the n of the bound
    bound_w = 1.01 * n_w[None] * 2.0 ** -24 * abs_w
    bound_b = 1.01 * n_b * 2.0 ** -24 * abs_b
    err_w, err_b = np.abs(dw.astype(np.float64) - want_dw), np.abs(db.astype(np.float64) - want_db)
    print(f'{name}: dw error / bound max {np.max(err_w / bound_w):.3g}, db error / bound max {np.max(err_b / bound_b):.3g}')
    assert (err_w <= bound_w).all(), float(np.max(err_w / bound_w))
    assert (err_b <= bound_b).all(), float(np.max(err_b / bound_b))


@pytest.mark.parametrize('name', ['c260_k3', 'c64_chunks'])
def test_weight_gradient_bits_repeat_and_do_not_depend_on_the_mode(name):
    from single_shot_detection_amd import ops
    xs, dys, weight, bias = ref.normal_operands(name)
    before = ops.is_deterministic()
    runs = []
    try:
        for mode in (False, False, True, True, False):
            ops.set_deterministic(mode)
            _, _, dw, db = run_group(name, xs, dys, weight, bias, want_dx=None)
            runs.append((dw.view(np.uint32), db.view(np.uint32)))
    finally:
        ops.set_deterministic(before)
    for dw, db in runs[1:]:
        assert np.array_equal(dw, runs[0][0]) and np.array_equal(db, runs[0][1])


def test_forward_and_backward_replay_from_a_captured_graph():
    """ops.depthwise_conv2d on a list and its backward inside one torch.cuda.graph, replayed twice: the eager bits (in a fresh process,
    as tests/bipartite_graph_worker.py is)."""
    out = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'dwgroup_graph_worker.py')], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res['replays'] == 2 and res['tensors_compared'] == 2 * (8 + 8 + 2)
