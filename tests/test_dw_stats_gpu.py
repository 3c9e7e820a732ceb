"""GPU: the two forward entry points of a depthwise Conv2dBn block through the C ABI (csrc/norm.hip) --
ssdk_depthwise_conv2d_stats_fwd (training: the stencil's launch adds the BatchNorm statistics of its output to the layer's fp64 `sums`) and
ssdk_depthwise_conv2d_norm_fwd (evaluation: the norm (+ ReLU) in the stencil's epilogue).

Shapes -- the smallest at which each index path can go wrong, each with and without a bias:
  C 8, 1 x 1 map, k3 s1 p1, B 1          every tap but the centre is padding, one row
  C 8, 3 x 3, k3 s2 p0 -> 1 x 1
  C 132 (C / 4 = 33), 5 x 7, B 3, k3 s1 p1   the last slab of channel quads is a single column
  C 16, 9 x 7: k5 s1 p2; k3 s2 p1 -> 5 x 4; k3 s2 p0 -> 4 x 3
  B 2, 48 x 48, C 1024                    1 179 648 float4: several trips of every thread

Checks:
  1. y equals ssdk_depthwise_conv2d_fwd's bit for bit (both entries share dw_fwd_point);
  2. exact operands: x and w multiples of 1/4 with |x| <= 4, |w| <= 2 (<= 1 for the 5 x 5 kernel), the bias a multiple of 1/4, so every y is
     a multiple of 1/16 below 128 (exact in the fp32 chain) and every y^2 a multiple of 2^-8 below 2^14: over at most 4608 rows every
     partial sum is exact in fp64, so sums[0 .. 2C) must EQUAL the fp64 sums of the downloaded y whatever order the atomics retire in,
     sums[2C] == rows, and a second call into the same buffer gives exactly twice the sums;
  3. N(0, 1) data with one channel whose mean is 100 standard deviations: |sum error| <= 2 * rows * 2^-53 * sum |term| against the sums of
     the kernel's own y (the terms, y and y^2 of fp32 values, are exact in fp64: this is the bound of an fp64 sum of `rows` terms), and the
     block's output -- the statistics entry followed by ssdk_batchnorm_apply_chained -- is within batchnorm_reference.elementwise_bar;
  4. the inference entry equals the stencil followed by ssdk_batchnorm_fwd(training = 0), relu 0 and 1, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import batchnorm_reference as bnref
from single_shot_detection_amd import _lib

pytestmark = pytest.mark.gpu

OK = 0
F32 = np.float32
MOMENTUM, EPS = float(F32(0.1)), float(F32(1e-5))

# (B, H, W, C, k, stride, pad)
SHAPES = [(1, 1, 1, 8, 3, 1, 1), (2, 3, 3, 8, 3, 2, 0), (3, 5, 7, 132, 3, 1, 1), (2, 9, 7, 16, 5, 1, 2), (2, 9, 7, 16, 3, 2, 1), (2, 9, 7, 16, 3, 2, 0),
          (2, 48, 48, 1024, 3, 1, 1)]
IDS = ['c8_1x1', 'c8_3x3_s2p0', 'c132_5x7', 'c16_k5', 'c16_s2p1', 'c16_s2p0', 'c1024_48x48']
OUT = {(2, 3, 3, 8, 3, 2, 0): (1, 1), (2, 9, 7, 16, 3, 2, 1): (5, 4), (2, 9, 7, 16, 3, 2, 0): (4, 3)}

_alive = []


@pytest.fixture(autouse=True)
def _device_buffers_live_until_the_test_ends():
    """The library is handed raw pointers: everything _dev makes stays alive until the test is over."""
    yield
    del _alive[:]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()   # (a copy: the shared operands are read-only)
    _alive.append(t)
    return t


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _out_hw(shape):
    B, H, W, C_, k, s, p = shape
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    assert OUT.get(shape, (ho, wo)) == (ho, wo)
    return ho, wo


HOT = 1   # the channel whose mean is 100 standard deviations (check 3)


@functools.lru_cache(maxsize=4)
def _operands(shape, kind):
    """x [B, H, W, C], w [C, k * k], bias [C] (the tests pass it or not), read-only and shared.  kind 'exact': multiples of 1/4;
    'normal': N(0, 1), channel HOT a centre-tap identity filter over 100 + N(0, 1) -- the centre tap is inside the map at every output
    pixel of every shape here (pad <= (k - 1) / 2), so that channel of y is x's: mean 100, deviation 1, with or without the bias."""
    B, H, W, C_, k, s, p = shape
    rng = np.random.default_rng(1000 * C_ + 10 * H + k + s + p)
    if kind == 'exact':
        x = rng.integers(-16, 17, (B, H, W, C_)).astype(F32) / F32(4)
        wmax = 8 if k <= 3 else 4
        w = rng.integers(-wmax, wmax + 1, (C_, k * k)).astype(F32) / F32(4)
        b = rng.integers(-16, 17, (C_,)).astype(F32) / F32(4)
    else:
        x = rng.standard_normal((B, H, W, C_), dtype=F32)
        w = rng.standard_normal((C_, k * k), dtype=F32) * F32(1.0 / k)
        b = rng.standard_normal((C_,), dtype=F32) * F32(0.1)
        x[..., HOT] += F32(100)
        w[HOT] = 0
        w[HOT, (k * k) // 2] = 1
    for a in (x, w, b):
        a.setflags(write=False)
    return x, w, b


def _stencil(shape, xd, wd, bd):
    """ssdk_depthwise_conv2d_fwd into a pre-filled buffer."""
    B, H, W, C_, k, s, p = shape
    ho, wo = _out_hw(shape)
    y = _dev(np.full((B, ho, wo, C_), 5.0, F32))
    assert _lib.lib().ssdk_depthwise_conv2d_fwd(_p(xd), _p(wd), _p(bd), B, H, W, C_, k, s, p, _p(y), _lib.current_stream()) == OK
    return y


def _stats(shape, xd, wd, bd, sums):
    B, H, W, C_, k, s, p = shape
    ho, wo = _out_hw(shape)
    y = _dev(np.full((B, ho, wo, C_), 5.0, F32))
    assert _lib.lib().ssdk_depthwise_conv2d_stats_fwd(_p(xd), _p(wd), _p(bd), B, H, W, C_, k, s, p, _p(y), _p(sums), _lib.current_stream()) == OK
    return y


def _sums_buffer(C_, fill):
    """A `sums` buffer [2C + 2] with 4 sentinel doubles behind it (nothing may write there)."""
    buf = np.full(2 * C_ + 6, -7.0)
    buf[:2 * C_ + 2] = fill
    return _dev(buf)


@pytest.mark.parametrize('bias', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_exact_operands_sums_equal_the_fp64_sums_of_y(shape, bias):
    B, H, W, C_, k, s, p = shape
    ho, wo = _out_hw(shape)
    rows = B * ho * wo
    assert rows <= 4608
    x, w, b = _operands(shape, 'exact')
    xd, wd, bd = _dev(x), _dev(w), (_dev(b) if bias else None)
    want = _stencil(shape, xd, wd, bd)
    sums = _sums_buffer(C_, 0.0)
    y = _stats(shape, xd, wd, bd, sums)
    assert torch.equal(y, want)                                         # check 1
    yn = y.cpu().numpy().reshape(rows, C_)
    assert np.abs(yn).max() < 128 and np.array_equal(yn * 16, np.round(yn * 16))   # (the premise: multiples of 1/16 below 128)
    y64 = yn.astype(np.float64)
    s0, s1 = y64.sum(axis=0), (y64 * y64).sum(axis=0)                   # exact: every partial sum is a multiple of 2^-8 below 2^27
    got = sums.cpu().numpy()
    assert np.array_equal(got[:C_], s0), ('sum y', np.abs(got[:C_] - s0).max())
    assert np.array_equal(got[C_:2 * C_], s1), ('sum y^2', np.abs(got[C_:2 * C_] - s1).max())
    assert got[2 * C_] == rows and (got[2 * C_ + 1:] == [0.0, -7.0, -7.0, -7.0, -7.0]).all()
    y2 = _stats(shape, xd, wd, bd, sums)                                # adds to what is there: no zero-fill
    got = sums.cpu().numpy()
    assert torch.equal(y2, want)
    assert np.array_equal(got[:C_], 2 * s0) and np.array_equal(got[C_:2 * C_], 2 * s1)
    assert got[2 * C_] == rows and (got[2 * C_ + 2:] == -7.0).all()


@pytest.mark.parametrize('bias', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_normal_data_sums_within_the_fp64_bound_and_block_within_the_bar(shape, bias):
    lib, st = _lib.lib(), _lib.current_stream()
    B, H, W, C_, k, s, p = shape
    ho, wo = _out_hw(shape)
    rows = B * ho * wo
    x, w, b = _operands(shape, 'normal')
    xd, wd, bd = _dev(x), _dev(w), (_dev(b) if bias else None)
    want = _stencil(shape, xd, wd, bd)
    sums, other = _sums_buffer(C_, 0.0), _sums_buffer(C_, 3.0)
    y = _stats(shape, xd, wd, bd, sums)
    assert torch.equal(y, want)                                         # check 1
    yn = y.cpu().numpy().reshape(rows, C_)
    if rows > 1:
        hot = yn[:, HOT].astype(np.float64)
        assert abs(hot.mean()) > 30 * hot.std() or rows < 8, (hot.mean(), hot.std())   # (the conditioning case is what it claims to be)
    yl = yn.astype(np.longdouble)
    got = sums.cpu().numpy()
    for name, terms, have in (('sum y', yl, got[:C_]), ('sum y^2', yl * yl, got[C_:2 * C_])):
        err = np.abs(have.astype(np.longdouble) - terms.sum(axis=0)).astype(np.float64)
        bound = 2.0 * rows * 2.0 ** -53 * np.abs(terms).sum(axis=0).astype(np.float64)
        print(f'{name}: worst {float((err / np.maximum(bound, 1e-300)).max()):.3f} of the bound')
        assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
    assert got[2 * C_] == rows
    # the block: the norm is the apply half alone, reading the statistics the stencil's launch left
    rng = np.random.default_rng(C_ + rows)
    gamma, beta = rng.uniform(0.5, 1.5, C_).astype(F32), (rng.standard_normal(C_) * 0.1).astype(F32)
    rm, rv = (rng.standard_normal(C_) * 0.1).astype(F32), rng.uniform(0.5, 2.0, C_).astype(F32)
    rmd, rvd, nbt = _dev(rm), _dev(rv), _dev(np.array([3], np.int64))
    out, sm, sr = _dev(np.full((rows, C_), 5.0, F32)), _dev(np.zeros(C_, F32)), _dev(np.zeros(C_, F32))
    assert lib.ssdk_batchnorm_apply_chained(_p(y), rows, C_, _p(_dev(gamma)), _p(_dev(beta)), _p(rmd), _p(rvd), _p(nbt), MOMENTUM, EPS, 1, _p(out),
                                            _p(sm), _p(sr), _p(sums), _p(other), st) == OK
    ref = bnref.reference(yn, gamma, beta, rm, rv, MOMENTUM, EPS, True, 1)
    ideal = bnref.ideal_fp32(yn, gamma, beta, rm, rv, MOMENTUM, EPS, True, 1)
    bar = bnref.elementwise_bar(ideal['y'], ref['y'])
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref['y']).max(axis=0)
    print(f'block output: worst channel at {float((err / np.maximum(bar, 1e-300)).max()):.3f} of the bar (hot channel {err[HOT] / max(bar[HOT], 1e-300):.3f})')
    assert (err <= bar).all(), (int((err > bar).sum()), float((err / np.maximum(bar, 1e-300)).max()))
    assert int(nbt.cpu()[0]) == 4 and (other.cpu().numpy()[:2 * C_ + 2] == 0.0).all() and (other.cpu().numpy()[2 * C_ + 2:] == -7.0).all()


@pytest.mark.parametrize('bias', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_inference_entry_equals_stencil_then_eval_norm_bit_for_bit(shape, bias):
    lib, st = _lib.lib(), _lib.current_stream()
    B, H, W, C_, k, s, p = shape
    ho, wo = _out_hw(shape)
    rows = B * ho * wo
    x, w, b = _operands(shape, 'normal')
    xd, wd, bd = _dev(x), _dev(w), (_dev(b) if bias else None)
    mid = _stencil(shape, xd, wd, bd)
    rng = np.random.default_rng(7 * C_ + rows)
    gamma, beta = _dev(rng.uniform(0.5, 1.5, C_).astype(F32)), _dev((rng.standard_normal(C_) * 0.1).astype(F32))
    rm, rv = _dev((rng.standard_normal(C_) * 0.1).astype(F32)), _dev(rng.uniform(0.5, 2.0, C_).astype(F32))
    rm0, rv0 = rm.clone(), rv.clone()
    for relu in (0, 1):
        for ga, be in ((gamma, beta), (None, None)):
            want, sm, sr = _dev(np.full((rows, C_), 5.0, F32)), _dev(np.zeros(C_, F32)), _dev(np.zeros(C_, F32))
            assert lib.ssdk_batchnorm_fwd(_p(mid), rows, C_, _p(ga), _p(be), _p(rm), _p(rv), None, MOMENTUM, EPS, 0, relu, _p(want), _p(sm), _p(sr),
                                          None, 0, st) == OK
            got = _dev(np.full((rows, C_), 7.0, F32))
            assert lib.ssdk_depthwise_conv2d_norm_fwd(_p(xd), _p(wd), _p(bd), B, H, W, C_, k, s, p, _p(ga), _p(be), _p(rm), _p(rv), EPS, relu, _p(got),
                                                      st) == OK
            assert torch.equal(got, want), (relu, ga is None, float((got - want).abs().max()))
            if relu:
                assert float(got.min()) == 0.0 or rows < 4
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)   # the running statistics are read, never written
