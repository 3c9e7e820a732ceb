"""The column-slab grid of bn_reduce_kernel (csrc/norm.hip, bn_reduce_plan): a workgroup owns a slab of float4 columns of its rows, and
a wave instruction takes 64 / slab consecutive rows.  Against the float64 model of tests/batchnorm_reference.py, as
test_batchnorm_kernels_gpu.py uses it.

Integer-valued operands make every partial sum exact in any order -- fp64 in the forward statistics, fp32 in the backward ones -- so the
`sums` of ssdk_batchnorm_stats, _stats_accumulate and _bwd_stats (ReLU mask on and off) must EQUAL numpy's, no tolerance, for

  channels  4 (one partial slab), 64 (exactly one slab), 68 (one slab plus one column), 128, 256, 512 (2, 4 and 8 slabs),
            132, 260, 896 (C / 4 = 33, 65, 224: the last slab is narrower or a single column);
  rows      1, 3, 63, 64, 65, 257, 1000, and 5000 -- above the 4096 rows a workgroup takes at the most -- plus one map of 525 000 rows on
            which the default rule itself picks those 4096;
  knobs     one case at every slab width SSDK_BN_SLAB accepts (0 = whole rows per workgroup, the form before) and at SSDK_BN_ROWS 16, 256.

The large-mean conditioning case (|mean| / std = 3000) goes through ssdk_batchnorm_fwd at the 4-ulp bars of test_batchnorm_kernels_gpu.py for
save_mean, save_rstd and running_var: fp64 accumulation from the first add is what the slab form must keep."""
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

CHANNELS = [4, 64, 68, 128, 132, 256, 260, 512, 896]
ROWS = [1, 3, 63, 64, 65, 257, 1000, 5000]

_alive = []


@pytest.fixture(autouse=True)
def _device_buffers_live_until_the_test_ends():
    """The library is handed raw pointers: everything _dev makes stays alive until the test is over."""
    yield
    del _alive[:]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()
    _alive.append(t)
    return t


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _sums_buffer(C_, fill):
    """A `sums` buffer [2C + 2] with 4 sentinel doubles behind it (nothing may write there)."""
    buf = np.full(2 * C_ + 6, -7.0)
    buf[:2 * C_ + 2] = fill
    return _dev(buf)


def _tail_untouched(buf, C_):
    return bool((buf[2 * C_ + 2:] == -7.0).all())


@functools.lru_cache(maxsize=8)
def _int_pattern(rows, C_, lo, hi, salt):
    """Integer values in [lo, hi], a different sequence in every row and channel (a swapped, dropped or doubled row or column changes a
    sum), no row entirely zero.  Read-only: the few most recent ones are shared between the checks that ask for them again."""
    r = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(C_, dtype=np.int64)[None, :]
    v = (r * (c % 5 + 1) + c * c + r // 3 + (r * r) // 7 * (c % 3) + salt) % (hi - lo + 1) + lo
    v[:, 0] = np.where((v != 0).any(axis=1), v[:, 0], hi)
    v.setflags(write=False)
    return v


def _check_forward_sums(C_, rows):
    lib, st = _lib.lib(), _lib.current_stream()
    xi = _int_pattern(rows, C_, -3, 3, 0)
    sums = _sums_buffer(C_, np.nan)   # ssdk_batchnorm_stats overwrites whatever is there
    assert lib.ssdk_batchnorm_stats(_p(_dev(xi, F32)), rows, C_, _p(sums), st) == OK
    got = sums.cpu().numpy()
    assert np.array_equal(got[:C_], xi.sum(axis=0)), ('sum x', C_, rows)
    assert np.array_equal(got[C_:2 * C_], (xi * xi).sum(axis=0)), ('sum x^2', C_, rows)
    assert got[2 * C_] == rows and _tail_untouched(got, C_)


def _check_accumulate(C_, rows_a, rows_b):
    lib, st = _lib.lib(), _lib.current_stream()
    xa, xb = _int_pattern(rows_a, C_, -3, 3, 1), _int_pattern(rows_b, C_, -3, 3, 4)
    sums = _sums_buffer(C_, 0.0)
    assert lib.ssdk_batchnorm_stats_accumulate(_p(_dev(xa, F32)), rows_a, C_, _p(sums), st) == OK
    assert lib.ssdk_batchnorm_stats_accumulate(_p(_dev(xb, F32)), rows_b, C_, _p(sums), st) == OK
    got = sums.cpu().numpy()
    assert np.array_equal(got[:C_], xa.sum(axis=0) + xb.sum(axis=0)), ('accumulated sum x', C_, rows_a, rows_b)
    assert np.array_equal(got[C_:2 * C_], (xa * xa).sum(axis=0) + (xb * xb).sum(axis=0)), ('accumulated sum x^2', C_, rows_a, rows_b)
    assert got[2 * C_] == rows_b and _tail_untouched(got, C_)   # (slot 2C: the rows of the call, as ssdk.h documents it)


def _check_backward_sums(C_, rows, relu):
    """save_mean integer, save_rstd 1/4, 1/2 or 1, dy in -2 .. 2: dy' * xhat is a multiple of 1/4 of at most 10, and a workgroup's fp32 sum
    over its at most 4096 rows stays far below 2^24 quarters: every partial sum is exact (across workgroups the sums are fp64)."""
    lib, st = _lib.lib(), _lib.current_stream()
    xi = _int_pattern(rows, C_, -3, 3, 2)
    gi = _int_pattern(rows, C_, -2, 2, 5)
    mean = (np.arange(C_) % 5 - 2).astype(np.float64)
    rstd = 2.0 ** (np.arange(C_) % 3 - 2)
    y = _int_pattern(rows, C_, -3, 3, 9).astype(F32)
    if relu:   # y > 0 decides: 0.0 and -0.0 are not positive, a denormal is
        flat = y.reshape(-1)
        for k, v in enumerate([0.0, -0.0, 1e-40, -1e-40, 0.0, -0.0, 1e-45]):
            flat[(k * 37 + k) % flat.size] = F32(v)
    g = gi * (y > 0) if relu else gi
    want0 = g.sum(axis=0).astype(np.float64)
    want1 = (g * ((xi - mean) * rstd)).sum(axis=0)
    sums = _sums_buffer(C_, np.nan)
    assert lib.ssdk_batchnorm_bwd_stats(_p(_dev(xi, F32)), _p(_dev(y)) if relu else None, _p(_dev(gi, F32)), rows, C_, _p(_dev(mean, F32)),
                                        _p(_dev(rstd, F32)), relu, _p(sums), st) == OK
    got = sums.cpu().numpy()
    assert np.array_equal(got[:C_], want0), ('sum dy', C_, rows, relu)
    assert np.array_equal(got[C_:2 * C_], want1), ('sum dy xhat', C_, rows, relu)
    assert got[2 * C_] == rows and _tail_untouched(got, C_)


def _plan(rows, C_):
    out = (C.c_longlong * 4)()
    assert _lib.lib().ssdk_debug_batchnorm_plan(rows, C_, out) == OK
    return dict(rows_per_block=out[0], row_blocks=out[1], slab=out[2], slabs=out[3])


def test_the_channel_counts_exercise_every_slab_layout():
    """What the case list claims, asked of the library (host only): slab width 16 by default, so 1 partial slab ... 56 slabs."""
    got = {C_: (_plan(1000, C_)['slab'], _plan(1000, C_)['slabs']) for C_ in CHANNELS}
    assert got == {4: (1, 1), 64: (16, 1), 68: (16, 2), 128: (16, 2), 132: (16, 3), 256: (16, 4), 260: (16, 5), 512: (16, 8), 896: (16, 14)}
    assert _plan(5000, 256)['row_blocks'] == 40 and _plan(525000, 4) == dict(rows_per_block=4096, row_blocks=129, slab=1, slabs=1)


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('C_', CHANNELS)
def test_forward_sums_are_exact(C_, rows):
    _check_forward_sums(C_, rows)
    _check_accumulate(C_, rows, 65)


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('C_', CHANNELS)
def test_backward_sums_are_exact(C_, rows):
    _check_backward_sums(C_, rows, 0)
    _check_backward_sums(C_, rows, 1)


@pytest.mark.parametrize('C_', [4, 20])
def test_sums_are_exact_at_the_largest_rows_per_workgroup_the_host_picks(C_):
    """525 000 rows: rows / 128 is above the cap, every workgroup takes 4096 rows (the last one 712)."""
    rows = 525000
    assert _plan(rows, C_)['rows_per_block'] == 4096
    _check_forward_sums(C_, rows)
    _check_backward_sums(C_, rows, 1)


@pytest.mark.parametrize('knob,value', [('SSDK_BN_SLAB', v) for v in (0, 1, 2, 4, 8, 16, 32, 64)] + [('SSDK_BN_ROWS', 16), ('SSDK_BN_ROWS', 256)])
@pytest.mark.parametrize('C_', [132, 260])
def test_sums_are_exact_at_every_slab_width_and_rows_setting(C_, knob, value, monkeypatch):
    """The library reads SSDK_BN_SLAB per call, as it reads SSDK_BN_ROWS: whole rows (0), every power-of-two width, and the default width
    at 16 and 256 rows per workgroup (one and four trips of a wave over its rows)."""
    monkeypatch.setenv(knob, str(value))
    plan = _plan(1000, C_)
    if knob == 'SSDK_BN_SLAB':
        assert (plan['slab'], plan['slabs']) == ((64, 1) if value == 0 else (value, -(-(C_ // 4) // value)))
    else:
        assert plan['rows_per_block'] == value and plan['slab'] == 16
    _check_forward_sums(C_, 1000)
    _check_backward_sums(C_, 1000, 1)
    _check_accumulate(C_, 1000, 257)


@pytest.mark.parametrize('rows,C_', [(1000, 260), (257, 512), (5000, 132)])
def test_large_means_keep_their_variance(rows, C_):
    """Every channel's |mean| / std = 3000 (either sign, std 0.5, 1 or 2) through ssdk_batchnorm_fwd: save_mean, save_rstd and running_var
    within 4 fp32 ulp of the float64 statistics (the bars of test_batchnorm_kernels_gpu.py).  With fp32 partial sums anywhere in the slab
    form the variance of such a channel is lost entirely."""
    lib, st = _lib.lib(), _lib.current_stream()
    rng = np.random.default_rng(1000 * C_ + rows)
    c = np.arange(C_)
    sigma = np.array([0.5, 1.0, 2.0])[c % 3]
    mu = (3000.0 * sigma * np.where(c % 2 == 1, -1.0, 1.0)).astype(F32)
    x = (rng.standard_normal((rows, C_)) * sigma).astype(F32) + mu
    gamma, beta = rng.uniform(0.5, 1.5, C_).astype(F32), rng.standard_normal(C_).astype(F32)
    mean, _ = bnref.statistics(x)
    rm0, rv0 = (mean * rng.uniform(0.5, 1.5, C_)).astype(F32), rng.uniform(0.5, 2.0, C_).astype(F32)
    ref = bnref.reference(x, gamma, beta, rm0, rv0, MOMENTUM, EPS, True, 0)
    d = dict(y=torch.empty((rows, C_), device='cuda'), mean=torch.empty(C_, device='cuda'), rstd=torch.empty(C_, device='cuda'), rm=_dev(rm0), rv=_dev(rv0))
    n = lib.ssdk_batchnorm_workspace_bytes(C_)
    ws = torch.empty((n,), dtype=torch.uint8, device='cuda')
    assert lib.ssdk_batchnorm_fwd(_p(_dev(x)), rows, C_, _p(_dev(gamma)), _p(_dev(beta)), _p(d['rm']), _p(d['rv']), None, MOMENTUM, EPS, 1, 0,
                                  _p(d['y']), _p(d['mean']), _p(d['rstd']), _p(ws), n, st) == OK
    figures = {k: float(bnref.ulps_fp32(d[a].cpu().numpy(), ref[k]).max())
               for k, a in (('save_mean', 'mean'), ('save_rstd', 'rstd'), ('running_var', 'rv'), ('running_mean', 'rm'))}
    print(f'[{rows}x{C_}] ulp: {figures}')
    assert all(v <= 4.0 for v in figures.values()), figures
