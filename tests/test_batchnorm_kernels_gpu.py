"""The BatchNorm family of csrc/norm.hip, entry point by entry point through the C ABI, against the float64 model of
tests/batchnorm_reference.py (pinned against torch.nn.BatchNorm2d in float64 by test_batchnorm_reference.py).

(a) the reductions, EXACTLY: integer-valued inputs make every partial sum exact in any order, so the fp64 `sums` must equal numpy's
    int64 sums -- no tolerance; every layout branch of bn_reduce_kernel and every rows-per-workgroup rule.
(b) the elementwise kernels, given exact sums: both constant paths of the apply kernels, the argument combinations the blocks never
    produce, ssdk_relu_bwd.
(c) the composed entry points, plain and chained.
(d) conditioning: channels whose mean is up to 3000 standard deviations.
(e) refusals: the documented return codes, and nothing launched.
(f) nearest-neighbour index arithmetic of ssdk_upsample_nearest_add_fwd / _bwd for every size pair up to 24.

Bars (all from the reference and the number format, none from the library): save_mean / save_rstd / running statistics within 4 fp32
ulp of the float64 value; y and dx within 4 x |ideal_fp32 - reference| (per channel) + 4 x 2^-24 x max|reference| of the channel, where
ideal_fp32 is the exact statistics rounded once and the elementwise chain in float32; dgamma / dbeta from given sums: float32(sum),
exactly.  The backward is handed save_mean / save_rstd as float32 by the ABI, so its ideal forms xhat from those rounded values in the
backward sums as well (with sums over the float64 mean instead, dx of a channel whose mean is 3000 standard deviations misses by
(mean64 - mean32) * rstd * mean(dy) * xhat: 6.9e-5 against a bar of 2.0e-6 at 64 rows -- DESIGN.md section 13)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import batchnorm_reference as bnref
from single_shot_detection_amd import _lib

pytestmark = pytest.mark.gpu

OK, E_INVALID, E_WORKSPACE, E_UNSUPPORTED = 0, -1, -2, -3   # include/ssdk.h
F32 = np.float32
MOMENTUM, EPS = float(F32(0.1)), float(F32(1e-5))


_alive = []


@pytest.fixture(autouse=True)
def _device_buffers_live_until_the_test_ends():
    """The library is handed raw pointers: a tensor made inside an argument list would be freed -- and its block handed to the next
    argument -- before the call.  Everything _dev makes stays alive until the test is over."""
    yield
    del _alive[:]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()
    _alive.append(t)
    return t


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _np(t):
    return t.cpu().numpy()


def _ws(C_):
    n = _lib.lib().ssdk_batchnorm_workspace_bytes(C_)
    return torch.empty((n,), dtype=torch.uint8, device='cuda'), n


def _sums_buffer(C_, *parts, fill=None):
    """A `sums` buffer [2C + 2] with 4 sentinel doubles behind it (nothing may write there)."""
    buf = np.full(2 * C_ + 6, -7.0)
    if fill is not None:
        buf[:2 * C_ + 2] = fill
    if parts:
        s0, s1, n = parts
        buf[:C_], buf[C_:2 * C_], buf[2 * C_], buf[2 * C_ + 1] = s0, s1, n, 0.0
    return _dev(buf)


def _tail_untouched(buf, C_):
    return bool((buf[2 * C_ + 2:] == -7.0).all())


# ---- (a) the reductions, exactly ------------------------------------------------------------------------------------------------------

def _int_pattern(rows, C_, lo, hi, salt):
    """Integer values in [lo, hi], a different sequence in every row and channel (a swapped, dropped or doubled row or column changes a
    sum), no row entirely zero."""
    r = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(C_, dtype=np.int64)[None, :]
    v = (r * (c % 5 + 1) + c * c + r // 3 + (r * r) // 7 * (c % 3) + salt) % (hi - lo + 1) + lo
    v[:, 0] = np.where((v != 0).any(axis=1), v[:, 0], hi)
    return v


PACKED = [4, 8, 32, 128]
UNPACKED = [12, 48, 132, 256]
TRIPS = [260, 640, 896]
ROWS = [1, 2, 3, 63, 64, 65, 127, 257, 1000]


def _check_forward_sums(C_, rows, salt=0):
    lib, st = _lib.lib(), _lib.current_stream()
    xi = _int_pattern(rows, C_, -3, 3, salt)
    x = _dev(xi, F32)
    sums = _sums_buffer(C_, fill=np.nan)   # ssdk_batchnorm_stats overwrites whatever is there
    assert lib.ssdk_batchnorm_stats(_p(x), rows, C_, _p(sums), st) == OK
    got = _np(sums)
    assert np.array_equal(got[:C_], xi.sum(axis=0)), ('sum x', C_, rows)
    assert np.array_equal(got[C_:2 * C_], (xi * xi).sum(axis=0)), ('sum x^2', C_, rows)
    assert got[2 * C_] == rows and _tail_untouched(got, C_)
    return xi, x


def _check_accumulate(C_, rows_a, rows_b):
    lib, st = _lib.lib(), _lib.current_stream()
    xa, xb = _int_pattern(rows_a, C_, -3, 3, 1), _int_pattern(rows_b, C_, -3, 3, 4)
    sums = _sums_buffer(C_, fill=0.0)
    assert lib.ssdk_batchnorm_stats_accumulate(_p(_dev(xa, F32)), rows_a, C_, _p(sums), st) == OK
    assert lib.ssdk_batchnorm_stats_accumulate(_p(_dev(xb, F32)), rows_b, C_, _p(sums), st) == OK
    got = _np(sums)
    assert np.array_equal(got[:C_], xa.sum(axis=0) + xb.sum(axis=0)), ('accumulated sum x', C_, rows_a, rows_b)
    assert np.array_equal(got[C_:2 * C_], (xa * xa).sum(axis=0) + (xb * xb).sum(axis=0)), ('accumulated sum x^2', C_, rows_a, rows_b)
    assert got[2 * C_] == rows_b and _tail_untouched(got, C_)   # (slot 2C: the rows of the call, as ssdk.h documents it)


def _check_backward_sums(C_, rows, relu):
    """save_mean integer, save_rstd a power of two, dy in -2 .. 2: dy' * xhat is a multiple of 1/4 below 2^6, every sum exact."""
    lib, st = _lib.lib(), _lib.current_stream()
    xi = _int_pattern(rows, C_, -3, 3, 2)
    gi = _int_pattern(rows, C_, -2, 2, 5)
    mean = (np.arange(C_) % 5 - 2).astype(np.float64)
    rstd = 2.0 ** (np.arange(C_) % 5 - 2)
    y = _int_pattern(rows, C_, -3, 3, 9).astype(F32)
    if relu:   # y > 0 decides: 0.0 and -0.0 are not positive, a denormal is
        flat = y.reshape(-1)
        for k, v in enumerate([0.0, -0.0, 1e-40, -1e-40, 0.0, -0.0, 1e-45]):
            flat[(k * 37 + k) % flat.size] = F32(v)
        assert (flat[(flat != 0) & (np.abs(flat) < 1e-38)] != 0).any()
    g = gi * (y > 0) if relu else gi
    want0 = g.sum(axis=0).astype(np.float64)
    want1 = (g * ((xi - mean) * rstd)).sum(axis=0)
    sums = _sums_buffer(C_, fill=np.nan)
    assert lib.ssdk_batchnorm_bwd_stats(_p(_dev(xi, F32)), _p(_dev(y)) if relu else None, _p(_dev(gi, F32)), rows, C_, _p(_dev(mean, F32)),
                                        _p(_dev(rstd, F32)), relu, _p(sums), st) == OK
    got = _np(sums)
    assert np.array_equal(got[:C_], want0), ('sum dy', C_, rows, relu)
    assert np.array_equal(got[C_:2 * C_], want1), ('sum dy xhat', C_, rows, relu)
    assert got[2 * C_] == rows and _tail_untouched(got, C_)


@pytest.mark.parametrize('C_', PACKED + UNPACKED + TRIPS)
def test_forward_sums_are_exact_in_every_layout(C_):
    for rows in ROWS:
        _check_forward_sums(C_, rows)
    _check_accumulate(C_, 65, 127)
    _check_accumulate(C_, 1000, 3)


@pytest.mark.parametrize('C_', PACKED + UNPACKED + TRIPS)
def test_backward_sums_are_exact_in_every_layout(C_):
    for rows in ROWS:
        _check_backward_sums(C_, rows, 0)
        _check_backward_sums(C_, rows, 1)


@pytest.mark.parametrize('rows', [8193, 20000])
@pytest.mark.parametrize('C_', [8, 128, 12, 132, 260])
def test_sums_are_exact_with_more_than_64_rows_per_workgroup(C_, rows):
    """rows / 128 rounded up to 16 exceeds 64 here: 80 rows per workgroup (and a partial last one) and 160."""
    assert (-(-rows // 128) + 15) // 16 * 16 == {8193: 80, 20000: 160}[rows]
    _check_forward_sums(C_, rows)
    _check_backward_sums(C_, rows, 1)


@pytest.mark.parametrize('knob,value', [('SSDK_BN_ROWS', 16), ('SSDK_BN_ROWS', 80), ('SSDK_BN_ROWS', 4096), ('SSDK_BN_WGS', 1), ('SSDK_BN_WGS', 7)])
@pytest.mark.parametrize('C_', [4, 32, 12, 260])
def test_sums_are_exact_at_every_rows_per_workgroup_setting(C_, knob, value, monkeypatch):
    """The library reads SSDK_BN_ROWS / SSDK_BN_WGS per call: 16 rows (below the default floor), 80, the 4096 cap reached directly and
    through one requested workgroup, and 720 rows through seven."""
    monkeypatch.setenv(knob, str(value))
    _check_forward_sums(C_, 5000)
    _check_backward_sums(C_, 5000, 1)
    _check_accumulate(C_, 5000, 257)


# ---- (b) the elementwise kernels, given exact sums ------------------------------------------------------------------------------------

def _apply_blocks(n4, C4):
    """The documented grid rule of the apply kernels (csrc/norm.hip apply_blocks), in plain Python."""
    b = min(max(-(-n4 // 256), 1), 4096)
    m = C4 // math.gcd(C4, 256)
    return b // m * m if b >= m else b


def _constant_path(rows, C_):
    """('fixed' | 'per_float4', grid-stride trips): constants once per thread exactly when 256 * grid is a multiple of C / 4."""
    n4, C4 = rows * C_ // 4, C_ // 4
    blocks = _apply_blocks(n4, C4)
    return ('fixed' if (256 * blocks) % C4 == 0 else 'per_float4'), -(-n4 // (256 * blocks)), blocks


def _data(rows, C_, seed, relu_input=False):
    """x = mu_c + sigma_c * n, |mu_c| in 0.5 .. 2 with either sign, a few exact zeros (+0.0 and -0.0) planted."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.5, 2.0, C_) * np.where(np.arange(C_) % 3 == 0, -1.0, 1.0)
    sigma = rng.uniform(0.5, 2.0, C_)
    x = (rng.standard_normal((rows, C_)) * sigma + mu).astype(F32)
    if relu_input:
        x = np.maximum(x, F32(0))
    flat = x.reshape(-1)
    for k in range(6):
        flat[(k * 41 + 3) % flat.size] = F32(-0.0 if k % 2 else 0.0)
    gamma = (rng.uniform(0.5, 1.5, C_) * np.where(np.arange(C_) % 4 == 1, -1.0, 1.0)).astype(F32)
    beta = rng.standard_normal(C_).astype(F32)
    dy = rng.standard_normal((rows, C_)).astype(F32)
    return rng, x, gamma, beta, dy


def _running(rng, x, stats_of=None):
    """Old running statistics with the sign of the batch mean: (1 - momentum) * old + momentum * new is then free of cancellation and
    its fp32 evaluation can be held to a few ulp OF THE RESULT (the bar is meaningless for a result that is a difference)."""
    mean, _ = bnref.statistics(x if stats_of is None else stats_of)
    return (mean * rng.uniform(0.5, 1.5, mean.shape)).astype(F32), rng.uniform(0.5, 2.0, mean.shape).astype(F32)


def _assert_elementwise(got, ideal, ref, what, info=None):
    bar = bnref.elementwise_bar(ideal, ref)
    err = np.abs(np.asarray(got, np.float64) - ref).max(axis=0)
    worst = int(np.argmax(np.divide(err, bar, out=np.zeros_like(err), where=bar > 0)))
    if info is not None:
        info[what] = (err, bar)
    assert (err <= bar).all(), (what, 'channel', worst, 'error', float(err[worst]), 'bar', float(bar[worst]))


def _assert_ulps(got, want64, what, limit=4.0):
    u = bnref.ulps_fp32(got, want64)
    assert (u <= limit).all(), (what, 'channel', int(np.argmax(u)), 'ulps', float(u.max()))


def _run_apply(rows, C_, seed=0, relu=0, gamma_null=False, beta_null=False, running=True, nbt=True, momentum=MOMENTUM, eps=EPS,
               double_count=False, chained=False):
    """ssdk_batchnorm_apply (or _apply_chained) on the float64 sums of the reference."""
    lib, st = _lib.lib(), _lib.current_stream()
    rng, x, gamma, beta, _ = _data(rows, C_, seed)
    gamma, beta = (None if gamma_null else gamma), (None if beta_null else beta)
    stats_of = np.concatenate([x, (x[::-1] * F32(1.5) + F32(0.25)).astype(F32)]) if double_count else None
    rm0, rv0 = _running(rng, x, stats_of)
    args = (x, gamma, beta, rm0, rv0, momentum, eps, True, relu, None, stats_of)
    ref, ideal = bnref.reference(*args), bnref.ideal_fp32(*args)
    sums = _sums_buffer(C_, ref['sum_x'], ref['sum_x2'], ref['count'])
    d = dict(x=_dev(x), y=torch.full((rows, C_), 77.0, device='cuda'), mean=torch.empty(C_, device='cuda'), rstd=torch.empty(C_, device='cuda'),
             rm=_dev(rm0) if running else None, rv=_dev(rv0) if running else None,
             nbt=torch.tensor([2 ** 32 + 5], dtype=torch.int64, device='cuda') if nbt else None,
             g=None if gamma is None else _dev(gamma), b=None if beta is None else _dev(beta))
    head = (_p(d['x']), rows, C_, _p(d['g']), _p(d['b']), _p(d['rm']), _p(d['rv']), _p(d['nbt']), momentum, eps, relu, _p(d['y']), _p(d['mean']), _p(d['rstd']))
    if chained:
        partner = _sums_buffer(C_, fill=np.nan)
        assert lib.ssdk_batchnorm_apply_chained(*head, _p(sums), _p(partner), st) == OK
        got = _np(partner)
        assert (got[:2 * C_ + 2] == 0.0).all() and _tail_untouched(got, C_)
    else:
        assert lib.ssdk_batchnorm_apply(*head, _p(sums), 1 if double_count else 0, st) == OK
    _assert_ulps(_np(d['mean']), ref['save_mean'], 'save_mean')
    _assert_ulps(_np(d['rstd']), ref['save_rstd'], 'save_rstd')
    if running:
        _assert_ulps(_np(d['rm']), ref['running_mean'], 'running_mean')
        _assert_ulps(_np(d['rv']), ref['running_var'], 'running_var')
    if nbt:
        assert d['nbt'].dtype == torch.int64 and int(d['nbt']) == 2 ** 32 + 6
    _assert_elementwise(_np(d['y']), ideal['y'], ref['y'], 'y')
    if relu:
        assert (_np(d['y']) >= 0).all() and (ref['y'] == 0).any()
    return ref


def _run_bwd_apply(rows, C_, seed=0, relu=0, training=1, gamma_null=False, dgamma_null=False, dbeta_null=False, split_sums=False, check_rows=None):
    """ssdk_batchnorm_bwd_apply on the float64 backward sums of the reference.  y (read for its sign only) is the reference's output
    with exact zeros, -0.0 and denormals planted."""
    lib, st = _lib.lib(), _lib.current_stream()
    rng, x, gamma, beta, dy = _data(rows, C_, seed, relu_input=bool(relu & 2))
    gamma = None if gamma_null else gamma
    mean, var = bnref.statistics(x)
    mean, rstd = mean.astype(F32), (1.0 / np.sqrt(var + EPS)).astype(F32)     # what the forward saved: fp32 values, given
    y = None
    if relu & 1:
        y = bnref.reference(x, gamma, beta, None, None, MOMENTUM, EPS, True, 1)['y'].astype(F32)
        flat = y.reshape(-1)
        for k, v in enumerate([0.0, -0.0, 1e-40, -1e-40, 1e-45, -0.0]):
            flat[(k * 29 + 1) % flat.size] = F32(v)
    glob = None
    local = bnref.backward(x, y, dy, gamma, mean, rstd, relu, training)
    sums_local = None
    if split_sums:   # dx from the sums of twice the rows (all ranks'), dgamma / dbeta from this call's own
        x2, dy2 = np.concatenate([x, x[::-1]]), np.concatenate([dy, (dy[::-1] * F32(0.5)).astype(F32)])
        y2 = None if y is None else np.concatenate([y, y[::-1]])
        both = bnref.backward(x2, y2, dy2, gamma, mean, rstd, relu, training)
        glob = (both['sums_dy'], both['sums_dy_xhat'], float(2 * rows))
        sums_local = _sums_buffer(C_, local['sums_dy'], local['sums_dy_xhat'], rows)
    ref = bnref.backward(x, y, dy, gamma, mean, rstd, relu, training, glob)
    ideal = bnref.ideal_fp32_backward(x, y, dy, gamma, mean, rstd, relu, training, glob)
    sums = _sums_buffer(C_, *(glob if glob else (ref['sums_dy'], ref['sums_dy_xhat'], rows)))
    dx = torch.full((rows, C_), 77.0, device='cuda')
    dgamma, dbeta = torch.full((C_,), 55.0, device='cuda'), torch.full((C_,), 55.0, device='cuda')
    total_rows = C.c_void_p(sums.data_ptr() + 16 * C_) if split_sums else None
    assert lib.ssdk_batchnorm_bwd_apply(_p(_dev(x)), None if y is None else _p(_dev(y)), _p(_dev(dy)), rows, C_, None if gamma is None else _p(_dev(gamma)),
                                        _p(_dev(mean)), _p(_dev(rstd)), relu, training, _p(sums), _p(sums_local), total_rows, _p(dx),
                                        None if dgamma_null else _p(dgamma), None if dbeta_null else _p(dbeta), st) == OK
    _assert_elementwise(_np(dx), ideal['dx'], ref['dx'], 'dx')
    if relu & 2:
        assert (_np(dx)[~(x > 0)] == 0).all() and (~(x > 0)).any()
    want_g, want_b = local['sums_dy_xhat'].astype(F32), local['sums_dy'].astype(F32)
    assert np.array_equal(_np(dgamma), np.full(C_, 55.0, F32) if dgamma_null else want_g)
    assert np.array_equal(_np(dbeta), np.full(C_, 55.0, F32) if dbeta_null else want_b)


PER_FLOAT4 = [(5, 12), (100, 132), (6, 896), (3, 260)]
ROUNDED_DOWN = [(1100, 12), (300, 132), (70, 896)]
POWERS_OF_TWO = [(64, 4), (257, 128), (33, 512)]


@pytest.mark.parametrize('rows,C_', PER_FLOAT4)
def test_apply_kernels_with_constants_per_float4(rows, C_):
    """A grid smaller than C4 / gcd(C4, 256) cannot be rounded to a stride that keeps a thread on its channels: the constants are
    worked out for every float4 from the channel index i % C4."""
    assert _constant_path(rows, C_)[0] == 'per_float4'
    _run_apply(rows, C_)
    _run_bwd_apply(rows, C_)


@pytest.mark.parametrize('rows,C_', ROUNDED_DOWN)
def test_apply_kernels_with_the_grid_rounded_down(rows, C_):
    path, trips, blocks = _constant_path(rows, C_)
    assert path == 'fixed' and trips > 1 and blocks < -(-rows * C_ // 4 // 256)
    _run_apply(rows, C_)
    _run_bwd_apply(rows, C_)


@pytest.mark.parametrize('rows,C_', POWERS_OF_TWO + [(7, 896)])
def test_apply_kernels_with_constants_once_per_thread(rows, C_):
    """Powers of two; and 7 x 896, whose 7 blocks are exactly C4 / gcd(C4, 256): the smallest grid that is NOT on the per-float4 path
    (6 x 896, one block fewer, is -- above)."""
    assert _constant_path(rows, C_)[0] == 'fixed'
    _run_apply(rows, C_)
    _run_bwd_apply(rows, C_)


def test_bwd_apply_past_the_block_cap():
    """400000 x 12: 4688 blocks wanted, capped to 4096 and rounded down to 4095 (C4 = 3); two grid-stride trips."""
    rows, C_ = 400000, 12
    path, trips, blocks = _constant_path(rows, C_)
    assert (path, trips, blocks) == ('fixed', 2, 4095)
    _run_bwd_apply(rows, C_)


ARGUMENTS = {
    'fwd_relu': ('f', dict(relu=1)),
    'fwd_no_gamma': ('f', dict(gamma_null=True)),
    'fwd_no_beta': ('f', dict(beta_null=True)),
    'fwd_no_affine_relu': ('f', dict(gamma_null=True, beta_null=True, relu=1)),
    'fwd_no_running_statistics': ('f', dict(running=False)),
    'fwd_no_num_batches_tracked': ('f', dict(nbt=False)),
    'fwd_momentum_1': ('f', dict(momentum=1.0)),
    'fwd_momentum_0.01': ('f', dict(momentum=float(F32(0.01)))),
    'fwd_eps_1e-3': ('f', dict(eps=float(F32(1e-3)))),
    'fwd_count_in_sums': ('f', dict(double_count=True)),
    'fwd_chained': ('f', dict(chained=True, relu=1)),
    'bwd_relu_1': ('b', dict(relu=1)),
    'bwd_relu_2': ('b', dict(relu=2)),
    'bwd_relu_3': ('b', dict(relu=3)),
    'bwd_eval': ('b', dict(training=0)),
    'bwd_eval_relu_3': ('b', dict(training=0, relu=3)),
    'bwd_no_gamma': ('b', dict(gamma_null=True, relu=1)),
    'bwd_no_dgamma': ('b', dict(dgamma_null=True)),
    'bwd_no_dbeta': ('b', dict(dbeta_null=True)),
    'bwd_no_dgamma_no_dbeta': ('b', dict(dgamma_null=True, dbeta_null=True, relu=2)),
    'bwd_global_and_local_sums': ('b', dict(split_sums=True)),
    'bwd_global_and_local_sums_relu_3': ('b', dict(split_sums=True, relu=3)),
}


@pytest.mark.parametrize('name', sorted(ARGUMENTS))
@pytest.mark.parametrize('rows,C_', [(37, 32), (37, 20), (300, 132)], ids=['packed32', 'unpacked20', 'unpacked132'])
def test_apply_kernels_argument_matrix(rows, C_, name):
    kind, kw = ARGUMENTS[name]
    (_run_apply if kind == 'f' else _run_bwd_apply)(rows, C_, seed=11, **kw)


@pytest.mark.parametrize('C_', [32, 20])
def test_one_row_in_training_mode(C_):
    """rows == 1 (torch refuses it): the kernel defines variance 0, the unbiasing factor 1, y = beta, dx = 0."""
    ref = _run_apply(1, C_, seed=2)
    assert (ref['batch_var_unbiased'] == 0).all() and np.allclose(ref['save_rstd'], 1.0 / math.sqrt(EPS))
    _run_bwd_apply(1, C_, seed=2)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('rows,C_', [(37, 32), (37, 20), (300, 132), (33, 512)])
def test_eval_forward(rows, C_, relu):
    """ssdk_batchnorm_fwd, training == 0: the running statistics normalise and are left alone, save_mean / save_rstd are published for a
    backward through the frozen norm, num_batches_tracked does not count."""
    lib, st = _lib.lib(), _lib.current_stream()
    rng, x, gamma, beta, _ = _data(rows, C_, 23)
    rm0, rv0 = _running(rng, x)
    args = (x, gamma, beta, rm0, rv0, MOMENTUM, EPS, False, relu)
    ref, ideal = bnref.reference(*args), bnref.ideal_fp32(*args)
    y, mean, rstd = torch.full((rows, C_), 77.0, device='cuda'), torch.empty(C_, device='cuda'), torch.empty(C_, device='cuda')
    rm, rv = _dev(rm0), _dev(rv0)
    nbt = torch.tensor([2 ** 32 + 5], dtype=torch.int64, device='cuda')
    assert lib.ssdk_batchnorm_fwd(_p(_dev(x)), rows, C_, _p(_dev(gamma)), _p(_dev(beta)), _p(rm), _p(rv), _p(nbt), MOMENTUM, EPS, 0, relu, _p(y), _p(mean),
                                  _p(rstd), None, 0, st) == OK
    assert np.array_equal(_np(mean), rm0) and np.array_equal(_np(rm), rm0) and np.array_equal(_np(rv), rv0) and int(nbt) == 2 ** 32 + 5
    _assert_ulps(_np(rstd), ref['save_rstd'], 'save_rstd')
    _assert_elementwise(_np(y), ideal['y'], ref['y'], 'y')


@pytest.mark.parametrize('n', [4, 1020, 1024 * 4096 * 4 + 4])
def test_relu_bwd_is_exact(n):
    """dx = dy where y > 0, else 0, bit for bit; the largest n is one float4 past four full trips of the capped grid."""
    pat_y = np.array([1.0, 0.0, -0.0, np.nan, -1.5, 1e-40, -1e-40, 3.0, np.inf, -np.inf, 2.0], F32)
    pat_g = np.array([1.5, -2.0, 3.0, -0.0, 0.25, 7.0, -7.0], F32)
    y, dy = np.resize(pat_y, n), np.resize(pat_g, n)
    dx = torch.full((n,), 9.0, device='cuda')
    assert _lib.lib().ssdk_relu_bwd(_p(_dev(y)), _p(_dev(dy)), n, _p(dx), _lib.current_stream()) == OK
    want = np.where(y > 0, dy, F32(0))
    assert np.array_equal(_np(dx).view(np.uint32), want.view(np.uint32))


# ---- (c) the composed entry points ------------------------------------------------------------------------------------------------------

# The backward sums of the composed entry points are accumulated by the library in fp32 per thread (the longest chain of adds a value
# passes through: rows per thread of a workgroup + 6 cross-lane + 3 cross-wave folds, <= 32 for every shape below) and in fp64 after that:
# |error| <= 32 * 2^-24 * sum |terms| is the textbook bound of such a sum.
SUM_CHAIN = 32


def _off_the_relu_edge(x, gamma, beta, margin=1e-4):
    """Moves the few elements whose pre-ReLU output lies within `margin` of zero: there the sign of y -- and with it a whole term of the
    backward sums -- is decided by rounding, and neither answer is wrong.  margin is 50x the widest bar of y used below."""
    x = x.copy()
    for _ in range(20):
        pre = bnref.reference(x, gamma, beta, None, None, MOMENTUM, EPS, True, 0)['y']
        near = np.abs(pre) < margin
        if not near.any():
            return x
        x[near] += F32(0.01)
    raise AssertionError('could not move the data off the ReLU edge')


def _composed_case(rows, C_, relu, seed):
    rng, x, gamma, beta, dy = _data(rows, C_, seed, relu_input=bool(relu & 2))
    if relu & 1:
        x = _off_the_relu_edge(x, gamma, beta)
    rm0, rv0 = _running(rng, x)
    return x, gamma, beta, dy, rm0, rv0


def _plain_fwd_bwd(x, gamma, beta, dy, rm0, rv0, relu, training):
    lib, st = _lib.lib(), _lib.current_stream()
    rows, C_ = x.shape
    ws, nws = _ws(C_)
    o = dict(y=torch.empty((rows, C_), device='cuda'), mean=torch.empty(C_, device='cuda'), rstd=torch.empty(C_, device='cuda'), rm=_dev(rm0), rv=_dev(rv0),
             nbt=torch.tensor([7], dtype=torch.int64, device='cuda'), dx=torch.empty((rows, C_), device='cuda'), dgamma=torch.empty(C_, device='cuda'),
             dbeta=torch.empty(C_, device='cuda'))
    xd, gd, bd, dyd = _dev(x), _dev(gamma), _dev(beta), _dev(dy)
    assert lib.ssdk_batchnorm_fwd(_p(xd), rows, C_, _p(gd), _p(bd), _p(o['rm']), _p(o['rv']), _p(o['nbt']), MOMENTUM, EPS, training, relu & 1, _p(o['y']),
                                  _p(o['mean']), _p(o['rstd']), _p(ws), nws, st) == OK
    assert lib.ssdk_batchnorm_bwd(_p(xd), _p(o['y']) if relu & 1 else None, _p(dyd), rows, C_, _p(gd), _p(o['mean']), _p(o['rstd']), relu, training,
                                  _p(o['dx']), _p(o['dgamma']), _p(o['dbeta']), _p(ws), nws, st) == OK
    return {k: _np(v) for k, v in o.items()}


def _assert_composed(got, x, gamma, beta, dy, rm0, rv0, relu, training, info=None, channels=None):
    args = (x, gamma, beta, rm0, rv0, MOMENTUM, EPS, bool(training), relu, dy)
    ref, ideal = bnref.reference(*args), bnref.ideal_fp32(*args)
    sel = slice(None) if channels is None else channels
    _assert_ulps(got['mean'][sel], ref['save_mean'][sel], 'save_mean')
    _assert_ulps(got['rstd'][sel], ref['save_rstd'][sel], 'save_rstd')
    _assert_ulps(got['rm'][sel], ref['running_mean'][sel], 'running_mean')
    _assert_ulps(got['rv'][sel], ref['running_var'][sel], 'running_var')
    _assert_elementwise(got['y'][:, sel], ideal['y'][:, sel], ref['y'][:, sel], 'y', info)
    if relu & 1:
        assert np.array_equal(got['y'] > 0, ref['y'] > 0)
    _assert_elementwise(got['dx'][:, sel], ideal['dx'][:, sel], ref['dx'][:, sel], 'dx', info)
    g = np.asarray(dy, np.float64) * (ref['y'] > 0) if relu & 1 else np.asarray(dy, np.float64)
    u = SUM_CHAIN * 2.0 ** -24
    # dgamma also carries the error of the library's fp32 xhat: mean within 4 ulp (its bar above) and the rounding of x - mean, times
    # rstd; rstd within 4 ulp and the rounding of the product
    xh_err = (4.5 * np.spacing(np.maximum(np.abs(x), np.abs(ref['save_mean']).astype(F32))) * ref['save_rstd'] + 6 * 2.0 ** -23 * np.abs(ref['xhat'])) * np.abs(g)
    assert (np.abs(got['dbeta'] - ref['dbeta']) <= u * np.abs(g).sum(axis=0) + 2.0 ** -24 * np.abs(ref['dbeta']))[sel].all(), 'dbeta'
    assert (np.abs(got['dgamma'] - ref['dgamma']) <= u * np.abs(g * ref['xhat']).sum(axis=0) + xh_err.sum(axis=0) + 2.0 ** -24 * np.abs(ref['dgamma']))[sel].all(), 'dgamma'
    return ref


COMPOSED = [(257, 128, 1), (300, 132, 3), (70, 896, 0)]


@pytest.mark.parametrize('training', [1, 0])
@pytest.mark.parametrize('rows,C_,relu', COMPOSED)
def test_fwd_and_bwd_against_the_reference(rows, C_, relu, training):
    case = _composed_case(rows, C_, relu, 31)
    if not training and relu & 1:   # (evaluation mode: the edge is that of the running statistics' output)
        x, gamma, beta, dy, rm0, rv0 = case
        pre = bnref.reference(x, gamma, beta, rm0, rv0, MOMENTUM, EPS, False, 0)['y']
        x = x.copy(); x[np.abs(pre) < 1e-4] += F32(0.01)
        case = (x,) + case[1:]
    got = _plain_fwd_bwd(*case, relu, training)
    assert got['nbt'][0] == (8 if training else 7)
    _assert_composed(got, *case, relu, training)


@pytest.mark.parametrize('rows,C_,relu', COMPOSED)
def test_chained_entry_points_over_three_cycles(rows, C_, relu):
    """ssdk_batchnorm_fwd_chained / _bwd_chained on one pair of buffers: the forward finds zeros in its own buffer and zero-fills the
    backward's (NaN before the first call), the backward the reverse; every output has the bits of the plain entry points."""
    lib, st = _lib.lib(), _lib.current_stream()
    fwd_sums, bwd_sums = _sums_buffer(C_, fill=0.0), _sums_buffer(C_, fill=np.nan)
    rm = rv = None
    nbt = torch.tensor([2 ** 32 + 5], dtype=torch.int64, device='cuda')
    for cycle in range(3):
        x, gamma, beta, dy, rm0, rv0 = _composed_case(rows, C_, relu, 40 + cycle)
        if cycle == 0:
            rm, rv, rm_plain, rv_plain = _dev(rm0), _dev(rv0), rm0, rv0
        plain = _plain_fwd_bwd(x, gamma, beta, dy, rm_plain, rv_plain, relu, 1)
        rm_plain, rv_plain = plain['rm'], plain['rv']
        xd, gd, bd, dyd = _dev(x), _dev(gamma), _dev(beta), _dev(dy)
        y, mean, rstd = torch.empty((rows, C_), device='cuda'), torch.empty(C_, device='cuda'), torch.empty(C_, device='cuda')
        dx, dgamma, dbeta = torch.empty((rows, C_), device='cuda'), torch.empty(C_, device='cuda'), torch.empty(C_, device='cuda')
        assert lib.ssdk_batchnorm_fwd_chained(_p(xd), rows, C_, _p(gd), _p(bd), _p(rm), _p(rv), _p(nbt), MOMENTUM, EPS, relu & 1, _p(y), _p(mean), _p(rstd),
                                              _p(fwd_sums), _p(bwd_sums), st) == OK
        got = _np(bwd_sums)
        assert (got[:2 * C_ + 2] == 0.0).all() and _tail_untouched(got, C_), cycle
        assert _np(fwd_sums)[2 * C_] == rows
        assert lib.ssdk_batchnorm_bwd_chained(_p(xd), _p(y) if relu & 1 else None, _p(dyd), rows, C_, _p(gd), _p(mean), _p(rstd), relu, _p(dx), _p(dgamma),
                                              _p(dbeta), _p(bwd_sums), _p(fwd_sums), st) == OK
        got = _np(fwd_sums)
        assert (got[:2 * C_ + 2] == 0.0).all() and _tail_untouched(got, C_), cycle
        assert int(nbt) == 2 ** 32 + 6 + cycle
        chained = dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv, dx=dx, dgamma=dgamma, dbeta=dbeta)
        for k, v in chained.items():
            assert np.array_equal(_np(v).view(np.uint32), plain[k].view(np.uint32)), (k, cycle)
        if cycle == 0:
            _assert_composed(plain, x, gamma, beta, dy, rm0, rv0, relu, 1)


# ---- (d) conditioning -------------------------------------------------------------------------------------------------------------------

RATIOS = [0.0, 3.0, 30.0, 300.0, 3000.0]   # |mean| / std of a channel


def _conditioning_case(rows, C_):
    """Channel c: mean / std = RATIOS[c % 5] (either sign), std in {0.5, 1, 2}; channel C-2 all zero, channel C-1 constant 3.1.
    x = float32(mu_c) + float32(sigma_c n) in ONE float32 addition, so that a 1 x 1 convolution with the identity as its weight and mu
    as its bias reproduces it bit for bit."""
    rng = np.random.default_rng(1000 * C_ + rows)
    c = np.arange(C_)
    ratio = np.array(RATIOS)[c % 5]
    sigma = np.array([0.5, 1.0, 2.0])[(c // 5) % 3]
    mu = (ratio * sigma * np.where(c % 2 == 1, -1.0, 1.0)).astype(F32)
    u = (rng.standard_normal((rows, C_)) * sigma).astype(F32)
    u[:, C_ - 2], mu[C_ - 2], ratio[C_ - 2] = 0.0, 0.0, -1.0
    u[:, C_ - 1], mu[C_ - 1], ratio[C_ - 1] = 0.0, F32(3.1), -2.0
    x = u + mu
    gamma = (rng.uniform(0.5, 1.5, C_) * np.where(c % 4 == 1, -1.0, 1.0)).astype(F32)
    beta = rng.standard_normal(C_).astype(F32)
    dy = rng.standard_normal((rows, C_)).astype(F32)
    rm0, rv0 = _running(rng, x)
    return dict(x=x, u=u, mu=mu, ratio=ratio, gamma=gamma, beta=beta, dy=dy, rm0=rm0, rv0=rv0)


def _check_conditioning(got, case, channels, label):
    """y, save_mean, save_rstd, running statistics and dx of `channels` at the bars of (b); for the all-zero and the constant channel
    the forward (y = beta) and dbeta only: rstd = 1 / sqrt(eps) makes their dx rounding noise times 316."""
    x, gamma, beta, dy, rm0, rv0 = (case[k] for k in ('x', 'gamma', 'beta', 'dy', 'rm0', 'rv0'))
    args = (x, gamma, beta, rm0, rv0, MOMENTUM, EPS, True, 0, dy)
    ref, ideal = bnref.reference(*args), bnref.ideal_fp32(*args)
    failures = []

    def check(ok, what, figures):
        print(f'{label} {what}: {figures}')
        if not ok:
            failures.append((what, figures))

    for r in sorted(set(case['ratio'][channels])):
        sel = channels & (case['ratio'] == r)
        name = {-1.0: 'zero channel', -2.0: 'constant channel'}.get(r, f'mean/std {r:g}')
        ey, by = np.abs(got['y'] - ref['y']).max(axis=0)[sel], bnref.elementwise_bar(ideal['y'], ref['y'])[sel]
        check((ey <= by).all(), f'{name} y', f'max error {ey.max():.3g}, bar {by[np.argmax(ey / by)]:.3g}')
        if 'rv' in got:
            ur = bnref.ulps_fp32(got['rv'], ref['running_var'])[sel]
            check((ur <= 4).all(), f'{name} running_var', f'{ur.max():.3g} ulp')
            um = bnref.ulps_fp32(got['rm'], ref['running_mean'])[sel]
            check((um <= 4).all(), f'{name} running_mean', f'{um.max():.3g} ulp')
        if 'mean' in got:
            um = bnref.ulps_fp32(got['mean'], ref['save_mean'])[sel]
            us = bnref.ulps_fp32(got['rstd'], ref['save_rstd'])[sel]
            check((um <= 4).all() and (us <= 4).all(), f'{name} save_mean / save_rstd', f'{um.max():.3g} / {us.max():.3g} ulp')
        eb = np.abs(got['dbeta'] - ref['dbeta'])[sel]
        bb = (SUM_CHAIN * 2.0 ** -24 * np.abs(dy.astype(np.float64)).sum(axis=0) + 2.0 ** -24 * np.abs(ref['dbeta']))[sel]
        check((eb <= bb).all(), f'{name} dbeta', f'max error {eb.max():.3g}, bar {bb[np.argmax(eb / bb)]:.3g}')
        if r >= 0:
            ed, bd = np.abs(got['dx'] - ref['dx']).max(axis=0)[sel], bnref.elementwise_bar(ideal['dx'], ref['dx'])[sel]
            check((ed <= bd).all(), f'{name} dx', f'max error {ed.max():.3g}, bar {bd[np.argmax(ed / bd)]:.3g}')
    assert not failures, failures


CONDITIONING = [(rows, C_) for C_ in (20, 32) for rows in (2, 64, 1000, 8192)]


@pytest.mark.parametrize('rows,C_', CONDITIONING)
def test_conditioning_of_the_statistics_pass(rows, C_):
    """ssdk_batchnorm_fwd / _bwd on channels whose mean is 0 ... 3000 standard deviations, one all-zero and one constant channel.
    With fp32 partial sums of x and x^2 (before the reduction kernel accumulated in fp64) every channel from mean / std = 30 upward
    missed these bars; see DESIGN.md, "BatchNorm statistics: conditioning", for the figures."""
    case = _conditioning_case(rows, C_)
    got = _plain_fwd_bwd(case['x'], case['gamma'], case['beta'], case['dy'], case['rm0'], case['rv0'], 0, 1)
    _check_conditioning(got, case, np.ones(C_, bool), f'[stats pass {rows}x{C_}]')


def _through_the_conv_epilogue(case, B, H, W):
    """ops.conv2d_batch_norm with a 1 x 1 convolution: identity weight, bias mu -- its output is x, bit for bit, and its epilogue
    accumulates the statistics."""
    from single_shot_detection_amd import ops
    C_ = case['x'].shape[1]
    bn = torch.nn.BatchNorm2d(C_, eps=1e-5, momentum=0.1).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(_dev(case['gamma'])); bn.bias.copy_(_dev(case['beta']))
        bn.running_mean.copy_(_dev(case['rm0'])); bn.running_var.copy_(_dev(case['rv0']))
    weight = torch.eye(C_, device='cuda').reshape(C_, C_, 1, 1).contiguous(memory_format=torch.channels_last)
    bias = _dev(case['mu'])
    u = _dev(case['u']).reshape(B, H, W, C_).permute(0, 3, 1, 2).requires_grad_(True)   # (NCHW view of NHWC memory: channels_last)
    with torch.no_grad():
        xc = ops.conv2d(u.detach(), weight, bias, 1, 0)
    assert np.array_equal(_np(xc.permute(0, 2, 3, 1).reshape(-1, C_)).view(np.uint32), case['x'].view(np.uint32)), 'the convolution does not reproduce x'
    before = ops.fused_stats_calls
    y = ops.conv2d_batch_norm(u, weight, bias, 1, 0, bn)
    assert ops.fused_stats_calls == before + 1
    y.backward(_dev(case['dy']).reshape(B, H, W, C_).permute(0, 3, 1, 2))
    rows = lambda t: _np(t.detach().permute(0, 2, 3, 1).reshape(-1, C_))
    return dict(y=rows(y), dx=rows(u.grad), rm=_np(bn.running_mean), rv=_np(bn.running_var), dgamma=_np(bn.weight.grad), dbeta=_np(bn.bias.grad))


MAPS = {2: (2, 1, 1), 64: (1, 8, 8), 1000: (1, 25, 40), 8192: (2, 64, 64)}


@pytest.mark.parametrize('rows,C_', CONDITIONING)
def test_conditioning_of_the_conv_epilogue_statistics_well_conditioned_channels(rows, C_):
    """The same data with the statistics taken by the convolution's epilogue (ssdk_conv_desc::stats): the channels with mean / std <= 3,
    the all-zero and the constant channel."""
    case = _conditioning_case(rows, C_)
    got = _through_the_conv_epilogue(case, *MAPS[rows])
    _check_conditioning(got, case, case['ratio'] <= 3.0, f'[conv epilogue {rows}x{C_}]')


@pytest.mark.parametrize('rows,C_', CONDITIONING)
def test_conditioning_of_the_conv_epilogue_statistics_large_means(rows, C_):
    """... and the channels with mean / std of 30, 300 and 3000."""
    case = _conditioning_case(rows, C_)
    got = _through_the_conv_epilogue(case, *MAPS[rows])
    _check_conditioning(got, case, case['ratio'] >= 30.0, f'[conv epilogue {rows}x{C_}]')


# ---- (e) refusals -----------------------------------------------------------------------------------------------------------------------

SENTINEL = 1234.5


class _Call(object):
    """Valid arguments of every entry point on an 8 x C problem, output buffers pre-filled with a sentinel; `call` replaces some."""

    def __init__(self, C_=8, rows=8):
        self.C, self.rows = C_, rows
        f = lambda *shape: torch.full(shape, SENTINEL, device='cuda')
        # inputs live one float inside a larger buffer so that `offset` can hand out a pointer 4 bytes off a 16-byte boundary
        self.t = dict(x=f(rows * C_ + 4), y=f(rows * C_ + 4), dy=f(rows * C_ + 4), dx=f(rows * C_ + 4), gamma=f(C_), beta=f(C_), rm=f(C_), rv=f(C_),
                      mean=f(C_), rstd=f(C_), dgamma=f(C_), dbeta=f(C_), nbt=torch.full((1,), 99, dtype=torch.int64, device='cuda'),
                      sums=torch.full((2 * C_ + 2,), SENTINEL, dtype=torch.float64, device='cuda'),
                      other=torch.full((2 * C_ + 2,), SENTINEL, dtype=torch.float64, device='cuda'))
        self.ws, self.nws = _ws(C_)
        self.ws.fill_(17)

    def ptr(self, name, offset=()):
        return C.c_void_p(self.t[name].data_ptr() + (4 if name in offset else 0))

    def call(self, entry, channels=None, offset=(), ws_bytes=None, same_buffers=False, training=1, no_running=False):
        lib, st, p = _lib.lib(), _lib.current_stream(), lambda n: self.ptr(n, offset)
        C_, rows = (self.C if channels is None else channels), self.rows
        nws = self.nws if ws_bytes is None else ws_bytes
        rm, rv = (None, None) if no_running else (p('rm'), p('rv'))
        other = p('sums') if same_buffers else p('other')
        fwd_head = (p('x'), rows, C_, p('gamma'), p('beta'), rm, rv, p('nbt'), MOMENTUM, EPS)
        if entry == 'fwd':
            return lib.ssdk_batchnorm_fwd(*fwd_head, training, 0, p('y'), p('mean'), p('rstd'), _p(self.ws), nws, st)
        if entry == 'bwd':
            return lib.ssdk_batchnorm_bwd(p('x'), p('y'), p('dy'), rows, C_, p('gamma'), p('mean'), p('rstd'), 1, training, p('dx'), p('dgamma'), p('dbeta'),
                                          _p(self.ws), nws, st)
        if entry in ('stats', 'stats_accumulate'):
            return getattr(lib, 'ssdk_batchnorm_' + entry)(p('x'), rows, C_, p('sums'), st)
        if entry == 'apply':
            return lib.ssdk_batchnorm_apply(*fwd_head, 0, p('y'), p('mean'), p('rstd'), p('sums'), 0, st)
        if entry in ('fwd_chained', 'apply_chained'):
            return getattr(lib, 'ssdk_batchnorm_' + entry)(*fwd_head, 0, p('y'), p('mean'), p('rstd'), p('sums'), other, st)
        if entry == 'bwd_stats':
            return lib.ssdk_batchnorm_bwd_stats(p('x'), p('y'), p('dy'), rows, C_, p('mean'), p('rstd'), 1, p('sums'), st)
        if entry == 'bwd_apply':
            return lib.ssdk_batchnorm_bwd_apply(p('x'), p('y'), p('dy'), rows, C_, p('gamma'), p('mean'), p('rstd'), 1, 1, p('sums'), None, None, p('dx'),
                                                p('dgamma'), p('dbeta'), st)
        if entry == 'bwd_chained':
            return lib.ssdk_batchnorm_bwd_chained(p('x'), p('y'), p('dy'), rows, C_, p('gamma'), p('mean'), p('rstd'), 1, p('dx'), p('dgamma'), p('dbeta'),
                                                  p('sums'), other, st)
        raise KeyError(entry)

    def untouched(self):
        torch.cuda.synchronize()
        ok = all(bool((v == (99 if k == 'nbt' else SENTINEL)).all()) for k, v in self.t.items())
        return ok and bool((self.ws == 17).all())


ENTRIES = ['fwd', 'bwd', 'stats', 'stats_accumulate', 'apply', 'bwd_stats', 'bwd_apply', 'fwd_chained', 'apply_chained', 'bwd_chained']
ALIGNED = {   # the buffers each entry point requires on a 16-byte boundary
    'fwd': ['x', 'y'], 'apply': ['x', 'y'], 'fwd_chained': ['x', 'y'], 'apply_chained': ['x', 'y'], 'stats': ['x'], 'stats_accumulate': ['x'],
    'bwd_stats': ['x', 'y', 'dy'], 'bwd': ['x', 'y', 'dy', 'dx'], 'bwd_apply': ['x', 'y', 'dy', 'dx'], 'bwd_chained': ['x', 'y', 'dy', 'dx'],
}


@pytest.mark.parametrize('entry', ENTRIES)
def test_channels_not_a_multiple_of_four_are_refused(entry):
    c = _Call()
    for channels in (6, 7, 1):
        assert c.call(entry, channels=channels) == E_UNSUPPORTED, channels
    assert c.untouched()


@pytest.mark.parametrize('entry', ENTRIES)
def test_buffers_off_a_16_byte_boundary_are_refused(entry):
    c = _Call()
    for name in ALIGNED[entry]:
        assert c.call(entry, offset=(name,)) == E_UNSUPPORTED, name
    assert c.untouched()


def test_other_refusals_launch_nothing():
    c = _Call()
    assert c.call('fwd', ws_bytes=c.nws - 1) == E_WORKSPACE
    assert c.call('bwd', ws_bytes=c.nws - 1) == E_WORKSPACE
    for entry in ('fwd_chained', 'apply_chained', 'bwd_chained'):
        assert c.call(entry, same_buffers=True) == E_INVALID, entry
    assert c.call('fwd', training=0, no_running=True) == E_INVALID
    assert _lib.lib().ssdk_relu_bwd(c.ptr('y'), c.ptr('dy'), 6, c.ptr('dx'), _lib.current_stream()) == E_INVALID
    assert c.untouched()
    assert b'ssdk_relu_bwd' in _lib.lib().ssdk_last_error_string()


# ---- (f) nearest-neighbour index arithmetic -----------------------------------------------------------------------------------------------

def _upsample_pairs(axis):
    fixed = (7, 4)
    for fine in range(1, 25):
        for coarse in range(1, fine + 1):
            yield ((fine, fixed[0], coarse, fixed[1]) if axis == 'h' else (fixed[0], fine, fixed[1], coarse))


@pytest.mark.parametrize('axis', ['h', 'w'])
def test_upsample_nearest_add_forward_equals_torch_cpu_for_every_size_pair(axis):
    """out = [fine +] nearest_upsample(coarse), bit for bit, for every pair 1 <= coarse <= fine <= 24 along one axis."""
    import torch.nn.functional as F
    lib, st = _lib.lib(), _lib.current_stream()
    B, C_ = 2, 8
    rng = np.random.default_rng(8)
    for hf, wf, hc, wc in _upsample_pairs(axis):
        coarse = torch.from_numpy(rng.standard_normal((B, hc, wc, C_), dtype=F32))
        fine = torch.from_numpy(rng.standard_normal((B, hf, wf, C_), dtype=F32))
        up = F.interpolate(coarse.permute(0, 3, 1, 2), size=(hf, wf), mode='nearest').permute(0, 2, 3, 1)
        cd, fd = coarse.cuda(), fine.cuda()
        out0, out1 = torch.full((B, hf, wf, C_), 5.0, device='cuda'), torch.full((B, hf, wf, C_), 5.0, device='cuda')
        assert lib.ssdk_upsample_nearest_add_fwd(None, _p(cd), B, hf, wf, hc, wc, C_, _p(out0), st) == OK
        assert lib.ssdk_upsample_nearest_add_fwd(_p(fd), _p(cd), B, hf, wf, hc, wc, C_, _p(out1), st) == OK
        assert torch.equal(out0.cpu(), up.contiguous()), (hf, wf, hc, wc)
        assert torch.equal(out1.cpu(), fine + up), (hf, wf, hc, wc)


@pytest.mark.parametrize('axis', ['h', 'w'])
def test_upsample_nearest_add_backward_loses_no_pixel_for_any_size_pair(axis):
    """dcoarse = scatter-add of an integer-valued dout over the index map (bnref.nearest_src_index, pinned against torch on the CPU):
    exact, so a fine pixel outside the kernel's candidate window would show."""
    lib, st = _lib.lib(), _lib.current_stream()
    B, C_ = 2, 8
    rng = np.random.default_rng(9)
    for hf, wf, hc, wc in _upsample_pairs(axis):
        dout = rng.integers(-4, 5, (B, hf, wf, C_)).astype(np.float64)
        want = np.zeros((B, hc, wc, C_))
        iy, ix = bnref.nearest_src_index(hc, hf), bnref.nearest_src_index(wc, wf)
        np.add.at(want, (slice(None), iy[:, None], ix[None, :]), dout)
        got = torch.full((B, hc, wc, C_), 5.0, device='cuda')
        assert lib.ssdk_upsample_nearest_add_bwd(_p(_dev(dout, F32)), B, hf, wf, hc, wc, C_, _p(got), st) == OK
        assert np.array_equal(_np(got), want), (hf, wf, hc, wc)
