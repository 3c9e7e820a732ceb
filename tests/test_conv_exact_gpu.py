"""The convolution GEMMs of csrc/conv.hip, entry point by entry point through the C ABI, on operands for which the right answer is
known EXACTLY: small integers.  Every product and every partial sum is then an integer below 2^24 (conv_reference.assert_exact, checked
on the CPU for every GEMM of every case), so the fp32 result is the same in any summation order, K split, atomic order and stream-K cut,
and the GPU result must EQUAL the float64 model of tests/conv_reference.py -- np.array_equal, no tolerance anywhere in this file.  The
same operands are exact in bf16, so the opt-in bf16x3 kernels must be bit-equal too.

Buffers: every input sits inside a larger allocation with NaN on both sides (at least the LDS-DMA kernel's deliberate over-read range
plus 4 KiB): a value read from there that reaches a result shows as NaN.  Every output sits between sentinels that must keep their
bits, and is pre-filled with NaN where the call overwrites (a missed zero-fill or an unwritten element shows) or with integers where it
accumulates.

Each case's comment carries the arithmetic that puts it on its dispatch path.  Which kernel a case really ran on is shown by the kernel
trace of this file, profiles/conv_exact_kernel_stats.md (DESIGN.md section 15 lists the instantiations seen there).  _plan() / _plan_dx()
ask the library itself: ssdk_debug_conv2d_plan builds the problems and the request of the real entry point and runs plan_launch
(csrc/conv_plan.h), the one function every launch is planned by, without touching a device.  So the comments' arithmetic is checked against
the rules that ship (tests/test_conv_reference.py runs the checks, no GPU needed), and the trace shows that the planned kernel is the
one that ran."""
import collections
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import conv_reference as cr
from single_shot_detection_amd import _lib

pytestmark = pytest.mark.gpu

OK, E_INVALID, E_WORKSPACE, E_UNSUPPORTED = 0, -1, -2, -3   # include/ssdk.h
F32 = np.float32
SENTINEL = F32(-1234.5)
SENTINEL64 = -1234.5
PAGE = 1024   # floats: 4 KiB


_alive = []


@pytest.fixture(autouse=True)
def _device_buffers_live_until_the_test_ends():
    """The library is handed raw pointers: everything made here stays alive until the test is over."""
    yield
    del _alive[:]


def _cdiv(a, b):
    return -(-a // b)


def _keep(t):
    _alive.append(t)
    return t


def _guarded_input(a, slack, shift=0):
    """Device address of `a` (as fp32) inside an allocation that is NaN for `slack` + 4 KiB floats on both sides; `shift` floats off
    16-byte alignment."""
    a = np.ascontiguousarray(a, F32).ravel()
    slack = (int(slack) + PAGE + 3) // 4 * 4
    host = np.full(2 * slack + a.size + shift, np.nan, F32)
    host[slack + shift:slack + shift + a.size] = a
    t = _keep(torch.from_numpy(host).cuda())
    assert t.data_ptr() % 16 == 0
    return t.data_ptr() + 4 * (slack + shift)


class _Output(object):
    """`n` elements between sentinels.  fill: NaN (the call overwrites), an array (it accumulates), or the sentinel itself (a refused
    call, a gap)."""

    def __init__(self, n, fill=np.nan, dtype=F32, slack=PAGE):
        self.n, self.slack, self.dtype = int(n), slack, dtype
        self.sent = SENTINEL if dtype == F32 else SENTINEL64
        host = np.full(self.n + 2 * slack, self.sent, dtype)
        host[slack:slack + self.n] = np.asarray(fill, dtype).ravel() if not np.isscalar(fill) else fill
        self.before = host.copy()
        self.t = _keep(torch.from_numpy(host).cuda())
        self.ptr = self.t.data_ptr() + host.itemsize * slack

    def read(self):
        """The payload, after checking that the bytes around it are the ones put there."""
        torch.cuda.synchronize()
        got = self.t.cpu().numpy()
        bits = np.uint32 if self.dtype == F32 else np.uint64
        s = self.slack
        assert np.array_equal(got[:s].view(bits), self.before[:s].view(bits)), 'bytes in front of an output were written'
        assert np.array_equal(got[s + self.n:].view(bits), self.before[s + self.n:].view(bits)), 'bytes behind an output were written'
        return got[s:s + self.n].copy()

    def untouched(self):
        got = self.read()
        bits = np.uint32 if self.dtype == F32 else np.uint64
        return np.array_equal(got.view(bits), self.before[self.slack:self.slack + self.n].view(bits))


def _workspace(nbytes):
    """A workspace of exactly nbytes with 4 KiB of 0xA5 behind it; returns (pointer, checker)."""
    t = _keep(torch.full((int(nbytes) + 4096,), 0xA5, dtype=torch.uint8, device='cuda'))

    def check():
        torch.cuda.synchronize()
        assert bool((t[int(nbytes):] == 0xA5).all().item()), 'bytes behind the workspace were written'
    return C.c_void_p(t.data_ptr()), check


@contextlib.contextmanager
def _deterministic(on):
    lib = _lib.lib()
    prev = lib.ssdk_set_deterministic(1 if on else 0)
    try:
        yield
    finally:
        lib.ssdk_set_deterministic(prev)


def _err():
    return _lib.lib().ssdk_last_error_string().decode('utf-8', 'replace')


# ---- problems and their exact answers ---------------------------------------------------------------------------------------------------

_SPEC_FIELDS = 'cin cout k stride pad H W B bias relu stats xr wr nnz dy_nnz salt'
Spec = collections.namedtuple('Spec', _SPEC_FIELDS)


def spec(cin, cout, k, stride, pad, H, B, W=None, bias=1, relu=0, stats=0, xr=(-3, 3), wr=(-2, 2), nnz=0, dy_nnz=0, salt=0):
    """(cin, cout, k, stride, pad) on a map of H x W (square unless W is given) at batch B.  nnz: non-zero weights per output channel
    (0 = dense); dy_nnz: non-zero gradient rows per output channel (0 = dense)."""
    return Spec(cin, cout, k, stride, pad, H, H if W is None else W, B, bias, relu, stats, tuple(xr), tuple(wr), nnz, dy_nnz, salt)


def _sparsify(m, nnz, step):
    """Keep `nnz` entries of every row of the matrix m (positions that move from row to row), zero the rest."""
    rows, K = m.shape
    j = np.arange(K)[None, :]
    r = np.arange(rows)[:, None]
    return np.where((j + step * r) % K < nnz, m, 0)


@functools.lru_cache(maxsize=None)
def _forward(s):
    """Integer operands and the exact forward answer of a Spec (shared by every variant of the case; never modified)."""
    x = cr.int_pattern((s.B, s.H, s.W, s.cin), s.xr[0], s.xr[1], 1 + s.salt)
    w = cr.int_pattern((s.cout, s.k, s.k, s.cin), s.wr[0], s.wr[1], 2 + s.salt)
    if s.nnz:   # exactly nnz non-zero weights per output channel
        keep = _sparsify(np.ones((s.cout, s.k * s.k * s.cin), np.int64), s.nnz, 5).reshape(w.shape)
        w = np.where(keep == 1, np.where(w == 0, s.wr[1], w), 0)
    b = cr.int_pattern((s.cout,), s.wr[0], s.wr[1], 3 + s.salt) if s.bias else None
    y = cr.conv_fwd(x, w, b, s.stride, s.pad, s.relu)
    out = dict(x=x, w=w, b=b, y=y, ho=y.shape[1], wo=y.shape[2])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _backward(s):
    f = _forward(s)
    dy = cr.int_pattern((s.B, f['ho'], f['wo'], s.cout), s.xr[0], s.xr[1], 4 + s.salt)
    if s.dy_nnz:
        keep = _sparsify(np.ones((s.cout, s.B * f['ho'] * f['wo']), np.int64), s.dy_nnz, 3).T.reshape(dy.shape)
        dy = np.where(keep == 1, np.where(dy == 0, s.xr[1], dy), 0)
    dx, dw, db = cr.conv_bwd(f['x'], f['w'], dy, s.stride, s.pad)
    out = dict(dy=dy, dx=dx, dw=dw, db=db)
    for v in out.values():
        v.setflags(write=False)
    return out


def _slack(s):
    """Floats of NaN around every input of a Spec: more than the LDS-DMA kernel's over-read, (ksize + pad) * (W + 1) * channels, of
    the forward (x) and of the mirrored-tap backward (dy: pad up to ksize - 1) launch."""
    return 2 * s.k * (max(s.W, s.H) + 1) * max(s.cin, s.cout)


def _exact_forward(s):
    f = _forward(s)
    amax, bmax = int(np.abs(f['x']).max()), int(np.abs(f['w']).max())
    terms = s.nnz if s.nnz else s.k * s.k * s.cin
    cr.assert_exact(terms, amax, bmax, extra=bmax if s.bias else 0)
    if s.stats:   # rows * max(y^2): the fp64 sums equal the integer sums whatever an epilogue accumulates in fp32 first
        ymax = int(np.abs(f['y']).max())
        cr.assert_exact(s.B * f['ho'] * f['wo'], ymax, ymax)


# ---- the dispatch rules, asked of the library ---------------------------------------------------------------------------------------------

def _planned(specs, direction, with_ws=False, det=False, no_dma=False, aligned=True):
    """ssdk_debug_conv2d_plan (host only: no device, the fake pointers are never read) on these Specs, under SSDK_CONV_NO_DMA and the
    deterministic flag as given (both restored): the launches it reports."""
    lib = _lib.lib()
    descs = (_lib.ConvDesc * len(specs))()
    for d, s in zip(descs, specs):
        d.x, d.hin, d.win, d.cin = 4096 + (0 if aligned else 4), s.H, s.W, s.cin
        d.w, d.bias, d.y, d.dy, d.dx = 4096, (4096 if s.bias else None), 4096, 4096, 4096
        d.cout, d.ksize, d.stride, d.pad, d.relu, d.stats = s.cout, s.k, s.stride, s.pad, s.relu, (4096 if s.stats else None)
    out, n = (_lib.ConvPlanLaunch * 3)(), C.c_int(0)
    before = os.environ.pop('SSDK_CONV_NO_DMA', None)
    try:
        if no_dma:
            os.environ['SSDK_CONV_NO_DMA'] = '1'
        with _deterministic(det):
            rc = lib.ssdk_debug_conv2d_plan(descs, len(specs), specs[0].B, direction, int(with_ws), out, 3, C.byref(n))
    finally:
        os.environ.pop('SSDK_CONV_NO_DMA', None)
        if before is not None:
            os.environ['SSDK_CONV_NO_DMA'] = before
    assert rc == OK, (rc, _err())
    return [out[i] for i in range(n.value)]


def _plan(specs, with_ws=False, det=False, no_dma=False, aligned=True):
    """ssdk_conv2d_fwd_ws on these Specs: (kernel, [(column blocks, K splits, half tile)] per problem)."""
    launch, = _planned(specs, 0, with_ws, det, no_dma, aligned)
    return launch.kernel.decode(), [(launch.n_blocks[i], launch.k_splits[i], launch.half_last[i]) for i in range(launch.count)]


def _plan_dx(s, det=False, no_dma=False):
    """The data-gradient launch of ssdk_conv2d_bwd for one Spec: (kernel, column blocks, K splits)."""
    launch, = _planned([s], 1, False, det, no_dma)
    return launch.kernel.decode(), launch.n_blocks[0], launch.k_splits[0]


# ---- ssdk_conv2d_fwd / _ws / _fast --------------------------------------------------------------------------------------------------------

def _stats_prior(cout):
    p = np.zeros(2 * cout + 2)
    p[:2 * cout] = cr.int_pattern((2 * cout,), -50, 50, 11)
    return p


def _streamk_workspace():
    n = _lib.lib().ssdk_heads_fwd_workspace_bytes()
    t = _keep(torch.zeros((n,), dtype=torch.uint8, device='cuda'))   # zero-filled ONCE, as ssdk.h asks
    return t, n


def _streamk_flags(t):
    """The flag region of a stream-K workspace (its last 256-byte-rounded part): [512] per-workgroup flags -- back to 0 once their partial
    tile was consumed --, the timeout counter, and the launch counter of the last stream-K launch that ran on the workspace.  Returns
    (the region without the timeout counter, the timeout counter)."""
    torch.cuda.synchronize()
    words = t[t.numel() - 2304:].cpu().numpy().view(np.uint32)[:514]
    return np.delete(words, 512), int(words[512])


def _timeouts(t, n):
    word = C.c_uint(77)
    assert _lib.lib().ssdk_heads_fwd_timeouts(C.c_void_p(t.data_ptr()), n, _lib.current_stream(), C.byref(word)) == OK
    return word.value


def _forward_descs(specs, x_shift=0, share_w=False):
    descs = (_lib.ConvDesc * len(specs))()
    outs = []
    w_of = {}
    for d, s in zip(descs, specs):
        _exact_forward(s)
        f = _forward(s)
        d.x, d.hin, d.win, d.cin = _guarded_input(f['x'], _slack(s), x_shift), s.H, s.W, s.cin
        key = (s.cout, s.k, s.cin, s.wr, s.nnz, s.salt)
        if share_w and key in w_of:
            d.w, d.bias = w_of[key]
        else:
            d.w = _guarded_input(f['w'], _slack(s))
            d.bias = _guarded_input(f['b'], 0) if s.bias else None
            w_of[key] = (d.w, d.bias)
        d.cout, d.ksize, d.stride, d.pad, d.relu = s.cout, s.k, s.stride, s.pad, s.relu
        y = _Output(f['y'].size)
        d.y = y.ptr
        st = None
        if s.stats:
            st = _Output(2 * s.cout + 2, _stats_prior(s.cout), dtype=np.float64, slack=4)
            d.stats = st.ptr
        outs.append((y, st))
    return descs, outs


def _check_forward(specs, outs, what=''):
    for i, (s, (y, st)) in enumerate(zip(specs, outs)):
        f = _forward(s)
        got = y.read()
        assert np.array_equal(got, f['y'].ravel()), (what, 'y of descriptor', i, s, int((got != f['y'].ravel()).sum()), int(np.isnan(got).sum()))
        if st is not None:
            want = _stats_prior(s.cout) + cr.stats(f['y'])
            assert np.array_equal(st.read(), want), (what, 'stats of descriptor', i, s)


def _run_forward(specs, entry='fwd', x_shift=0, share_w=False, ws=None):
    """One grouped call; every output and statistics buffer must equal the model.  entry: 'fwd', 'ws' (ws = (tensor, bytes)), 'fast'."""
    lib, st = _lib.lib(), _lib.current_stream()
    B = specs[0].B
    assert all(s.B == B for s in specs)
    descs, outs = _forward_descs(specs, x_shift, share_w)
    if entry == 'fwd':
        rc = lib.ssdk_conv2d_fwd(descs, len(specs), B, st)
    elif entry == 'ws':
        rc = lib.ssdk_conv2d_fwd_ws(descs, len(specs), B, C.c_void_p(ws[0].data_ptr()), ws[1], st)
    else:
        n = lib.ssdk_conv2d_fwd_fast_workspace_bytes(descs, len(specs))
        wp, wcheck = _workspace(n)
        rc = lib.ssdk_conv2d_fwd_fast(descs, len(specs), B, 3, wp, n, st)
    assert rc == OK, (rc, _err())
    _check_forward(specs, outs, entry)
    if entry == 'fast':
        wcheck()


# (a) 32 -> 256, 1 x 1, 64 x 64, batch 4: 16 384 rows = 128 row tiles; 8 column tiles = 2 blocks of 128 columns; 128 x 2 = 256 workgroups:
#     not below 256, so no K split (one slice anyway) and no narrowing -> igemm_dma_kernel<generic>, 128-column blocks, whole K
CASE_A = spec(32, 256, 1, 1, 0, 64, 4)
# (b) 64 -> 64, 3 x 3, 8 x 8, batch 2, ReLU: 128 rows = 1 row tile, 2 column tiles; the ReLU forbids a K split; 1 workgroup < 256 ->
#     narrowed to 2 blocks of one tile each -> the one-tile three-stage instantiation
CASE_B = spec(64, 64, 3, 1, 1, 8, 2, relu=1)
# (c) 128 -> 64, 3 x 3 / 2, 20 x 20, batch 4: 10 x 10 x 4 = 400 rows = 4 row tiles; 9 x 128 / 32 = 36 slices >= 32 -> rule "3..8 row
#     tiles": 2 column blocks, splits = min(max(2, 256 / 8), 36 / 8) = 4
CASE_C = spec(128, 64, 3, 2, 1, 20, 4)
# (d) as (b) without the ReLU: 1 row tile, 18 slices, 8 workgroup slots -> fall-through rule: min(ceil(512 / 8), 18 / 4) = 4 splits,
#     then narrowed for the atomics to 2 column blocks
CASE_D = spec(64, 64, 3, 1, 1, 8, 2)
# (e) 512 -> 256, 1 x 1, 32 x 32, batch 8: 8 192 rows = 64 row tiles, 8 column tiles, 16 slices; 64 x 2 = 128 < 256 workgroups, and
#     64 x (8 / 2) = 256 >= 256 with <= 32 slices -> 4 blocks of 64 columns, no split
CASE_E = spec(512, 256, 1, 1, 0, 32, 8)
# (f) cout 40 (40 % 32 = 8) and 48 (48 % 32 = 16): the last column tile is at most 16 wide -> half-width last tile.  cout 48 is 1 x 1: one
#     slice, no split, and `stats` in the epilogue rules the half tile out.  cout 40 is 3 x 3 on 243 rows = 2 row tiles, 9 slices:
#     min(ceil(512 / 8), 9 / 4) = 2 splits -- the half tile WITH the atomic epilogue, and `stats` as a pass of its own behind it
CASE_F40 = spec(32, 40, 3, 1, 1, 9, 3)
CASE_F48 = spec(32, 48, 1, 1, 0, 9, 3)
# (g) cin 24: 16-byte rows but no whole 32-channel chunk -> register-staged float4 kernel
CASE_G = spec(24, 40, 3, 1, 1, 9, 3)
# (h) cin 3 and 6: rows that are no multiple of 16 bytes -> scalar kernel (and cin 32 one float off alignment, below)
CASE_H3 = spec(3, 40, 3, 2, 1, 9, 3)
CASE_H6 = spec(6, 36, 3, 1, 1, 9, 3)
CASE_H32 = spec(32, 40, 3, 1, 1, 9, 3, salt=3)
# (i) 32 -> 32, 3 x 3, 129 x 129, batch 8: 133 128 rows = 1 041 row tiles, 1 column block: ceil(1 041 / 8) x 8 = 1 048 workgroups = two
#     rounds of 512 and a tail round of 24 (<= 384); units = 1 041 x 9 x 2 = 18 738 -> min(512, 18 738 / 48 / 8 x 8) = 384 workgroups >= 256
CASE_I = spec(32, 32, 3, 1, 1, 129, 8, xr=(-1, 1), wr=(-1, 1), nnz=8)

DMA_CASES = {'a': CASE_A, 'b': CASE_B, 'c': CASE_C, 'd': CASE_D, 'e': CASE_E, 'f40': CASE_F40, 'f48': CASE_F48}


def check_forward_cases_land_on_their_paths():
    """The arithmetic of the comments above, against the library's own dispatch rules."""
    assert _plan([CASE_A]) == ('dma generic', [(2, 1, 0)])
    assert _plan([CASE_B]) == ('dma generic one-tile', [(2, 1, 0)])
    assert _plan([CASE_C]) == ('dma generic one-tile', [(2, 4, 0)])
    assert _plan([CASE_D]) == ('dma generic one-tile', [(2, 4, 0)])
    assert _plan([CASE_E]) == ('dma generic', [(4, 1, 0)])
    assert _plan([CASE_F40]) == ('dma generic', [(2, 2, 1)]) and _plan([CASE_F48]) == ('dma generic', [(2, 1, 1)])
    assert _plan([CASE_F40._replace(relu=1)]) == ('dma generic', [(2, 1, 1)])
    assert _plan([CASE_F48._replace(stats=1)]) == ('dma generic one-tile', [(2, 1, 0)])
    assert _plan([CASE_F40._replace(stats=1)]) == ('dma generic', [(2, 2, 1)])
    assert _plan([CASE_G])[0] == 'staged<4> generic'
    assert _plan([CASE_H3])[0] == 'staged<1> generic' and _plan([CASE_H6])[0] == 'staged<1> generic'
    assert _plan([CASE_H32], aligned=False)[0] == 'staged<1> generic'
    assert _plan([CASE_I], with_ws=True) == ('streamk', [(1, 1, 0)])
    assert _plan([CASE_I._replace(stats=1)], with_ws=True)[0] == 'streamk'
    assert _plan([CASE_A], with_ws=True) == ('dma generic', [(2, 1, 0)])
    for s in DMA_CASES.values():
        assert _plan([s], no_dma=True)[0] == 'staged<4> generic'
    # deterministic mode never splits K with atomics
    assert _plan([CASE_C], det=True)[1][0][1] == 1 and _plan([CASE_D], det=True)[1][0][1] == 1


@pytest.mark.parametrize('no_dma', [False, True])
@pytest.mark.parametrize('name', sorted(DMA_CASES))
def test_forward_dma_cases(name, no_dma, monkeypatch):
    """(a) .. (f), and each again on the register-staged float4 kernel (SSDK_CONV_NO_DMA is read on every call).  (c), (d): the output is
    NaN before the call, so the library's own zero-fill in front of the atomics is what is tested."""
    if no_dma:
        monkeypatch.setenv('SSDK_CONV_NO_DMA', '1')
    _run_forward([DMA_CASES[name]])


@pytest.mark.parametrize('no_dma', [False, True])
@pytest.mark.parametrize('cout', [40, 48])
def test_forward_half_width_last_tile_with_stats_and_with_relu(cout, no_dma, monkeypatch):
    """(f) once with `stats` (which rules the half tile out: the statistics epilogue walks whole tiles) and once with a fused ReLU."""
    if no_dma:
        monkeypatch.setenv('SSDK_CONV_NO_DMA', '1')
    base = CASE_F40 if cout == 40 else CASE_F48
    _run_forward([base._replace(stats=1, xr=(-1, 1), wr=(-1, 1), nnz=9)])
    _run_forward([base._replace(relu=1)])
    _run_forward([base._replace(relu=1, stats=1, xr=(-1, 1), wr=(-1, 1), nnz=9)])


@pytest.mark.parametrize('name,s,shift', [('g', CASE_G, 0), ('h3', CASE_H3, 0), ('h6', CASE_H6, 0), ('h32_off_alignment', CASE_H32, 1),
                                          ('g_relu', CASE_G._replace(relu=1), 0), ('h3_k1', spec(3, 8, 1, 2, 0, 7, 2), 0)])
def test_forward_register_staged_cases(name, s, shift):
    """(g), (h): the channel counts the LDS-DMA kernel cannot take, and an x that is not 16-byte aligned."""
    _run_forward([s], x_shift=shift)


def test_forward_stream_k_through_the_workspace():
    """(i), plain and with bias + stats; the flag region shows that the stream-K form ran (its launch-counter word changes with every
    stream-K launch), and stays all-zero for a launch that must not take it ((a): 256 workgroups are not two rounds)."""
    ws = _streamk_workspace()
    _run_forward([CASE_A], entry='ws', ws=ws)
    flags, timeouts = _streamk_flags(ws[0])
    assert not flags.any() and timeouts == 0, 'a launch of one round took stream-K'
    _run_forward([CASE_I], entry='ws', ws=ws)
    flags, timeouts = _streamk_flags(ws[0])
    assert flags.any() and timeouts == 0, 'the stream-K form did not run'
    assert _timeouts(*ws) == 0
    counter = int(flags[-1])
    _run_forward([CASE_I._replace(stats=1, salt=1)], entry='ws', ws=ws)
    flags, timeouts = _streamk_flags(ws[0])
    assert int(flags[-1]) not in (0, counter) and timeouts == 0, 'the stream-K form did not run with stats'
    assert not flags[:-1].any(), 'a consumed ready flag was left up'
    assert _timeouts(*ws) == 0 and _lib.lib().ssdk_streamk_poisoned() == 0


@pytest.mark.parametrize('force', ['1,1', '1,2', '2,3', '99,7'])
@pytest.mark.parametrize('name', ['d', 'c', 'wide'])
def test_forward_forced_decompositions(name, force, monkeypatch):
    """SSDK_CONV_FORCE = '<column blocks>,<K splits>' walks the decompositions of one small problem: one block, every tile its own block
    (99 -> tiles_n), 2, 3 and 7 splits of 18 / 36 / 27 slices (7 divides none of them; 'wide' has 3 column tiles, so 2 blocks are uneven)."""
    s = {'d': CASE_D, 'c': CASE_C, 'wide': spec(96, 72, 3, 1, 1, 11, 3, W=7)}[name]
    monkeypatch.setenv('SSDK_CONV_FORCE', force)
    _run_forward([s])
    _run_forward([s._replace(stats=1, xr=(-1, 1), wr=(-1, 1), nnz=6)])


# eight problems of different work (plan_launch orders them by K chain x columns per workgroup, so not in descriptor order): 1 x 1 and
# 3 x 3, both strides, a 1 x 1 map, H != W, maps of fewer than 128 rows, rows that are no multiple of 32 or 128
GROUP8 = [spec(32, 40, 1, 1, 0, 5, 3, W=7), spec(64, 64, 3, 1, 1, 13, 3), spec(32, 96, 3, 2, 1, 9, 3, W=12), spec(128, 32, 1, 2, 0, 7, 3),
          spec(64, 8, 3, 1, 1, 1, 3), spec(32, 160, 3, 1, 0, 6, 3, W=11), spec(96, 64, 3, 2, 2, 8, 3), spec(64, 64, 3, 1, 1, 5, 3, W=3, salt=7)]
GROUP8_STAGED = [s._replace(cin=s.cin - 8) for s in GROUP8]       # 24, 56, ...: the register-staged float4 kernel
GROUP8_SCALAR = [s._replace(cin=s.cin // 8 + 1) for s in GROUP8]  # 5, 9, ...: the scalar kernel


@pytest.mark.parametrize('variant', ['dma', 'no_dma', 'staged', 'scalar', 'deterministic', 'shared_w', 'stats'])
def test_forward_group_of_eight(variant, monkeypatch):
    specs = {'staged': GROUP8_STAGED, 'scalar': GROUP8_SCALAR}.get(variant, GROUP8)
    if variant == 'no_dma':
        monkeypatch.setenv('SSDK_CONV_NO_DMA', '1')
    if variant == 'stats':
        specs = [s._replace(stats=1, xr=(-1, 1), wr=(-1, 1), nnz=7, cout=(s.cout + 3) // 4 * 4) for s in specs]
    if variant == 'shared_w':   # two descriptors share w (a tower layer over two pyramid levels)
        specs = specs[:1] + [specs[1], specs[7]._replace(salt=0)] + specs[2:7]
        assert specs[1][:3] == specs[2][:3]
    with _deterministic(variant == 'deterministic'):
        _run_forward(specs, share_w=variant == 'shared_w')


@pytest.mark.parametrize('cin', [32, 24, 6])
@pytest.mark.parametrize('k,stride,pad', [(3, 1, 0), (3, 1, 1), (3, 1, 2), (3, 2, 0), (3, 2, 1), (3, 2, 2), (1, 1, 0), (1, 2, 0)])
def test_forward_every_legal_pad(k, stride, pad, cin):
    """Even and odd maps, H != W, on the three kernel families."""
    for H, W in ((8, 5), (7, 10)):
        _run_forward([spec(cin, 40, k, stride, pad, H, 3, W=W)])


@pytest.mark.parametrize('what', ['ksize', 'stride', 'pad', 'n', 'stats'])
def test_forward_refusals_write_nothing(what):
    lib, st = _lib.lib(), _lib.current_stream()
    s = spec(32, 38 if what == 'stats' else 40, 3, 1, 1, 6, 2, stats=0)
    n = 9 if what == 'n' else 1
    descs, outs = _forward_descs([s] * n)
    want = E_UNSUPPORTED
    if what == 'ksize':
        descs[0].ksize = 5
    elif what == 'stride':
        descs[0].stride = 3
    elif what == 'pad':
        descs[0].pad = 3
    elif what == 'n':
        want = E_INVALID
    else:
        stats = _Output(2 * 38 + 2, _stats_prior(38), dtype=np.float64, slack=4)
        descs[0].stats = stats.ptr
    assert lib.ssdk_conv2d_fwd(descs, n, s.B, st) == want, _err()
    assert all(y.untouched() for y, _ in outs)
    if what == 'stats':
        assert stats.untouched()


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd', 'f40', 'group'])
def test_forward_bf16x3_is_bit_equal_on_small_integers(name, monkeypatch):
    """ssdk_conv2d_fwd_fast: integers up to 3 have one bf16 piece, so the three cross terms are the exact products."""
    monkeypatch.setenv('SSDK_FAST_MIN_FLOPS', '0')
    _run_forward(GROUP8 if name == 'group' else [DMA_CASES[name]], entry='fast')
    if name == 'f40':
        _run_forward([CASE_F40._replace(stats=1, xr=(-1, 1), wr=(-1, 1), nnz=9)], entry='fast')


# ---- ssdk_conv2d_bwd ---------------------------------------------------------------------------------------------------------------------

def _exact_backward(s, accumulate_prior=0, shared_rows=None):
    f, g = _forward(s), _backward(s)
    xmax, wmax, gmax = int(np.abs(f['x']).max()), int(np.abs(f['w']).max()), int(np.abs(g['dy']).max())
    rows = s.B * f['ho'] * f['wo'] if shared_rows is None else shared_rows
    if s.nnz or s.dy_nnz:   # sparse operands: the bound is the model on the operands' magnitudes (no partial sum, in any order, exceeds it)
        ax, aw, ab = cr.conv_bwd(np.abs(f['x']), np.abs(f['w']), np.abs(g['dy']), s.stride, s.pad)
        cr.assert_exact(1, int(ax.max()), 1)
        cr.assert_exact(1, int(aw.max()), 1, extra=accumulate_prior)
        cr.assert_exact(1, int(ab.max()), 1, extra=accumulate_prior)
        return
    cr.assert_exact(s.k * s.k * s.cout, gmax, wmax)           # dx
    cr.assert_exact(rows, gmax, xmax, extra=accumulate_prior)  # dw
    cr.assert_exact(rows, gmax, 1, extra=accumulate_prior)     # db


def _run_backward(specs, accumulate=0, want=('dx', 'dw', 'db'), share=None, with_wt=False, fast=False):
    """One grouped ssdk_conv2d_bwd call (ssdk_conv2d_bwd_fast when `fast`); dx, dw, db must equal the model.  share: a group id per
    descriptor -- descriptors with the same id share w, dw and db (summed into it).  with_wt: the weights re-laid out beforehand by
    ssdk_conv2d_transpose_weights.  Returns the bits of every result."""
    lib, st = _lib.lib(), _lib.current_stream()
    n, B = len(specs), specs[0].B
    assert all(s.B == B for s in specs)
    share = list(range(n)) if share is None else share
    descs = (_lib.ConvDesc * n)()
    prior_dw = lambda s: cr.int_pattern((s.cout, s.k, s.k, s.cin), -9, 9, 21)
    prior_db = lambda s: cr.int_pattern((s.cout,), -9, 9, 22)
    groups = {}
    dxs = []
    for i, (d, s) in enumerate(zip(descs, specs)):
        members = [specs[j] for j in range(n) if share[j] == share[i]]
        _exact_backward(s, 9 if accumulate else 0, sum(m.B * _forward(m)['ho'] * _forward(m)['wo'] for m in members))
        f, g = _forward(s), _backward(s)
        d.x, d.hin, d.win, d.cin = _guarded_input(f['x'], _slack(s)), s.H, s.W, s.cin
        d.cout, d.ksize, d.stride, d.pad, d.relu = s.cout, s.k, s.stride, s.pad, 0
        d.dy = _guarded_input(g['dy'], _slack(s))
        if share[i] not in groups:
            assert all(m[:3] == s[:3] and _forward(m)['w'].tobytes() == f['w'].tobytes() for m in members)
            grp = dict(w=_guarded_input(f['w'], _slack(s)),
                       dw=_Output(f['w'].size, prior_dw(s) if accumulate else np.nan) if 'dw' in want else None,
                       db=_Output(s.cout, prior_db(s) if accumulate else np.nan) if 'db' in want else None,
                       want_dw=sum(_backward(m)['dw'] for m in members) + (prior_dw(s) if accumulate else 0),
                       want_db=sum(_backward(m)['db'] for m in members) + (prior_db(s) if accumulate else 0))
            groups[share[i]] = grp
        grp = groups[share[i]]
        d.w = grp['w']
        d.dw = grp['dw'].ptr if grp['dw'] else None
        d.db = grp['db'].ptr if grp['db'] else None
        dx = _Output(f['x'].size) if 'dx' in want else None
        d.dx = dx.ptr if dx else None
        dxs.append(dx)
    if with_wt:
        wts = [_Output(_forward(s)['w'].size) for s in specs]
        ptrs = (C.c_void_p * n)(*[w.ptr for w in wts])
        assert lib.ssdk_conv2d_transpose_weights(descs, n, ptrs, st) == OK, _err()
        for d, s, w in zip(descs, specs, wts):
            assert np.array_equal(w.read(), cr.transposed_weights(_forward(s)['w'], s.stride).ravel()), ('w_t', s)
            d.w_t = w.ptr
    size = (lib.ssdk_conv2d_bwd_fast_workspace_bytes if fast else lib.ssdk_conv2d_bwd_workspace_bytes)(descs, n, B)
    wp, wcheck = _workspace(size)
    if fast:
        rc = lib.ssdk_conv2d_bwd_fast(descs, n, B, accumulate, 3, wp, size, st)
    else:
        rc = lib.ssdk_conv2d_bwd(descs, n, B, accumulate, wp, size, st)
    assert rc == OK, (rc, _err())
    bits = []
    for i, (s, dx) in enumerate(zip(specs, dxs)):
        if dx is not None:
            got = dx.read()
            assert np.array_equal(got, _backward(s)['dx'].ravel()), ('dx of descriptor', i, s, int((got != _backward(s)['dx'].ravel()).sum()), int(np.isnan(got).sum()))
            bits.append(got.view(np.uint32))
    for key, grp in sorted(groups.items()):
        if grp['dw']:
            got = grp['dw'].read()
            assert np.array_equal(got, np.asarray(grp['want_dw'], np.float64).ravel()), ('dw of group', key, int((got != grp['want_dw'].ravel()).sum()), int(np.isnan(got).sum()))
            bits.append(got.view(np.uint32))
        if grp['db']:
            got = grp['db'].read()
            assert np.array_equal(got, np.asarray(grp['want_db'], np.float64).ravel()), ('db of group', key)
            bits.append(got.view(np.uint32))
    wcheck()
    return bits


def _both_modes(specs, **kw):
    """The default mode, then deterministic mode twice with equal bits (the mode is restored whatever happens)."""
    _run_backward(specs, **kw)
    with _deterministic(True):
        a = _run_backward(specs, **kw)
        b = _run_backward(specs, **kw)
    assert len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b)), 'deterministic mode: two runs differ'


# stride-1 data gradients (the forward convolution of dy with the mirrored taps; K = taps x cout, columns = cin):
BWD_S1 = {
    # cout 64: whole 32-channel chunks of dy -> the mirrored LDS-DMA kernel; 3 x 13 x 13 = 507 rows = 4 row tiles, 18 slices < 32: rule
    # "3..8 row tiles" does not apply, fall-through: min(ceil(512 / 8), 18 / 4) = 4 splits
    'cout64_dma': spec(32, 64, 3, 1, 1, 13, 3),
    # cout 40 / cout 4: no whole chunk of dy -> the register-staged mirrored kernel
    'cout40_staged': spec(32, 40, 3, 1, 1, 9, 3, W=6),
    'cout4_staged': spec(36, 4, 3, 1, 1, 9, 3, W=6),
    # a small map whose dx splits K: 2 x 8 x 8 = 128 rows = 1 row tile, 9 x 64 / 32 = 18 slices -> 4 splits into a zero-filled dx
    'small_map_split_k': spec(64, 64, 3, 1, 1, 8, 2),
    # many row tiles, whole K: 4 x 40 x 40 = 6 400 rows = 50 row tiles, 1 column block: 56 workgroups, 9 slices -> min(ceil(512 / 56), 9 / 4) = 2 splits
    'larger_map': spec(32, 32, 3, 1, 1, 40, 4),
    '1x1': spec(64, 96, 1, 1, 0, 10, 3, W=7),
    '1x1_cout36': spec(4, 36, 1, 1, 0, 10, 3, W=7),
    'pad0': spec(32, 64, 3, 1, 0, 9, 3, W=6),
    'pad2': spec(32, 64, 3, 1, 2, 9, 3, W=6),
}
SMALL3 = spec(64, 64, 3, 1, 1, 6, 3)   # 108 rows: as 'small_map_split_k' at the batch of the other cases
# stride-2 data gradients: the scatter form (default mode: T = dy . W as a GEMM whose epilogue adds into a zero-filled dx) and the
# ordered rows-plus-sum form (deterministic mode); every dx element is written, the pixels no tap reaches as zeros
BWD_S2 = {
    'cout64_dma_scatter': spec(32, 64, 3, 2, 1, 9, 3, W=12),
    'cout40_staged_scatter': spec(32, 40, 3, 2, 1, 9, 3, W=12),
    '1x1_even_map': spec(32, 64, 1, 2, 0, 8, 3, W=6),
    '1x1_odd_map': spec(32, 64, 1, 2, 0, 7, 3, W=9),
    '3x3_pad0_odd': spec(32, 32, 3, 2, 0, 9, 3, W=7),
    '3x3_pad0_even': spec(32, 32, 3, 2, 0, 8, 3, W=10),
    '3x3_pad1_even': spec(64, 32, 3, 2, 1, 8, 3, W=10),
    '3x3_pad2_odd': spec(32, 32, 3, 2, 2, 7, 3, W=9),
    '3x3_pad2_even': spec(36, 36, 3, 2, 2, 6, 3, W=8),
}


def check_backward_cases_land_on_their_paths():
    assert _plan_dx(BWD_S1['cout64_dma']) == ('dma mirror one-tile', 1, 4)
    assert _plan_dx(BWD_S1['cout40_staged'])[0] == 'staged<4> mirror' and _plan_dx(BWD_S1['cout4_staged'])[0] == 'staged<4> mirror'
    assert _plan_dx(BWD_S1['small_map_split_k']) == ('dma mirror one-tile', 2, 4)
    assert _plan_dx(BWD_S1['small_map_split_k'], det=True) == ('dma mirror one-tile', 2, 1)
    assert _plan_dx(BWD_S1['larger_map']) == ('dma mirror one-tile', 1, 2)
    assert _plan_dx(BWD_S2['cout64_dma_scatter'])[0] == 'dma scatter one-tile' and _plan_dx(BWD_S2['cout40_staged_scatter'])[0] == 'staged<4> scatter'
    assert _plan_dx(BWD_S2['cout64_dma_scatter'], det=True)[0] == 'dma generic one-tile + strided_dx'
    assert _plan_dx(BWD_S2['cout40_staged_scatter'], det=True)[0] == 'staged<4> generic + strided_dx'
    assert _plan_dx(BWD_S1['cout64_dma'], no_dma=True)[0] == 'staged<4> mirror'


@pytest.mark.parametrize('name', sorted(BWD_S1))
def test_backward_stride_1(name):
    _both_modes([BWD_S1[name]])


@pytest.mark.parametrize('name', sorted(BWD_S2))
def test_backward_stride_2(name):
    _both_modes([BWD_S2[name]])


@pytest.mark.parametrize('name', ['cout64_dma', 'small_map_split_k', '1x1'])
def test_backward_stride_1_register_staged_and_plain_weight_gradient(name, monkeypatch):
    """SSDK_CONV_NO_DMA: the mirrored register-staged kernel on shapes the LDS-DMA kernel normally takes, and igemm_wgrad_kernel."""
    monkeypatch.setenv('SSDK_CONV_NO_DMA', '1')
    _both_modes([BWD_S1[name]])


# weight gradients.  K = the B * Ho * Wo rows in slices of 32; one problem: the per-problem rule (size_wgrad_splits); groups: the
# launch-wide rule (size_wgrad_group)
WGRAD_ONE = {
    # 3 x 24 x 24 = 1 728 rows = 54 slices; 9 taps x 1 x 1 tiles -> narrowed to ... splits = min(ceil(256 / tiles), 27)
    'one_problem': spec(32, 64, 3, 1, 1, 24, 3),
    'rows_fewer_than_32': spec(32, 64, 3, 1, 1, 3, 2, W=5),       # 30 rows: one partly filled slice, one split
    'one_row': spec(64, 32, 3, 2, 1, 1, 1),                        # a single output pixel
    'cin4_cout36': spec(4, 36, 3, 1, 1, 7, 3),
    'cin36_cout4': spec(36, 4, 3, 2, 1, 7, 3),
    'cin36_cout36_1x1': spec(36, 36, 1, 1, 0, 9, 3, W=5),
    'rows_not_a_multiple_of_32': spec(64, 128, 1, 1, 0, 5, 3),    # 75 rows
    'cout_above_128': spec(32, 160, 1, 1, 0, 9, 3),               # two 128-row tiles of dy columns, the second partly filled
    'cin_above_128': spec(160, 32, 3, 1, 1, 6, 3),
}
# tests/test_tail_gemms_gpu.py EDGE_GROUPS['last_split_without_rows']: 5 x 24 x 24 = 2 880 rows = 90 slices beside a small problem: 11
# chains of 9 slices would leave the last split without rows
WGRAD_LAST_SPLIT = [spec(64, 128, 1, 1, 0, 24, 5), spec(128, 128, 1, 1, 0, 4, 5)]
WGRAD_GROUP8 = WGRAD_LAST_SPLIT + [spec(64, 64, 3, 2, 1, 7, 5), spec(32, 36, 3, 1, 1, 5, 5, W=3), spec(4, 128, 1, 1, 0, 9, 5), spec(128, 4, 3, 1, 1, 6, 5),
                                   spec(64, 128, 1, 2, 0, 5, 5), spec(36, 64, 3, 2, 0, 9, 5, W=8)]


@pytest.mark.parametrize('name', sorted(WGRAD_ONE))
def test_weight_gradient_one_problem(name):
    _both_modes([WGRAD_ONE[name]], want=('dw', 'db'))


@pytest.mark.parametrize('no_dma', [False, True])
@pytest.mark.parametrize('name', ['group2', 'group8'])
def test_weight_gradient_groups(name, no_dma, monkeypatch):
    """The launch-wide sizing, with the shapes that leave a problem's last K split without rows; the whole group again on
    igemm_wgrad_kernel."""
    if no_dma:
        monkeypatch.setenv('SSDK_CONV_NO_DMA', '1')
    _both_modes(WGRAD_LAST_SPLIT if name == 'group2' else WGRAD_GROUP8)


@pytest.mark.parametrize('name,s', [('rows_fewer_than_64', spec(32, 40, 1, 1, 0, 3, 2, W=5)),        # 30 rows: one workgroup, partly filled
                                    ('rows_above_64x256', spec(4, 8, 1, 1, 0, 150, 2)),              # 45 000 rows: 176 rows per workgroup
                                    ('rows_above_64x256_wide', spec(4, 132, 1, 1, 0, 140, 1, W=130))])  # 18 200 rows of 132 columns
def test_bias_gradient(name, s):
    _both_modes([s], want=('db',))
    _both_modes([s], want=('db',), accumulate=1)


@pytest.mark.parametrize('skip', ['dx', 'dw', 'db'])
@pytest.mark.parametrize('name', ['s1', 's2'])
def test_backward_with_one_output_null(name, skip):
    s = BWD_S1['cout64_dma'] if name == 's1' else BWD_S2['cout64_dma_scatter']
    _both_modes([s, BWD_S1['cout40_staged']], want=tuple(k for k in ('dx', 'dw', 'db') if k != skip))


@pytest.mark.parametrize('name', ['s1', 's2', 'group8'])
def test_backward_accumulates_into_integers(name):
    """accumulate = 1 over integers (accumulate = 0 over NaN is every other test)."""
    specs = {'s1': [BWD_S1['cout64_dma']], 's2': [BWD_S2['cout64_dma_scatter']], 'group8': WGRAD_GROUP8}[name]
    _both_modes(specs, accumulate=1)


@pytest.mark.parametrize('accumulate', [0, 1])
def test_backward_three_descriptors_share_dw_and_db(accumulate):
    """A tower layer over maps of three sizes: one w, one dw, one db, each dx its own."""
    specs = [spec(32, 64, 3, 1, 1, 9, 3), spec(32, 64, 3, 1, 1, 5, 3, W=7), spec(32, 64, 3, 1, 1, 2, 3, W=3), spec(64, 32, 1, 1, 0, 4, 3)]
    _both_modes(specs, accumulate=accumulate, share=[0, 0, 0, 1])


@pytest.mark.parametrize('name', ['s1', 's2', 'mixed'])
def test_backward_with_weights_laid_out_beforehand_gives_the_same_bits(name):
    specs = {'s1': [BWD_S1['cout64_dma'], BWD_S1['cout4_staged']], 's2': [BWD_S2['cout64_dma_scatter'], BWD_S2['3x3_pad2_even']],
             'mixed': [SMALL3, BWD_S2['cout40_staged_scatter'], BWD_S1['1x1'], BWD_S2['1x1_odd_map']]}[name]
    for det in (False, True):
        with _deterministic(det):
            a = _run_backward(specs, with_wt=True)
            b = _run_backward(specs, with_wt=False)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('stride', [1, 2])
def test_transpose_weights_24_jobs_in_one_call(stride):
    """Both kinds, cin and cout in {4, 36, 100} (tiles of 32 x 32: one partly filled tile, one and a bit, three and a bit), 1 x 1 and 3 x 3."""
    lib, st = _lib.lib(), _lib.current_stream()
    shapes = [(ci, co, k) for ci in (4, 36, 100) for co in (4, 36, 100) for k in (1, 3)] + [(32, 64, 3), (64, 32, 1), (100, 4, 3), (4, 100, 3), (36, 36, 3), (33, 31, 3)]
    assert len(shapes) == 24
    descs = (_lib.ConvDesc * 24)()
    ws, outs = [], []
    for i, (d, (ci, co, k)) in enumerate(zip(descs, shapes)):
        w = cr.int_pattern((co, k, k, ci), -1000, 1000, i)
        ws.append(w)
        d.w, d.cin, d.cout, d.ksize, d.stride = _guarded_input(w, 0), ci, co, k, stride
        outs.append(_Output(w.size))
    ptrs = (C.c_void_p * 24)(*[o.ptr for o in outs])
    assert lib.ssdk_conv2d_transpose_weights(descs, 24, ptrs, st) == OK, _err()
    for i, (w, o) in enumerate(zip(ws, outs)):
        assert np.array_equal(o.read(), cr.transposed_weights(w, stride).ravel()), (i, shapes[i])
    assert lib.ssdk_conv2d_transpose_weights(descs, 25, ptrs, st) == E_INVALID


@pytest.mark.parametrize('name', ['s1', 's1_split', 's2', 'group'])
def test_backward_bf16x3_is_bit_equal_on_small_integers(name, monkeypatch):
    """ssdk_conv2d_bwd_fast (terms = 3): the stride-1 data gradients and every weight gradient on the split-bf16 kernels."""
    monkeypatch.setenv('SSDK_FAST_MIN_FLOPS', '0')
    specs = {'s1': [BWD_S1['cout64_dma']], 's1_split': [SMALL3, BWD_S1['1x1']], 's2': [BWD_S2['cout64_dma_scatter']],
             'group': [s for s in WGRAD_GROUP8 if s.cin % 32 == 0 and s.cout % 32 == 0]}[name]
    _run_backward(specs, fast=True)
    _run_backward(specs, fast=True, accumulate=1)


# ---- wide mantissas: a reduced-precision multiply, which small integers cannot show -------------------------------------------------------

# integers up to 2^11 - 1 (22-bit products), weights with four non-zeros per output channel and gradients with four non-zero rows per
# channel: at most a handful of products per result, every sum below 2^24 (asserted on the magnitudes by _exact_backward)
WIDE = dict(xr=(-2047, 2047), wr=(-2047, 2047), nnz=4, dy_nnz=2, bias=0)
WIDE_CASES = {
    'dma': spec(32, 64, 3, 1, 1, 6, 2, **WIDE),
    'staged_float4': spec(24, 40, 3, 1, 1, 6, 2, **WIDE),
    'scalar': spec(6, 40, 3, 1, 1, 6, 2, **WIDE),
    'scatter_dma': spec(32, 64, 3, 2, 1, 7, 2, **WIDE),
    'scatter_staged': spec(32, 40, 3, 2, 1, 7, 2, **WIDE),
}


@pytest.mark.parametrize('name', sorted(WIDE_CASES))
def test_wide_mantissa_products_are_exact(name, monkeypatch):
    s = WIDE_CASES[name]
    f = _forward(s)
    for a in (f['x'], f['w']):   # 11-bit operands, most of them with more significant bits than bf16 (8) or tf32 (11 with the hidden one) keep exactly
        a = np.abs(a[a != 0])
        assert int(a.max()) > 2000 and np.mean((a & -a) < a // 256) > 0.5
    assert int(np.abs(f['y']).max()) > 2 ** 20   # (a tf32- or bf16-rounded operand would miss these)
    cr.assert_exact(4, 2047, 2047)
    _run_forward([s])
    if s.cin % 4 == 0:
        _both_modes([s])
        monkeypatch.setenv('SSDK_CONV_NO_DMA', '1')   # igemm_wgrad_kernel, the register-staged mirrored and scatter kernels
        _both_modes([s])


# ---- the heads: ssdk_heads_fwd / _ex / _fast, ssdk_heads_bwd / _ex --------------------------------------------------------------------------

Head = collections.namedtuple('Head', 'cin H W types classes loc bias gap')


def head(cin, H, W, types, classes, loc=1, bias=1, gap=0):
    """A pyramid level: `types` anchor types per pixel, n_score = types * classes, n_loc = 4 * types (loc = 0: a single head, which
    carries its anchor-type count in locs_offset); `gap` anchors of nothing behind it in the concatenated rows."""
    return Head(cin, H, W, types, classes, loc, bias, gap)


@functools.lru_cache(maxsize=None)
def _heads_problem(defs, B, density):
    """Operands, layout and exact answers of a heads call (forward and backward); shared, never modified."""
    C_ = defs[0].classes
    assert all(h.classes == C_ for h in defs)
    levels, a_off = [], 0
    for i, h in enumerate(defs):
        ns, nl = h.types * h.classes, 4 * h.types if h.loc else 0
        lv = dict(x=cr.int_pattern((B, h.H, h.W, h.cin), -3, 3, 31 + i), w_score=cr.int_pattern((ns, 3, 3, h.cin), -2, 2, 32 + i),
                  b_score=cr.int_pattern((ns,), -2, 2, 33 + i) if h.bias else None,
                  w_loc=cr.int_pattern((nl, 3, 3, h.cin), -2, 2, 34 + i) if nl else None, b_loc=cr.int_pattern((nl,), -2, 2, 35 + i) if nl and h.bias else None,
                  scores_offset=a_off * C_, locs_offset=a_off * 4, a_off=a_off, anchors=h.H * h.W * h.types, ns=ns, nl=nl)
        cr.assert_exact(9 * h.cin, 3, 2, extra=2)
        a_off += lv['anchors'] + h.gap
        levels.append(lv)
    A = a_off
    out = dict(levels=levels, A=A, sb=A * C_, lb=A * 4, C=C_)
    # forward: the rows as the library must leave them -- sentinel wherever no level lives
    scores, locs = np.full((B, out['sb']), SENTINEL64), np.full((B, out['lb']), SENTINEL64)
    cr.heads_fwd(levels, B, out['sb'], out['lb'], scores, locs)
    out['scores'], out['locs'] = scores, locs
    if density is not None:
        a = np.arange(A, dtype=np.int64)[None, :]
        b = np.arange(B, dtype=np.int64)[:, None]
        keep = np.ones((B, A), bool) if density >= 1.0 else ((b * 7 + a * 13 + (a * a) // 5) % int(round(1 / density)) == 0)
        live = np.zeros((A,), bool)
        for lv in levels:
            live[lv['a_off']:lv['a_off'] + lv['anchors']] = True
        keep = keep & live[None, :]
        ds = np.where(keep[..., None], cr.int_pattern((B, A, C_), -3, 3, 41), 0).astype(np.float64)
        dl = np.where(keep[..., None], cr.int_pattern((B, A, 4), -3, 3, 42), 0).astype(np.float64)
        out['mask'] = keep.astype(np.uint8)
        out['grads'] = cr.heads_bwd(levels, B, ds.reshape(B, -1), dl.reshape(B, -1))
        ds[~np.broadcast_to(live[None, :, None], ds.shape)] = np.nan   # the gaps of the gradient rows: nothing may read them
        dl[~np.broadcast_to(live[None, :, None], dl.shape)] = np.nan
        out['ds'], out['dl'] = ds.reshape(B, -1), dl.reshape(B, -1)
        for h, lv in zip(defs, levels):
            rows = B * h.H * h.W
            cr.assert_exact(9 * (lv['ns'] + lv['nl']), 3, 2)   # dx: both heads' columns in one K chain
            cr.assert_exact(rows, 3, 3)                          # dw
            cr.assert_exact(rows, 3, 1)                          # db
    return out


def _head_array(defs, P, B, with_grads=False):
    arr = (_lib.HeadLevel * len(defs))()
    outs = []
    for d, h, lv in zip(arr, defs, P['levels']):
        slack = 6 * (h.W + 1) * h.cin
        d.x, d.h, d.w, d.cin = _guarded_input(lv['x'], slack), h.H, h.W, h.cin
        d.w_score, d.n_score = _guarded_input(lv['w_score'], slack), lv['ns']
        d.b_score = _guarded_input(lv['b_score'], 0) if h.bias else None
        d.n_loc = lv['nl']
        if lv['nl']:
            d.w_loc = _guarded_input(lv['w_loc'], slack)
            d.b_loc = _guarded_input(lv['b_loc'], 0) if h.bias else None
        d.scores_offset = lv['scores_offset']
        d.locs_offset = lv['locs_offset'] if lv['nl'] else h.types   # a single head: its anchor-type count
        if with_grads:
            o = dict(dx=_Output(lv['x'].size), dw_score=_Output(lv['w_score'].size), db_score=_Output(lv['ns']),
                     dw_loc=_Output(lv['w_loc'].size) if lv['nl'] else None, db_loc=_Output(lv['nl']) if lv['nl'] else None)
            d.dx, d.dw_score, d.db_score = o['dx'].ptr, o['dw_score'].ptr, o['db_score'].ptr
            if lv['nl']:
                d.dw_loc, d.db_loc = o['dw_loc'].ptr, o['db_loc'].ptr
            outs.append(o)
    return arr, outs


def _run_heads_forward(defs, B, entry='fwd', ws=None, max_workgroups=0):
    lib, st = _lib.lib(), _lib.current_stream()
    defs = tuple(defs)
    P = _heads_problem(defs, B, None)
    arr, _ = _head_array(defs, P, B)
    # NaN where a level lives (the call overwrites), the sentinel in the gaps between and behind the levels and around the rows
    scores = _Output(B * P['sb'], np.where(P['scores'] == SENTINEL64, SENTINEL64, np.nan))
    any_loc = any(lv['nl'] for lv in P['levels'])
    locs = _Output(B * P['lb'], np.where(P['locs'] == SENTINEL64, SENTINEL64, np.nan)) if any_loc else None
    lp = C.c_void_p(locs.ptr) if locs else None
    wp, wn = (C.c_void_p(ws[0].data_ptr()), ws[1]) if ws else (None, 0)
    if entry == 'fwd':
        rc = lib.ssdk_heads_fwd(arr, len(defs), B, C.c_void_p(scores.ptr), P['sb'], lp, P['lb'], wp, wn, st)
    elif entry == 'ex':
        rc = lib.ssdk_heads_fwd_ex(arr, len(defs), B, C.c_void_p(scores.ptr), P['sb'], lp, P['lb'], max_workgroups, wp, wn, st)
    else:
        n = lib.ssdk_heads_fwd_fast_workspace_bytes(arr, len(defs))
        fp, fcheck = _workspace(n)
        rc = lib.ssdk_heads_fwd_fast(arr, len(defs), B, C.c_void_p(scores.ptr), P['sb'], lp, P['lb'], 3, fp, n, st)
    assert rc == OK, (rc, _err())
    got = scores.read()
    assert np.array_equal(got, P['scores'].ravel()), ('scores', int((got != P['scores'].ravel()).sum()), int(np.isnan(got).sum()))
    if locs:
        got = locs.read()
        assert np.array_equal(got, P['locs'].ravel()), ('locs', int((got != P['locs'].ravel()).sum()), int(np.isnan(got).sum()))
    if entry == 'fast':
        fcheck()


# two levels with a gap between them and behind them.  Level 0: 4 x 21 = 84 score columns padded to 88, + 16 loc columns = 104: 104 % 32 = 8,
# a half-width last tile; level 1: 6 x 21 = 126 -> 128, + 24 = 152 columns
HEADS_TWO = (head(32, 5, 7, 4, 21, gap=3), head(64, 3, 3, 6, 21, gap=2))
HEADS_SINGLE = (head(32, 5, 7, 4, 21, loc=0, gap=1), head(64, 3, 3, 6, 21, loc=0, gap=2))          # n_loc = 0
HEADS_340 = (head(64, 6, 5, 4, 81, gap=1),)                                                         # 324 + 16 = 340 columns: 11 column tiles, 3 blocks
HEADS_STAGED = (head(24, 5, 7, 4, 21, gap=3), head(40, 3, 3, 6, 21, gap=2))                          # cin 24 / 40: register-staged float4
# batch 1: 1 row tile per level, 8 workgroup slots; 9 x 64 / 32 = 18 slices -> min(ceil(512 / 8), 18 / 4) = 4 splits, 9 slices -> 2 splits:
# the outputs are zero-filled first, levels 0 and 1 as ONE merged segment (they touch), level 2 behind a gap that must stay as it is
HEADS_TINY = (head(64, 4, 4, 4, 21), head(32, 2, 3, 6, 21, gap=5), head(64, 1, 1, 4, 21, gap=2))
# stream-K: cin 64, 340 columns, 63 x 63, batch 4: 15 876 rows = 125 row tiles x 3 column blocks -> 384 workgroups (at most 512: a few
# rounds); units = 125 x 18 x 22 half-tiles = 49 500 -> min(512, 49 500 / 192 / 8 x 8) = 256 persistent workgroups
HEADS_STREAMK = (head(64, 63, 63, 4, 81),)


@pytest.mark.parametrize('name,defs,B', [('two_levels_gaps_half_tile', HEADS_TWO, 3), ('single_heads', HEADS_SINGLE, 3), ('n340', HEADS_340, 3),
                                         ('cin24_staged', HEADS_STAGED, 3), ('tiny_batch_split_k', HEADS_TINY, 1), ('no_bias', tuple(h._replace(bias=0) for h in HEADS_TWO), 2)])
def test_heads_forward(name, defs, B):
    _run_heads_forward(defs, B)
    with _deterministic(True):
        _run_heads_forward(defs, B)


@pytest.mark.parametrize('name,defs,B', [('two_levels_gaps_half_tile', HEADS_TWO, 3), ('tiny_batch_split_k', HEADS_TINY, 1)])
def test_heads_forward_register_staged_and_bf16x3(name, defs, B, monkeypatch):
    _run_heads_forward(defs, B, entry='fast')
    monkeypatch.setenv('SSDK_CONV_NO_DMA', '1')
    _run_heads_forward(defs, B)


@pytest.mark.parametrize('max_workgroups', [None, 0, 256])
def test_heads_forward_stream_k(max_workgroups):
    """With a workspace the launch runs in stream-K form (the flag region shows it, and no wait ran out), through ssdk_heads_fwd and
    through ssdk_heads_fwd_ex with max_workgroups 0 and 256.  (The uncapped launch of this shape already has 256 persistent workgroups,
    the floor of the cap: 256 exercises the argument, not a smaller launch.)"""
    ws = _streamk_workspace()
    _run_heads_forward(HEADS_TWO, 3, entry='fwd', ws=ws)   # (far below 256 workgroups' worth of units: whole tiles)
    flags, timeouts = _streamk_flags(ws[0])
    assert not flags.any() and timeouts == 0
    for _ in range(2):   # (twice on the same workspace: the launch counter moves each time)
        counter = int(flags[-1])
        if max_workgroups is None:
            _run_heads_forward(HEADS_STREAMK, 4, entry='fwd', ws=ws)
        else:
            _run_heads_forward(HEADS_STREAMK, 4, entry='ex', ws=ws, max_workgroups=max_workgroups)
        flags, timeouts = _streamk_flags(ws[0])
        assert int(flags[-1]) not in (0, counter) and timeouts == 0, 'the stream-K form did not run'
        assert not flags[:-1].any(), 'a consumed ready flag was left up'
    assert _timeouts(*ws) == 0 and _lib.lib().ssdk_streamk_poisoned() == 0


def _run_heads_backward(defs, B, density, use_mask):
    lib, st = _lib.lib(), _lib.current_stream()
    defs = tuple(defs)
    P = _heads_problem(defs, B, density)
    arr, outs = _head_array(defs, P, B, with_grads=True)
    ds = _guarded_input(P['ds'], PAGE)
    dl = _guarded_input(P['dl'], PAGE) if any(lv['nl'] for lv in P['levels']) else None
    size = lib.ssdk_heads_bwd_workspace_bytes(arr, len(defs), B)
    wp, wcheck = _workspace(size)
    if use_mask:
        mask = _keep(torch.from_numpy(P['mask']).cuda())
        rc = lib.ssdk_heads_bwd_ex(arr, len(defs), B, ds, P['sb'], dl, P['lb'], C.c_void_p(mask.data_ptr()), P['A'], 0, wp, size, st)
    else:
        rc = lib.ssdk_heads_bwd(arr, len(defs), B, ds, P['sb'], dl, P['lb'], wp, size, st)
    assert rc == OK, (rc, _err())
    bits = []
    for i, (o, want) in enumerate(zip(outs, P['grads'])):
        for key in ('dx', 'dw_score', 'db_score', 'dw_loc', 'db_loc'):
            if o[key] is None:
                continue
            got = o[key].read()
            assert np.array_equal(got, want[key].ravel()), (key, 'of level', i, int((got != want[key].ravel()).sum()), int(np.isnan(got).sum()))
            bits.append(got.view(np.uint32))
    wcheck()
    return bits


def _heads_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv('SSDK_HEADS_BWD_MODE', raising=False)
    else:
        monkeypatch.setenv('SSDK_HEADS_BWD_MODE', mode)


@pytest.mark.parametrize('use_mask', [False, True])
@pytest.mark.parametrize('density', [1.0, 0.05])
@pytest.mark.parametrize('mode', [None, '0', '1', '2'])
def test_heads_backward_two_levels(mode, density, use_mask, monkeypatch):
    """Integer dscores / dlocs, dense and with one anchor in twenty carrying a gradient, in every form SSDK_HEADS_BWD_MODE selects (unset:
    by density on the device; 0 dense, 1 pixel rows -- the legacy pipeline --, 2 anchor rows), with the rows' gaps NaN, with and without
    a truthful row mask: dx, dw_score, dw_loc, db_score, db_loc all exact."""
    _heads_mode(monkeypatch, mode)
    _run_heads_backward(HEADS_TWO, 3, density, use_mask)
    with _deterministic(True):
        a = _run_heads_backward(HEADS_TWO, 3, density, use_mask)
        b = _run_heads_backward(HEADS_TWO, 3, density, use_mask)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('use_mask', [False, True])
@pytest.mark.parametrize('density', [1.0, 0.05])
@pytest.mark.parametrize('mode', [None, '0', '1', '2'])
def test_heads_backward_single_head_levels(mode, density, use_mask, monkeypatch):
    """Levels that are a single head, their anchor-type count in locs_offset."""
    _heads_mode(monkeypatch, mode)
    _run_heads_backward(HEADS_SINGLE, 3, density, use_mask)


@pytest.mark.parametrize('name,defs,B', [('n340', HEADS_340, 3), ('cin24_legacy_pipeline', HEADS_STAGED, 3), ('tiny', HEADS_TINY, 1),
                                         ('larger_map', (head(32, 19, 17, 4, 21, gap=1), head(64, 10, 10, 6, 21)), 2)])
@pytest.mark.parametrize('density', [1.0, 0.05])
def test_heads_backward_other_shapes(name, defs, B, density, monkeypatch):
    _heads_mode(monkeypatch, None)
    _run_heads_backward(defs, B, density, True)
    _run_heads_backward(defs, B, density, False)
