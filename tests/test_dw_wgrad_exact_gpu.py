"""GPU: the two atomic weight-gradient kernels of the depthwise family, dw_wgrad_kernel (ssdk_depthwise_conv2d_bwd) and dwup_wgrad_kernel
(ssdk_depthwise_upsample_conv2d_bwd), with their data gradients, on INTEGER operands through the ctypes binding.

x, dy in {-3..3} and w in {-2..2}: every product and every partial sum is an integer, and the test asserts that the model's largest
magnitude stays below 2^24 -- so the fp32 result is exact in ANY summation order, the atomics' included, and is compared bit for bit with
the int64 model of tests/dwgroup_reference.py (weight_grad, data_grad).  Every case runs in both modes of ops.set_deterministic (one chunk
against several).

The shapes are the smallest that reach every index path of the kernels: a second channel block (C = 260: 65 quads, the second block holds
one), two pixel chunks that the four pixel phases share unevenly (300 = 2 x 150 and 350 = 2 x 175 output pixels), 25 taps (= kDwMaxTaps),
stride 2, k 1, a non-integer upsampling ratio, a 1 x 1 coarse map; and the argument forms accumulate = 1, db == NULL, dx / dcoarse == NULL."""
import numpy as np
import pytest

import dwgroup_reference as ref
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

# name: (batch, channels, h, w, ksize, stride, pad)
SINGLE = {
    'c260_k3': (3, 260, 10, 10, 3, 1, 1),        # 65 channel quads; 300 output pixels = two chunks of 150
    'c8_k5_pad1': (2, 8, 7, 5, 5, 1, 1),         # 25 taps = kDwMaxTaps, the map shrinks
    'c8_k5_pad2': (2, 8, 7, 5, 5, 1, 2),
    'c8_k3_stride2': (2, 8, 9, 7, 3, 2, 1),
    'c8_k1': (2, 8, 4, 3, 1, 1, 0),
}
# name: (batch, channels, (hc, wc), (hf, wf))
UPSAMPLED = {
    'c260_5x4_to_10x7': (5, 260, (5, 4), (10, 7)),   # 350 fine pixels = two chunks of 175
    'c8_3x2_to_5x4': (2, 8, (3, 2), (5, 4)),         # a non-integer ratio
    'c8_1x1_to_2x1': (2, 8, (1, 1), (2, 1)),
}
MODES = [False, True]


@pytest.fixture(params=MODES, ids=['atomic', 'deterministic'])
def mode(request):
    from single_shot_detection_amd import ops
    before = ops.set_deterministic(request.param)
    yield request.param
    ops.set_deterministic(before)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(shape):
    import torch
    return torch.full(shape, float('nan'), device='cuda')


def _ptr(t):
    return None if t is None else t.data_ptr()


def _exact(got, want, what, times=1):
    """``got`` (fp32 from the device) holds exactly the integers ``times * want`` (int64); the model itself stays below 2^24."""
    assert int(np.abs(want).max()) * times < 2 ** 24, what
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.astype(np.float64), (times * want).astype(np.float64)), what


_single_cache = {}


def _single(name):
    """Operands and int64 model (dx, dw, db) of a SINGLE case, computed once."""
    if name not in _single_cache:
        B, C, H, W, k, stride, pad = SINGLE[name]
        rng = np.random.default_rng(sorted(SINGLE).index(name))
        x = rng.integers(-3, 4, (B, H, W, C)).astype(np.float32)
        dy = rng.integers(-3, 4, (B, ref.out_dim(H, k, stride, pad), ref.out_dim(W, k, stride, pad), C)).astype(np.float32)
        weight = rng.integers(-2, 3, (C, k, k)).astype(np.float32)
        dx = ref.data_grad([dy], weight, [(H, W)], stride, pad, np.int64)[0]
        dw, db = ref.weight_grad([x], [dy], k, stride, pad, np.int64)
        _single_cache[name] = (x, dy, weight, dx, dw, db)
    return _single_cache[name]


def _run_single(name, want_dx=True, want_db=True, calls=1):
    """ssdk_depthwise_conv2d_bwd into NaN-filled outputs: the first call with accumulate = 0, every further one with accumulate = 1."""
    import torch
    from single_shot_detection_amd import _lib
    lib = _lib.lib()
    B, C, H, W, k, stride, pad = SINGLE[name]
    x, dy, weight = (_dev(a) for a in _single(name)[:3])
    dx = _nan(x.shape) if want_dx else None
    dw = _nan(weight.shape)
    db = _nan((C,)) if want_db else None
    for call in range(calls):
        _lib.check(lib.ssdk_depthwise_conv2d_bwd(x.data_ptr(), weight.data_ptr(), dy.data_ptr(), B, H, W, C, k, stride, pad, _ptr(dx), dw.data_ptr(),
                                                 _ptr(db), 1 if call else 0, _lib.current_stream()), 'ssdk_depthwise_conv2d_bwd')
    torch.cuda.synchronize()
    return dx, dw, db


@pytest.mark.parametrize('name', sorted(SINGLE))
def test_single_map_gradients_equal_the_int64_model(name, mode):
    dx, dw, db = _run_single(name)
    _, _, _, want_dx, want_dw, want_db = _single(name)
    _exact(dx, want_dx, 'dx')
    _exact(dw, want_dw, 'dw')
    _exact(db, want_db, 'db')


@pytest.mark.parametrize('name', ['c260_k3', 'c8_k3_stride2'])
def test_single_map_accumulate_adds_the_second_call(name, mode):
    dx, dw, db = _run_single(name, calls=2)
    _, _, _, want_dx, want_dw, want_db = _single(name)
    _exact(dx, want_dx, 'dx', times=2)
    _exact(dw, want_dw, 'dw', times=2)
    _exact(db, want_db, 'db', times=2)


@pytest.mark.parametrize('name', ['c260_k3', 'c8_k5_pad1'])
def test_single_map_without_db(name, mode):
    dx, dw, db = _run_single(name, want_db=False)
    _, _, _, want_dx, want_dw, _ = _single(name)
    assert db is None
    _exact(dx, want_dx, 'dx')
    _exact(dw, want_dw, 'dw')


@pytest.mark.parametrize('name', ['c260_k3', 'c8_k5_pad1'])
def test_single_map_without_dx(name, mode):
    dx, dw, db = _run_single(name, want_dx=False)
    _, _, _, _, want_dw, want_db = _single(name)
    assert dx is None
    _exact(dw, want_dw, 'dw')
    _exact(db, want_db, 'db')


_up_cache = {}


def _upsampled(name):
    """Operands and model of an UPSAMPLED case: dw / db are weight_grad (int64) of the CPU F.interpolate(mode='nearest') of the coarse map
    with k 3 and pad 1, dcoarse is torch's float64 autograd through interpolate -> conv2d on the same integers."""
    if name not in _up_cache:
        import torch
        import torch.nn.functional as F
        B, C, (hc, wc), (hf, wf) = UPSAMPLED[name]
        rng = np.random.default_rng(100 + sorted(UPSAMPLED).index(name))
        coarse = rng.integers(-3, 4, (B, hc, wc, C)).astype(np.float32)
        dy = rng.integers(-3, 4, (B, hf, wf, C)).astype(np.float32)
        weight = rng.integers(-2, 3, (C, 3, 3)).astype(np.float32)
        up = F.interpolate(torch.from_numpy(coarse).permute(0, 3, 1, 2), size=(hf, wf), mode='nearest').permute(0, 2, 3, 1).numpy()
        dw, db = ref.weight_grad([up], [dy], 3, 1, 1, np.int64)
        c64 = torch.from_numpy(coarse).double().permute(0, 3, 1, 2).requires_grad_(True)
        y = F.conv2d(F.interpolate(c64, size=(hf, wf), mode='nearest'), torch.from_numpy(weight).double()[:, None], padding=1, groups=C)
        y.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
        dcoarse = c64.grad.permute(0, 2, 3, 1).contiguous().numpy()
        assert np.array_equal(dcoarse, np.rint(dcoarse))
        _up_cache[name] = (coarse, dy, weight, dcoarse.astype(np.int64), dw, db)
    return _up_cache[name]


def _run_upsampled(name, want_dcoarse=True, want_db=True):
    import torch
    from single_shot_detection_amd import _lib
    lib = _lib.lib()
    B, C, (hc, wc), (hf, wf) = UPSAMPLED[name]
    coarse, dy, weight = (_dev(a) for a in _upsampled(name)[:3])
    dcoarse = _nan(coarse.shape) if want_dcoarse else None
    dw = _nan(weight.shape)
    db = _nan((C,)) if want_db else None
    _lib.check(lib.ssdk_depthwise_upsample_conv2d_bwd(coarse.data_ptr(), weight.data_ptr(), dy.data_ptr(), B, hc, wc, hf, wf, C, _ptr(dcoarse),
                                                      dw.data_ptr(), _ptr(db), _lib.current_stream()), 'ssdk_depthwise_upsample_conv2d_bwd')
    torch.cuda.synchronize()
    return dcoarse, dw, db


@pytest.mark.parametrize('want_db', [True, False], ids=['db', 'no_db'])
@pytest.mark.parametrize('name', sorted(UPSAMPLED))
def test_upsampled_gradients_equal_the_model(name, want_db, mode):
    dcoarse, dw, db = _run_upsampled(name, want_db=want_db)
    _, _, _, want_dcoarse, want_dw, want_db_model = _upsampled(name)
    _exact(dcoarse, want_dcoarse, 'dcoarse')
    _exact(dw, want_dw, 'dw')
    if want_db:
        _exact(db, want_db_model, 'db')
    else:
        assert db is None


@pytest.mark.parametrize('name', ['c260_5x4_to_10x7', 'c8_3x2_to_5x4'])
def test_upsampled_without_dcoarse(name, mode):
    dcoarse, dw, db = _run_upsampled(name, want_dcoarse=False)
    _, _, _, _, want_dw, want_db = _upsampled(name)
    assert dcoarse is None
    _exact(dw, want_dw, 'dw')
    _exact(db, want_db, 'db')
