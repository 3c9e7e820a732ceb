"""The float64 model of tests/conv_reference.py against torch.nn.functional.conv2d in float64 (forward and autograd), its weight
re-layout against a plain loop, and the stated properties of int_pattern / assert_exact.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_reference as cr


def _torch_conv(x, w, bias, dy, stride, pad):
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).requires_grad_(True)
    wt = torch.from_numpy(np.ascontiguousarray(w.transpose(0, 3, 1, 2))).requires_grad_(True)
    bt = torch.from_numpy(bias).requires_grad_(True)
    y = F.conv2d(xt, wt, bt, stride=stride, padding=pad)
    (y * torch.from_numpy(np.ascontiguousarray(dy.transpose(0, 3, 1, 2)))).sum().backward()
    nhwc = lambda t: t.detach().numpy().transpose(0, 2, 3, 1)
    return nhwc(y), nhwc(xt.grad), nhwc(wt.grad), bt.grad.numpy()


CASES = [(k, s, p, h, w_) for k in (1, 3) for s in (1, 2) for p in range(k) for (h, w_) in ((5, 8), (6, 7), (4, 4), (7, 3))]


@pytest.mark.parametrize('k,stride,pad,H,W', CASES)
def test_model_equals_torch_float64(k, stride, pad, H, W):
    rng = np.random.default_rng(k * 100 + stride * 10 + pad)
    B, cin, cout = 2, 5, 3
    ho, wo = cr.out_dim(H, k, stride, pad), cr.out_dim(W, k, stride, pad)
    x = rng.standard_normal((B, H, W, cin))
    w = rng.standard_normal((cout, k, k, cin))
    bias = rng.standard_normal(cout)
    dy = rng.standard_normal((B, ho, wo, cout))
    y, dx, dw, db = _torch_conv(x, w, bias, dy, stride, pad)
    np.testing.assert_allclose(cr.conv_fwd(x, w, bias, stride, pad, 0), y, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(cr.conv_fwd(x, w, bias, stride, pad, 1), np.maximum(y, 0), rtol=1e-12, atol=1e-12)
    gdx, gdw, gdb = cr.conv_bwd(x, w, dy, stride, pad)
    np.testing.assert_allclose(gdx, dx, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gdw, dw, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gdb, db, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('k,stride,pad,H,W', CASES)
def test_model_equals_torch_exactly_on_integers(k, stride, pad, H, W):
    """With integer operands both float64 computations are exact: equality, whatever the order of the sums."""
    B, cin, cout = 2, 6, 4
    ho, wo = cr.out_dim(H, k, stride, pad), cr.out_dim(W, k, stride, pad)
    x = cr.int_pattern((B, H, W, cin), -3, 3, 1).astype(np.float64)
    w = cr.int_pattern((cout, k, k, cin), -2, 2, 2).astype(np.float64)
    bias = cr.int_pattern((cout,), -2, 2, 3).astype(np.float64)
    dy = cr.int_pattern((B, ho, wo, cout), -3, 3, 4).astype(np.float64)
    y, dx, dw, db = _torch_conv(x, w, bias, dy, stride, pad)
    assert np.array_equal(cr.conv_fwd(x, w, bias, stride, pad), y)
    gdx, gdw, gdb = cr.conv_bwd(x, w, dy, stride, pad)
    assert np.array_equal(gdx, dx) and np.array_equal(gdw, dw) and np.array_equal(gdb, db)
    s = cr.stats(y)
    assert s.shape == (2 * cout + 2,) and s[2 * cout] == B * ho * wo and s[2 * cout + 1] == 0
    assert np.array_equal(s[:cout], y.sum(axis=(0, 1, 2))) and np.array_equal(s[cout:2 * cout], (y * y).sum(axis=(0, 1, 2)))


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('cout,k,cin', [(3, 3, 5), (4, 1, 2), (36, 3, 4)])
def test_transposed_weights_equal_a_plain_loop(cout, k, cin, stride):
    w = cr.int_pattern((cout, k, k, cin), -50, 50, 7)
    got = cr.transposed_weights(w, stride)
    want = np.zeros((cin, k * k, cout) if stride == 1 else (k * k, cin, cout), w.dtype)
    for n in range(cout):
        for ky in range(k):
            for kx in range(k):
                for c in range(cin):
                    if stride == 1:
                        want[c, ky * k + kx, n] = w[n, ky, kx, c]
                    else:
                        want[ky * k + kx, c, n] = w[n, ky, kx, c]
    assert got.shape == want.shape and got.flags['C_CONTIGUOUS'] and np.array_equal(got, want)


def test_heads_model_is_the_concatenation_of_its_convolutions():
    B = 2
    lv = []
    so = lo = 0
    for (h, w_, cin, ns, nl, gap) in ((3, 4, 4, 6, 8, 5), (2, 2, 8, 3, 0, 2)):
        d = dict(x=cr.int_pattern((B, h, w_, cin), -3, 3, 1), w_score=cr.int_pattern((ns, 3, 3, cin), -2, 2, 2), b_score=cr.int_pattern((ns,), -2, 2, 3),
                 w_loc=cr.int_pattern((nl, 3, 3, cin), -2, 2, 4) if nl else None, b_loc=None, scores_offset=so, locs_offset=lo)
        so += h * w_ * ns + gap
        lo += h * w_ * nl + gap
        lv.append(d)
    scores, locs = np.full((B, so), -7.0), np.full((B, lo), -7.0)
    cr.heads_fwd(lv, B, so, lo, scores, locs)
    y0 = cr.conv_fwd(lv[0]['x'], lv[0]['w_score'], lv[0]['b_score'], 1, 1)
    assert np.array_equal(scores[:, :72], y0.reshape(B, -1)) and (scores[:, 72:77] == -7).all() and (scores[:, 89:] == -7).all()
    assert np.array_equal(locs[:, :96], cr.conv_fwd(lv[0]['x'], lv[0]['w_loc'], None, 1, 1).reshape(B, -1)) and (locs[:, 96:] == -7).all()
    ds, dl = cr.int_pattern((B, so), -3, 3, 5), cr.int_pattern((B, lo), -3, 3, 6)
    g = cr.heads_bwd(lv, B, ds, dl)
    dxs, dws, dbs = cr.conv_bwd(lv[0]['x'], lv[0]['w_score'], ds[:, :72].reshape(B, 3, 4, 6), 1, 1)
    dxl, dwl, dbl = cr.conv_bwd(lv[0]['x'], lv[0]['w_loc'], dl[:, :96].reshape(B, 3, 4, 8), 1, 1)
    assert np.array_equal(g[0]['dx'], dxs + dxl) and np.array_equal(g[0]['dw_score'], dws) and np.array_equal(g[0]['dw_loc'], dwl)
    assert np.array_equal(g[0]['db_score'], dbs) and np.array_equal(g[0]['db_loc'], dbl)
    assert g[1]['dw_loc'] is None and g[1]['db_loc'] is None
    assert np.array_equal(g[1]['dx'], cr.conv_bwd(lv[1]['x'], lv[1]['w_score'], ds[:, 77:89].reshape(B, 2, 2, 3), 1, 1)[0])


def test_int_pattern_is_deterministic_in_range_and_differs_along_every_axis():
    a = cr.int_pattern((4, 3, 3, 8), -3, 3, 5)
    assert a.dtype == np.int64 and np.array_equal(a, cr.int_pattern((4, 3, 3, 8), -3, 3, 5))
    assert a.min() == -3 and a.max() == 3
    assert not np.array_equal(a, cr.int_pattern((4, 3, 3, 8), -3, 3, 6))
    for ax in range(a.ndim):   # no two slices along an axis are equal: swapping, dropping or doubling one changes a sum over the others
        sl = [np.take(a, i, axis=ax) for i in range(a.shape[ax])]
        for i in range(len(sl)):
            for j in range(i + 1, len(sl)):
                assert not np.array_equal(sl[i], sl[j]), (ax, i, j)
    big = cr.int_pattern((5, 9, 7, 32), -2, 2, 1)
    assert set(np.unique(big)) == {-2, -1, 0, 1, 2}


@pytest.mark.parametrize('lo,hi', [(-2, 2), (-1, 1), (-2047, 2047)])
def test_int_pattern_has_no_tap_or_transpose_symmetry(lo, hi):
    w = cr.int_pattern((8, 3, 3, 32), lo, hi, 2)
    assert not np.array_equal(w, w[:, ::-1, ::-1, :])     # mirrored taps
    assert not np.array_equal(w, w[:, ::-1, :, :]) and not np.array_equal(w, w[:, :, ::-1, :])
    assert not np.array_equal(w, w.transpose(0, 2, 1, 3))  # x / y exchanged
    x = cr.int_pattern((2, 6, 6, 4), lo, hi, 3)
    assert not np.array_equal(x, x.transpose(0, 2, 1, 3)) and not np.array_equal(x, x[:, ::-1, ::-1, :])
    # ... and the sums the kernels form see it: a convolution with the mirrored or transposed kernel differs
    xs = cr.int_pattern((1, 6, 6, 32), -3, 3, 1)
    y = cr.conv_fwd(xs, w, None, 1, 1)
    assert not np.array_equal(y, cr.conv_fwd(xs, w[:, ::-1, ::-1, :], None, 1, 1))
    assert not np.array_equal(y, cr.conv_fwd(xs, w.transpose(0, 2, 1, 3), None, 1, 1))


def test_assert_exact_accepts_what_fp32_holds_and_refuses_the_rest():
    assert cr.assert_exact(9 * 512, 3, 2) == 27648
    assert cr.assert_exact(4, 2047, 2047) == 4 * 2047 * 2047 < 2 ** 24
    cr.assert_exact(1, 4095, 4095, extra=2 ** 24 - 4095 * 4095 - 1)   # the largest sum that passes
    with pytest.raises(AssertionError):
        cr.assert_exact(1, 4095, 4095, extra=2 ** 24 - 4095 * 4095)
    with pytest.raises(AssertionError):
        cr.assert_exact(5, 2047, 2047)          # a fifth wide-mantissa product
    with pytest.raises(AssertionError):
        cr.assert_exact(9 * 512, 64, 64)
    # the condition is sharp: 2^24 + 1 is the first integer fp32 cannot hold
    assert np.float32(2 ** 24) + np.float32(1) == np.float32(2 ** 24)
    assert np.float32(2 ** 24 - 1) + np.float32(1) == np.float32(2 ** 24)


def test_exact_gpu_cases_land_on_the_paths_their_comments_derive():
    """The arithmetic in the comments of tests/test_conv_exact_gpu.py, against the dispatch rules of the built library
    (ssdk_debug_conv2d_plan: pure host arithmetic, it belongs to the suite that runs without a GPU)."""
    import test_conv_exact_gpu as exact
    exact.check_forward_cases_land_on_their_paths()
    exact.check_backward_cases_land_on_their_paths()


_CIN = (3, 6, 24, 32, 64, 128, 256, 512, 1024)
_COUT = (4, 32, 36, 40, 48, 64, 104, 256, 512)
_KSP = ((1, 1, 0), (3, 1, 1), (3, 2, 1))
_HS = (1, 2, 3, 5, 8, 9, 10, 19, 20, 32, 38, 64, 129)
_BS = (1, 2, 4, 8, 32)


@pytest.mark.parametrize('direction', [0, 1])
@pytest.mark.parametrize('count', [1, 3, 8])
def test_launch_plans_are_well_formed(count, direction):
    """Grouped requests through ssdk_debug_conv2d_plan (host only): in every planned launch the problems' block ranges are disjoint and
    tile the grid, lie in non-increasing order of work per workgroup (problem_block_work of csrc/conv_plan.h), K is split only where
    nothing forbids it (deterministic mode, a fused ReLU; the third reason, a tile list, exists in the heads' backward only) and the
    half-width last tile is set only where the column space ends in 1..16 columns."""
    import test_conv_exact_gpu as exact
    cdiv = lambda a, b: -(-a // b)
    rng = np.random.RandomState(17 * count + direction)
    pick = lambda seq: seq[rng.randint(len(seq))]
    cins = [c for c in _CIN if direction == 0 or c % 4 == 0]
    for trial in range(48):
        B, det, with_ws = pick(_BS), bool(trial & 1), bool(trial & 2)
        specs = []
        for _ in range(count):
            k, stride, pad = pick(_KSP)
            specs.append(exact.spec(pick(cins), pick(_COUT), k, stride, pad, pick(_HS), B, relu=int(rng.randint(2)), stats=int(rng.randint(2))))
        launches = exact._planned(specs, direction, with_ws=with_ws, det=det)
        assert sum(l.count for l in launches) == count and sorted(d for l in launches for d in l.desc[:l.count]) == list(range(count))
        for l in launches:
            kernel = l.kernel.decode()
            work, ranges = {}, []
            for i in range(l.count):
                s = specs[l.desc[i]]
                if direction == 0:
                    Cc, N, taps = s.cin, s.cout, s.k * s.k
                elif s.stride == 1:
                    Cc, N, taps = s.cout, s.cin, s.k * s.k
                else:   # scatter: the taps are columns; ordered rows: a 1 x 1 GEMM
                    Cc, N, taps = s.cout, s.k * s.k * s.cin, (1 if 'strided_dx' in kernel else s.k * s.k)
                tiles_n = cdiv(N, 32)
                assert 1 <= l.n_blocks[i] <= tiles_n and l.k_splits[i] >= 1, (specs, kernel, i)
                if det or (direction == 0 and s.relu) or 'streamk' in kernel:
                    assert l.k_splits[i] == 1, (specs, kernel, i)
                if l.half_last[i]:
                    assert 1 <= N % 32 <= 16, (specs, kernel, i)
                ranges.append((l.block_begin[i], l.blocks[i]))
                work[l.block_begin[i]] = taps * cdiv(Cc, 32) * cdiv(tiles_n, l.n_blocks[i]) // l.k_splits[i]
            ranges.sort()
            end = 0
            for begin, blocks in ranges:
                assert begin == end and blocks > 0, (specs, kernel, ranges)
                end += blocks
            assert end == l.grid or 'streamk' in kernel, (specs, kernel, ranges, l.grid)
            in_order = [work[b] for b, _ in ranges]
            assert in_order == sorted(in_order, reverse=True), (specs, kernel, in_order)
