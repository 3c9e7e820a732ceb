"""The float64 model of tests/conv_reference.py against torch.nn.functional.conv2d in float64 (forward and autograd), its weight
re-layout against a plain loop, the stated properties of int_pattern / assert_exact, the three-term (split-bf16) form of the model, and
the conditions on the operands of every case of tests/test_conv_fast_exact_gpu.py.  CPU only."""
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


# ---- the three-term (split-bf16) model and the operands of tests/test_conv_fast_exact_gpu.py --------------------------------------------------

def test_bf16_split_is_exact_with_two_integer_pieces_below_2_to_the_16():
    v = np.arange(-(2 ** 16) + 1, 2 ** 16, dtype=np.int64)
    h, m, rest = cr.bf16_split(v)
    assert h.dtype == np.int64 and np.array_equal(h + m, v) and not rest.any()
    pieces = lambda n: tuple(int(p[0]) for p in cr.bf16_split(np.array([n], np.int64)))
    assert pieces(257) == (256, 1, 0) and pieces(259) == (260, -1, 0) and pieces(385) == (384, 1, 0) and pieces(514) == (512, 2, 0)
    assert pieces(-259) == (-260, 1, 0) and pieces(3) == (3, 0, 0)
    odd = v[(np.abs(v) >= 257) & (np.abs(v) <= 511) & (v % 2 != 0)]
    assert (np.abs(cr.bf16_split(odd)[1]) == 1).all()
    wide = v[(np.abs(v) >= 513) & (np.abs(v) <= 1023)]
    assert np.abs(cr.bf16_split(wide)[1]).max() == 2
    # rounding to nearest even against truncation: another h for a quarter of the integers in 257..511
    r = np.arange(257, 512, dtype=np.int64)
    assert abs(np.mean(cr.bf16_truncated(r) != cr.bf16_split(r)[0]) - 0.25) < 0.01


def test_bf16_split_drops_a_third_piece_from_2_to_the_17():
    """2^16 + 2^8 + 1 still has two pieces (bf16 steps by 512 there: it rounds UP to 66 048, and -255 fits a bf16); the smallest
    integers with a third piece lie above 2^17, where the step is 1 024 -- the GPU tests' 2^17 + 2^8 + 1 is one."""
    assert tuple(int(p[0]) for p in cr.bf16_split(np.array([65793], np.int64))) == (66048, -255, 0)
    v = np.arange(-(2 ** 17), 2 ** 17 + 1, dtype=np.int64)
    assert not cr.bf16_split(v)[2].any()
    import test_conv_fast_exact_gpu as fast
    assert fast.THIRD == 131329 and tuple(int(p[0]) for p in cr.bf16_split(np.array([fast.THIRD], np.int64))) == (131072, 256, 1)
    assert tuple(int(p[0]) for p in cr.bf16_split(np.array([-fast.THIRD], np.int64))) == (-131072, -256, -1)


def test_two_piece_pattern_has_mid_pieces_everywhere():
    for lo, hi in ((257, 1023), (257, 511), (257, 287)):
        a = cr.two_piece_pattern((3, 5, 7, 32), 4, lo, hi)
        h, m, rest = cr.bf16_split(a)
        assert np.abs(a).min() >= lo and np.abs(a).max() <= hi and (m != 0).all() and not rest.any()
        assert 0.3 < np.mean(a > 0) < 0.7 and np.mean(cr.bf16_truncated(a) != h) > 0.2
    s = cr.two_piece_pattern((3, 5, 7, 32), 4, density=0.1)
    assert 0.05 < np.mean(s != 0) < 0.2


@pytest.mark.parametrize('k,stride,pad', [(3, 1, 1), (3, 2, 1), (1, 1, 0), (3, 2, 0)])
def test_three_term_model_is_the_sum_of_its_terms_and_the_exact_model_without_mid_pieces(k, stride, pad):
    B, H, W, cin, cout = 2, 6, 5, 8, 4
    ho, wo = cr.out_dim(H, k, stride, pad), cr.out_dim(W, k, stride, pad)
    x, w, dy = cr.two_piece_pattern((B, H, W, cin), 1), cr.two_piece_pattern((cout, k, k, cin), 2), cr.two_piece_pattern((B, ho, wo, cout), 3)
    bias = cr.int_pattern((cout,), -2, 2, 3)
    (hx, mx, _), (hw_, mw, _), (hy, my, _) = cr.bf16_split(x), cr.bf16_split(w), cr.bf16_split(dy)
    # sum(a b) - sum(m_a m_b), GEMM by GEMM
    y3 = cr.conv_fwd(x, w, bias, stride, pad, 0, 'split3')
    assert np.array_equal(y3, cr.conv_fwd(x, w, bias, stride, pad) - cr.conv_fwd(mx, mw, None, stride, pad))
    assert not np.array_equal(y3, cr.conv_fwd(x, w, bias, stride, pad))
    assert np.array_equal(cr.conv_fwd(x, w, bias, stride, pad, 1, 'split3'), np.maximum(y3, 0))
    dx3, dw3, db3 = cr.conv_bwd(x, w, dy, stride, pad, ('split3', 'split3'))
    dx, dw, db = cr.conv_bwd(x, w, dy, stride, pad)
    assert np.array_equal(dx3, dx - cr.conv_bwd(x, mw, my, stride, pad)[0]) and np.array_equal(dw3, dw - cr.conv_bwd(mx, w, my, stride, pad)[1])
    assert np.array_equal(db3, db)
    mixed = cr.conv_bwd(x, w, dy, stride, pad, ('exact', 'split3'))
    assert np.array_equal(mixed[0], dx) and np.array_equal(mixed[1], dw3)
    # every m forced to 0 (operands that are their own h): the existing exact model
    assert np.array_equal(cr.conv_fwd(hx, hw_, bias, stride, pad, 0, 'split3'), cr.conv_fwd(hx, hw_, bias, stride, pad))
    for a, b in zip(cr.conv_bwd(hx, hw_, hy, stride, pad, ('split3', 'split3')), cr.conv_bwd(hx, hw_, hy, stride, pad)):
        assert np.array_equal(a, b)
    # the magnitudes bound every term group
    assert (cr.conv_fwd(x, w, bias, stride, pad, 0, 'split3', mag=True) >= np.abs(y3)).all()
    assert cr.assert_exact_model([np.array([5.0, 2 ** 24 - 2]), None], extra=1) == 2 ** 24 - 1
    with pytest.raises(AssertionError):
        cr.assert_exact_model(np.array([2.0 ** 24 - 1]), extra=1)


def test_three_term_heads_model_takes_an_arithmetic_per_level_and_equals_the_exact_one_without_mid_pieces():
    import test_conv_fast_exact_gpu as fast
    defs, B = fast.HEADS_BWD['two']
    one = fast.heads_backward_case(defs, B, 'a2', 1.0, ('split3', 'split3'))   # dy two-piece, x and w one-piece: equal to the exact model
    for g, e in zip(one['grads'], one['grads_exact']):
        assert all(np.array_equal(g[k], e[k]) for k in g)
    P = fast.heads_backward_case(defs, B, 'both', 1.0, ('exact', 'split3'))
    ds, dl = np.nan_to_num(P['ds']), np.nan_to_num(P['dl'])
    per_level = cr.heads_bwd(P['levels'], B, ds, dl, [('split3', 'exact'), ('exact', 'split3')])
    assert np.array_equal(per_level[0]['dw_score'], P['grads_exact'][0]['dw_score']) and np.array_equal(per_level[1]['dx'], P['grads_exact'][1]['dx'])
    assert np.array_equal(per_level[1]['dw_loc'], P['grads'][1]['dw_loc']) and not np.array_equal(per_level[0]['dx'], P['grads_exact'][0]['dx'])


def _differing(a, b):
    return float(np.mean(np.asarray(a) != np.asarray(b)))


def _fast_case_ids():
    import test_conv_fast_exact_gpu as fast
    return fast.all_cases()


def _fast_case_name(c):
    word = lambda p: ('x'.join(str(v) for v in p[:8]) if hasattr(p, 'cin') else '+'.join(word(q) for q in p) if isinstance(p, tuple) else str(p))
    return '-'.join(word(p) for p in c)


@pytest.mark.parametrize('case', _fast_case_ids(), ids=_fast_case_name)
def test_fast_exact_gpu_case_meets_the_conditions_on_its_operands(case):
    """For every case of tests/test_conv_fast_exact_gpu.py: the magnitude bound is below 2^24 (asserted while the case is built); a2 / b2:
    every non-zero of the two-piece operand has a mid piece (at least half are asked for) and at least a fifth an h that truncation gets
    wrong; `both`: the three-term answer differs from the exact product on at least half of the elements of every output tensor that is
    three-term (behind a fused ReLU: of the elements it lets through, and it must cut at least a fifth -- the negative sums); `third`: the
    dropped piece shows in every such tensor."""
    import test_conv_fast_exact_gpu as fast
    kind, regime = case[0], case[3] if case[0].startswith('heads') else case[2]
    P = fast.case_of(case)
    assert 0 < P['bound'] < 2 ** 24
    if kind == 'fwd':
        two, pairs = (P['x'] if regime == 'a2' else P['w']), [(P['y'], P['y_exact'], 'split3')]
    elif kind == 'bwd':
        two = P['dy'] if regime == 'a2' else np.concatenate([P['w'].ravel(), P['x'].ravel()])
        pairs = [(P['dx'], P['dx_exact'], P['arith'][0]), (P['dw'], P['dw_exact'], P['arith'][1])]
    elif kind == 'heads_fwd':
        two = np.concatenate([lv['x' if regime == 'a2' else 'w_score'].ravel() for lv in P['levels']])
        pairs = [(P['scores'], P['scores_exact'], 'split3'), (P['locs'], P['locs_exact'], 'split3')]
    else:
        two = np.nan_to_num(P['ds']) if regime == 'a2' else np.concatenate([lv[k].ravel() for lv in P['levels'] for k in ('x', 'w_score')])
        arith = case[5]
        pairs = [(g[k], e[k], arith[0] if k == 'dx' else arith[1]) for g, e in zip(P['grads'], P['grads_exact']) for k in ('dx', 'dw_score', 'dw_loc')
                 if g[k] is not None]
    if regime in ('a2', 'b2'):
        nz = two[two != 0]
        h, m, rest = cr.bf16_split(nz)
        assert nz.size and np.mean(m != 0) >= 0.5 and np.mean(cr.bf16_truncated(nz) != h) >= 0.2 and not rest.any()
        assert all(np.array_equal(a, b) for a, b, _ in pairs)   # one side has no mid piece: sum(a b)
    for got, exact, arith in pairs:
        if arith == 'exact':
            assert np.array_equal(got, exact)
        elif regime == 'both' and kind == 'fwd' and case[1].relu:
            through = (got > 0) | (exact > 0)
            assert np.mean(~through) >= 0.2 and _differing(got[through], exact[through]) >= 0.5
        elif regime == 'both':
            assert _differing(got, exact) >= 0.5, _differing(got, exact)
        elif regime == 'third':
            assert _differing(got, exact) > 0
