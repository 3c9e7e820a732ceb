"""Float64 model of the convolution GEMMs of csrc/conv.hip (numpy only): what ssdk_conv2d_fwd / _bwd, ssdk_conv2d_transpose_weights and
ssdk_heads_fwd / _bwd compute, on NHWC arrays in the layouts include/ssdk.h documents -- x [B, H, W, Cin], w [Cout, k, k, Cin],
y / dy [B, Ho, Wo, Cout].  im2col and one BLAS matmul per image, in float64: for the small-integer operands the exact tests use,
every product and partial sum is an integer far below 2^53, so the result is THE answer, not an approximation of it
(assert_exact states the condition under which the same holds for fp32 on the GPU, in any summation order).
Every model also takes the arithmetic of the opt-in split-bf16 fast mode per GEMM ('split3': the three cross terms of the operands'
bf16 pieces, bf16_split) and can sum magnitudes instead of values (mag=True: the bound assert_exact_model checks).
Pinned against torch.nn.functional.conv2d in float64 by test_conv_reference.py."""
import numpy as np


def out_dim(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _im2col(x, k, stride, pad):
    """x [B, H, W, C] (float64) -> cols [B, Ho * Wo, k * k * C], taps in (ky, kx) order, channel minor: the K order of w.reshape(Cout, -1)."""
    B, H, W, C = x.shape
    ho, wo = out_dim(H, k, stride, pad), out_dim(W, k, stride, pad)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, C), np.float64)
    xp[:, pad:pad + H, pad:pad + W, :] = x
    cols = np.empty((B, ho, wo, k * k, C), np.float64)
    for ky in range(k):
        for kx in range(k):
            cols[:, :, :, ky * k + kx, :] = xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride, :]
    return cols.reshape(B, ho * wo, k * k * C), ho, wo


def _conv_lin(x, w, stride, pad):
    """The bilinear part of conv_fwd: no bias, no ReLU."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    cout, k = w.shape[0], w.shape[1]
    wm = w.reshape(cout, -1).T
    B = x.shape[0]
    ho, wo = out_dim(x.shape[1], k, stride, pad), out_dim(x.shape[2], k, stride, pad)
    y = np.empty((B, ho, wo, cout), np.float64)
    for b in range(B):   # (one image at a time: the im2col matrix of a large map stays small)
        cols, _, _ = _im2col(x[b:b + 1], k, stride, pad)
        y[b] = (cols[0] @ wm).reshape(ho, wo, cout)
    return y


def conv_fwd(x, w, bias=None, stride=1, pad=0, relu=0, arith='exact', mag=False):
    """y [B, Ho, Wo, Cout] as the library stores it: the complete sum (plus bias) is formed first, the ReLU (relu != 0) is applied to it.
    arith: 'exact', or 'split3' = the three bf16 cross terms of the fast mode (x is the A operand, w the B operand).  mag: the same sums
    over the magnitudes of every piece and of the bias, without the ReLU -- the bound of assert_exact_model."""
    y = sum(_conv_lin(a, b, stride, pad) for a, b in _terms(x, w, arith, mag))
    if bias is not None:
        y += np.abs(np.asarray(bias, np.float64)) if mag else np.asarray(bias, np.float64)
    return np.maximum(y, 0.0) if relu and not mag else y


def _conv_bwd_lin(x, w, dy, stride, pad):
    """conv_bwd in the plain arithmetic: dx is bilinear in (dy, w), dw in (dy, x), db linear in dy."""
    x, w, dy = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(dy, np.float64)
    B, H, W, C = x.shape
    cout, k = w.shape[0], w.shape[1]
    wm = w.reshape(cout, -1)
    dw = np.zeros((cout, k * k * C), np.float64)
    dxp = np.zeros((B, H + 2 * pad, W + 2 * pad, C), np.float64)
    for b in range(B):
        cols, ho, wo = _im2col(x[b:b + 1], k, stride, pad)
        g = dy[b].reshape(ho * wo, cout)
        dw += g.T @ cols[0]
        dcols = (g @ wm).reshape(ho, wo, k * k, C)
        for ky in range(k):
            for kx in range(k):
                dxp[b, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride, :] += dcols[:, :, ky * k + kx, :]
    dx = dxp[:, pad:pad + H, pad:pad + W, :].copy()
    return dx, dw.reshape(w.shape), dy.reshape(-1, cout).sum(axis=0)


def conv_bwd(x, w, dy, stride=1, pad=0, arith=('exact', 'exact'), mag=False):
    """(dx like x, dw like w, db [Cout]) for dy = the gradient w.r.t. the convolution's output.  arith = (dx, dw): each GEMM 'exact' or
    'split3' -- dx is the forward form of dy (A) with the mirrored kernel (B = w), dw is dy (A) times x (B); db is a plain sum always.
    mag: the sums over the pieces' magnitudes (see conv_fwd)."""
    x, w, dy = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(dy, np.float64)
    dx = sum(_conv_bwd_lin(np.zeros_like(x), b, a, stride, pad)[0] for a, b in _terms(dy, w, arith[0], mag))
    dw = sum(_conv_bwd_lin(b, np.zeros_like(w), a, stride, pad)[1] for a, b in _terms(dy, x, arith[1], mag))
    return dx, dw, (np.abs(dy) if mag else dy).reshape(-1, w.shape[0]).sum(axis=0)


def stats(y):
    """The [2 * cout + 2] `sums` of ssdk_conv_desc::stats for a stored output y: per-channel sums, sums of squares, the rows, a zero."""
    y = np.asarray(y, np.float64)
    cout = y.shape[-1]
    r = y.reshape(-1, cout)
    return np.concatenate([r.sum(axis=0), (r * r).sum(axis=0), [float(r.shape[0]), 0.0]])


def transposed_weights(w, stride):
    """ssdk_conv2d_transpose_weights: w [cout][tap][cin] -> stride 1: [cin][tap][cout], otherwise [tap][cin][cout]."""
    w = np.asarray(w)
    cout, k, _, cin = w.shape
    w3 = w.reshape(cout, k * k, cin)
    return np.ascontiguousarray(w3.transpose(2, 1, 0) if stride == 1 else w3.transpose(1, 2, 0))


def heads_fwd(levels, batch, scores_batch_stride, locs_batch_stride, scores, locs, arith='exact', mag=False):
    """ssdk_heads_fwd: `levels` is a list of dicts with x [B, H, W, Cin], w_score [n_score, 3, 3, Cin], b_score or None, w_loc
    [n_loc, 3, 3, Cin] or None, b_loc, scores_offset, locs_offset.  Writes element (b, pixel p, channel n) of a level at
    scores[b, scores_offset + p * n_score + n] (locs alike) into the given float64 arrays [B, *_batch_stride] and leaves every other
    element as it was (the gaps of a row).  arith / mag: as conv_fwd, for both heads of every level."""
    for lv in levels:
        B, H, W, _ = lv['x'].shape
        assert B == batch
        ys = conv_fwd(lv['x'], lv['w_score'], lv.get('b_score'), 1, 1, 0, arith, mag).reshape(B, -1)
        assert lv['scores_offset'] + ys.shape[1] <= scores_batch_stride
        scores[:, lv['scores_offset']:lv['scores_offset'] + ys.shape[1]] = ys
        if lv.get('w_loc') is not None:
            yl = conv_fwd(lv['x'], lv['w_loc'], lv.get('b_loc'), 1, 1, 0, arith, mag).reshape(B, -1)
            assert lv['locs_offset'] + yl.shape[1] <= locs_batch_stride
            locs[:, lv['locs_offset']:lv['locs_offset'] + yl.shape[1]] = yl
    return scores, locs


def heads_bwd(levels, batch, dscores, dlocs, arith=('exact', 'exact'), mag=False):
    """ssdk_heads_bwd: per level a dict dx, dw_score, db_score, dw_loc, db_loc (the last three None for a single head) from the gradients
    of the concatenated rows, dscores [B, scores_batch_stride] / dlocs [B, locs_batch_stride]; dx sums both heads.  arith: one (dx, dw)
    pair as conv_bwd takes it, or a list of them, one per level; mag as conv_bwd."""
    out = []
    per_level = [arith] * len(levels) if isinstance(arith[0], str) else list(arith)
    assert len(per_level) == len(levels)
    for lv, ar in zip(levels, per_level):
        B, H, W, _ = lv['x'].shape
        assert B == batch
        ns = lv['w_score'].shape[0]
        gs = np.asarray(dscores, np.float64)[:, lv['scores_offset']:lv['scores_offset'] + H * W * ns].reshape(B, H, W, ns)
        dx, dws, dbs = conv_bwd(lv['x'], lv['w_score'], gs, 1, 1, ar, mag)
        r = dict(dx=dx, dw_score=dws, db_score=dbs, dw_loc=None, db_loc=None)
        if lv.get('w_loc') is not None:
            nl = lv['w_loc'].shape[0]
            gl = np.asarray(dlocs, np.float64)[:, lv['locs_offset']:lv['locs_offset'] + H * W * nl].reshape(B, H, W, nl)
            dx2, r['dw_loc'], r['db_loc'] = conv_bwd(lv['x'], lv['w_loc'], gl, 1, 1, ar, mag)
            r['dx'] = dx + dx2
        out.append(r)
    return out


_COEF = (7, 3, 11, 5, 13, 17)


def int_pattern(shape, lo, hi, salt=0):
    """Deterministic integers in [lo, hi] (int64, of `shape`).  A different linear coefficient per axis plus a quadratic term and a
    product of neighbouring axes: the value sequence differs along every axis (a swapped, dropped or doubled row, tap or channel changes
    a sum), the values are scrambled over the whole range (a wide range gives wide mantissas), and the array is not symmetric under
    a flip of an axis or an exchange of two axes of equal length (the mirrored-tap and tap-major weight layouts, x against y)."""
    shape = tuple(int(s) for s in shape)
    assert hi > lo and len(shape) <= len(_COEF)
    idx = np.indices(shape, dtype=np.int64) if shape else np.zeros((0,), np.int64)
    v = np.full(shape, int(salt), np.int64)
    for a in range(len(shape)):
        i = idx[a]
        v += _COEF[a] * i + (i * i) // (a + 2)
        if a + 1 < len(shape):
            v += (i + 1) * (idx[a + 1] % (a + 3))
    v = v * 2654435761 + v // 7   # (spread over the whole range, whatever its width: neighbours differ in their low AND high bits)
    return v % (hi - lo + 1) + lo


def assert_exact(max_terms, amax, bmax, extra=0):
    """The condition under which an fp32 GEMM is exact in ANY summation order: every partial sum of at most max_terms products of
    integers bounded by amax and bmax (plus what the output already holds or the bias adds, `extra`) stays below 2^24, where fp32
    represents every integer.  Each GPU case asserts it for each of its GEMMs: then the integer reference alone decides the answer."""
    bound = int(max_terms) * int(amax) * int(bmax) + int(extra)
    assert bound < 2 ** 24, f'not exact in fp32: {max_terms} terms x {amax} x {bmax} + {extra} = {bound} >= 2^24'
    return bound


# ---- the split-bf16 fast mode ('bf16x3'): a = h + m (+ rest, dropped), a product is h_a h_b + h_a m_b + m_a h_b -----------------------------

def bf16_split(v):
    """(h, m, rest) of the fast mode's operand split, h = bf16(v), m = bf16(v - h), rest = v - h - m, as float64 arrays (int64 for an integer
    input).  The casts are torch's CPU bfloat16 conversion (round to nearest even): nothing here is shared with the device code."""
    import torch
    a = np.asarray(v)
    f = np.ascontiguousarray(a, np.float64)
    assert np.array_equal(f.astype(np.float32).astype(np.float64), f), 'the operands are fp32 values'
    rne = lambda t: torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    h = rne(f)
    m = rne(f - h)
    rest = f - h - m
    if np.issubdtype(a.dtype, np.integer):
        return h.astype(np.int64), m.astype(np.int64), rest.astype(np.int64)
    return h, m, rest


def bf16_truncated(v):
    """What a split that truncates instead of rounding would take as h: the top 16 bits of the fp32 pattern."""
    f = np.ascontiguousarray(v, np.float32)
    return (f.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


def _terms(a, b, arith, mag=False):
    """The (A piece, B piece) pairs whose bilinear forms add up to one GEMM in arithmetic `arith`; mag: every piece by its magnitude."""
    assert arith in ('exact', 'split3'), arith
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if arith == 'exact':
        pairs = [(a, b)]
    else:
        (ha, ma, _), (hb, mb, _) = bf16_split(a), bf16_split(b)
        pairs = [(ha, hb), (ha, mb), (ma, hb)]
    return [(np.abs(p), np.abs(q)) for p, q in pairs] if mag else pairs


def assert_exact_model(magnitudes, extra=0):
    """assert_exact with the bound taken from a model run with mag=True on the case's own operands: `magnitudes` (an array, or several)
    holds, per output element, the sum of the magnitudes of every product of every term group (plus the bias).  No partial sum, of any
    subset in any order -- the MFMA's internal order, K splits, atomics, split copies -- exceeds it; `extra`: what an accumulating call
    finds in its output."""
    arrays = magnitudes if isinstance(magnitudes, (list, tuple)) else [magnitudes]
    bound = max(int(np.max(m)) for m in arrays if m is not None and np.size(m)) + int(extra)
    assert bound < 2 ** 24, f'not exact in fp32: sum of magnitudes {bound} >= 2^24'
    return bound


def two_piece_pattern(shape, salt=0, lo=257, hi=1023, density=1.0):
    """Integers with TWO bf16 pieces (int64, of `shape`): magnitudes in [lo, hi] within 257..1023 that are odd (below 512, where bf16 steps
    by 2) or no multiple of 4 (from 512, where it steps by 4), so v = h + m exactly with m != 0; signs and -- density < 1 -- the positions
    of the non-zeros from int_pattern with other salts."""
    assert 257 <= lo < hi <= 1023
    mag = int_pattern(shape, lo, hi, 101 + salt)
    low = mag < 512
    mag = np.where(low, mag | 1, np.where(mag % 4 == 0, mag + 1, mag))
    v = np.where(int_pattern(shape, 0, 1, 102 + salt) == 1, mag, -mag)
    return np.where(sparse_mask(shape, density, 103 + salt), v, 0)


def sparse_mask(shape, density, salt=0):
    """A boolean array with about `density` of its elements set, positions from int_pattern."""
    if density >= 1.0:
        return np.ones(tuple(shape), bool)
    return int_pattern(shape, 0, 9999, salt) < int(round(10000 * density))
