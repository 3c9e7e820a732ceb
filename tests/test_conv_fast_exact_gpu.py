"""The split-bf16 fast mode ('bf16x3') of csrc/conv.hip through the C ABI, on operands whose MID pieces are not zero, with no tolerance.

Every operand v is split as h = bf16(v), m = bf16(v - h) and a product becomes h_a h_b + h_a m_b + m_a h_b.  An integer below 2^16 in
magnitude splits exactly into two integer pieces (conv_reference.bf16_split, torch's CPU bfloat16 cast), so the three-term result is the
integer  sum(a b) - sum(m_a m_b),  and while the sum of the magnitudes of all three term groups stays below 2^24
(conv_reference.assert_exact_model: the model run on the pieces' magnitudes) every partial sum is an exact integer in any order.  The GPU
result must then be np.array_equal to the float64 model of tests/conv_reference.py.  Four operand regimes:

    a2     A two-piece and dense, B in -3..3: every A element's mid piece in every tile position, border tap and remainder row
    b2     A in -3..3, B two-piece and dense: every B element's mid piece -- for the weights the mid PLANE, its tap flip, its zero rows
    both   A and B two-piece and sparse: the m_a m_b term is missing, so the result shows WHICH arithmetic ran (ARITH below is asserted)
    third  A a few elements of 2^17 + 2^8 + 1 (pieces 131 072 and 256, the third piece 1 is dropped), B sparse +-1

(A = x, or dy in the backward GEMMs; B = w, or x in the weight gradient.)  Buffers are guarded as in test_conv_exact_gpu.py, whose helpers
and shapes are used here.  The conditions on the operands -- the bound, the share of non-zero mid pieces, the share of outputs on which the
two arithmetics differ -- are checked without a GPU by tests/test_conv_reference.py for every case of this file."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import conv_reference as cr
import test_conv_exact_gpu as ex
from test_conv_exact_gpu import _device_buffers_live_until_the_test_ends   # noqa: F401  (autouse here too: the buffers live until a test ends)
from test_conv_exact_gpu import OK, PAGE, SENTINEL64, _Output, _deterministic, _err, _guarded_input, _keep, _slack, _workspace, spec
from single_shot_detection_amd import _lib

pytestmark = pytest.mark.gpu

REGIMES = ('a2', 'b2', 'both', 'third')
THIRD = 2 ** 17 + 2 ** 8 + 1   # bf16 steps by 1024 from 2^17: h = 131 072, m = bf16(257) = 256 (a tie, to even), rest = 1
PRODUCTS = 6                   # `both`: products per output element aimed at (non-zeros that meet); `third`: half as many
DEFAULT_MIN_FLOPS = 1.0e9      # SSDK_FAST_MIN_FLOPS unset (csrc/conv_plan.h)

# ---- which outputs are three-term: read off the dispatch code of csrc/conv.hip ----------------------------------------------------------------
# fast_conv_ok: a forward-form launch takes igemm_bf16x3_kernel when its K chain is made of whole 32-channel chunks of 16-byte aligned rows.
# ssdk_conv2d_bwd_fast: conv_dgrad_kind sends a strided data gradient to the scatter / ordered-rows forms, which have no fast kernel; a
#   stride-1 one is the forward form of dy (channels = cout) and needs cout % 32 == 0 and 2 B Hin Win cin k^2 cout >= SSDK_FAST_MIN_FLOPS.
#   launch_wgrad(wg, s, fast) has NO FLOP rule: with 4-multiple channels (the LDS-DMA kernel's condition, which the entry point demands
#   anyway) every weight gradient runs on igemm_wgrad_bf16x3_kernel.  Bias gradients are column sums.
# ssdk_heads_bwd_fast / _ex(fast_terms = 3), ordered pipeline (SSDK_HEADS_BWD_MODE unset, 0, 2): a level in the dense form packs dy to
#   npad = ceil((n_score + n_loc) / 32) * 32 columns -- always whole chunks, so its dx is three-term whatever the forward's column count
#   is (HEADS_TWO level 0: 104 forward columns, 128 packed ones); a level in the anchor-row form (what the device picks at these sizes when
#   the mode is unset) gets dx from anchor_rowgemm_kernel + anchor_dx_kernel, fp32.  Both forms' weight gradients pass `fast` to
#   launch_wgrad, where it takes precedence over rows32.  Legacy pipeline (mode 1): pixel rows scatter dx in fp32; deterministic mode
#   forces its dense form, three-term; both weight-gradient launches pass `fast`.
ARITH = {
    ('ssdk_conv2d_fwd_fast', 'y', 'always'): 'split3',
    ('ssdk_heads_fwd_fast', 'scores locs', 'always'): 'split3',
    ('ssdk_conv2d_bwd_fast', 'dx', 'stride 1, cout % 32 == 0, at or above the FLOP threshold'): 'split3',
    ('ssdk_conv2d_bwd_fast', 'dx', 'stride 1, cout % 32 == 0, below the FLOP threshold'): 'exact',
    ('ssdk_conv2d_bwd_fast', 'dx', 'stride 1, cout % 32 != 0'): 'exact',
    ('ssdk_conv2d_bwd_fast', 'dx', 'stride 2'): 'exact',
    ('ssdk_conv2d_bwd_fast', 'dw', 'always'): 'split3',
    ('ssdk_conv2d_bwd_fast', 'db', 'always'): 'exact',
    ('ssdk_heads_bwd_fast', 'dx', 'ordered, dense form'): 'split3',
    ('ssdk_heads_bwd_fast', 'dx', 'ordered, anchor rows'): 'exact',
    ('ssdk_heads_bwd_fast', 'dx', 'legacy, dense form'): 'split3',
    ('ssdk_heads_bwd_fast', 'dx', 'legacy, pixel rows'): 'exact',
    ('ssdk_heads_bwd_fast', 'dw', 'always'): 'split3',
    ('ssdk_heads_bwd_fast', 'db', 'always'): 'exact',
}


def conv_bwd_arith(s, min_flops=0.0):
    """(dx, dw) of ssdk_conv2d_bwd_fast for a Spec, in either mode (deterministic mode changes the fp32 forms only)."""
    if s.stride != 1:
        path = 'stride 2'
    elif s.cout % 32:
        path = 'stride 1, cout % 32 != 0'
    else:
        flops = 2.0 * s.B * s.H * s.W * s.cin * s.k * s.k * s.cout
        path = 'stride 1, cout % 32 == 0, ' + ('at or above' if flops >= min_flops else 'below') + ' the FLOP threshold'
    return ARITH[('ssdk_conv2d_bwd_fast', 'dx', path)], ARITH[('ssdk_conv2d_bwd_fast', 'dw', 'always')]


def heads_bwd_arith(mode, det):
    """(dx, dw) of ssdk_heads_bwd_fast / _ex(fast_terms = 3) at the sizes of this file (every level's anchor rows fit its T buffer)."""
    if mode == '1':
        path = 'legacy, dense form' if det else 'legacy, pixel rows'
    else:
        path = 'ordered, dense form' if mode == '0' else 'ordered, anchor rows'
    return ARITH[('ssdk_heads_bwd_fast', 'dx', path)], ARITH[('ssdk_heads_bwd_fast', 'dw', 'always')]


# ---- operands -------------------------------------------------------------------------------------------------------------------------------

def _sign(shape, salt):
    return np.where(cr.int_pattern(shape, 0, 1, 104 + salt) == 1, 1, -1)


def _operand(shape, role, regime, salt, density, small, hi):
    """One operand of a GEMM.  role 'A' / 'B'; density: of the non-zeros in `both` and `third`; small: the range of the one-piece side of
    a2 / b2; hi: the largest two-piece magnitude of a2 / b2."""
    if regime in ('a2', 'b2'):
        two = (regime == 'a2') == (role == 'A')
        return cr.two_piece_pattern(shape, salt, 257, hi) if two else cr.int_pattern(shape, small[0], small[1], salt)
    if regime == 'both':
        return cr.two_piece_pattern(shape, salt, 257, 511, density)   # (odd: every m is +-1, a product at most 2^18)
    assert regime == 'third'
    return np.where(cr.sparse_mask(shape, density, 105 + salt), (THIRD if role == 'A' else 1) * _sign(shape, salt), 0)


def _two_piece_hi(longest_chain):
    """a2 / b2: the chain's magnitudes sum to at most chain x (1024 + 2) x 3 -- two-piece values up to 1023 while that stays below 2^24,
    else up to 511 (the case's bound assertion has the last word)."""
    return 1023 if longest_chain * 1026 * 3 < 2 ** 24 else 511


def _densities(regime, chain_a, chains_b, rows=None):
    """Densities (A, [B per chain]) that make about PRODUCTS non-zero products meet per output element of each GEMM.  `both`: A half
    dense when one A serves several GEMMs, else both sides alike; `third`: A a few elements -- at most 64 per column of the `rows` a
    bias gradient sums, 64 x 2^17 = 2^23 --, B as dense as it takes."""
    if regime in ('a2', 'b2'):
        return 1.0, [1.0] * len(chains_b)
    if regime == 'both':
        if len(chains_b) == 1:
            p = min(1.0, (PRODUCTS / chains_b[0]) ** 0.5)
            return p, [p]
        return 0.5, [min(1.0, PRODUCTS / (0.5 * k)) for k in chains_b]
    pa = min(1.0, max(0.05, PRODUCTS / min([chain_a] + list(chains_b))))
    if rows is not None:
        pa = min(pa, 64.0 / rows)
    return pa, [min(1.0, PRODUCTS / 2 / (pa * k)) for k in chains_b]


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def forward_case(s, regime):
    """Operands, the three-term answer and the bound of one forward Spec (shared, never modified).  A Spec with `stats` takes a2 with
    magnitudes small enough for the statistics rule of test_conv_exact_gpu._exact_forward: rows x max(y)^2 < 2^24."""
    K = s.k * s.k * s.cin
    pa, (pb,) = _densities(regime, K, [K])
    xs, ws = (s.B, s.H, s.W, s.cin), (s.cout, s.k, s.k, s.cin)
    if s.stats:
        assert regime == 'a2' and not s.bias
        x = cr.two_piece_pattern(xs, 1 + s.salt, 257, 287)
        w = np.where(ex._sparsify(np.ones((s.cout, K), np.int64), 2, 5).reshape(ws) == 1, _sign(ws, 2 + s.salt), 0)   # two +-1 per output channel
    else:
        hi = _two_piece_hi(K)
        x = _operand(xs, 'A', regime, 1 + s.salt, pa, (-3, 3), hi)
        w = _operand(ws, 'B', regime, 2 + s.salt, pb, (-3, 3), hi)
    b = cr.int_pattern((s.cout,), -2, 2, 3 + s.salt) if s.bias else None
    y = cr.conv_fwd(x, w, b, s.stride, s.pad, s.relu, 'split3')
    bound = cr.assert_exact_model(cr.conv_fwd(x, w, b, s.stride, s.pad, 0, 'split3', mag=True))
    if s.stats:
        ymax = int(np.abs(y).max())
        cr.assert_exact(y[..., 0].size, ymax, ymax)
    return _frozen(dict(x=x, w=w, b=b, y=y, y_exact=cr.conv_fwd(x, w, b, s.stride, s.pad, s.relu), bound=bound))


@functools.lru_cache(maxsize=None)
def backward_case(s, regime, min_flops=0.0):
    """Operands (dy is the A operand of both GEMMs, w and x their B operands), the answers in the arithmetic of conv_bwd_arith, the
    exact-product answers and the bound of one backward Spec."""
    ho, wo = cr.out_dim(s.H, s.k, s.stride, s.pad), cr.out_dim(s.W, s.k, s.stride, s.pad)
    rows = s.B * ho * wo
    k_dx = max(1, s.k * s.k // (s.stride * s.stride)) * s.cout   # (a strided dx element meets about a quarter of the taps)
    pa, (pw, px) = _densities(regime, min(k_dx, rows), [k_dx, rows], rows)
    hi = _two_piece_hi(max(s.k * s.k * s.cout, rows))
    dy = _operand((s.B, ho, wo, s.cout), 'A', regime, 4 + s.salt, pa, (-3, 3), hi)
    w = _operand((s.cout, s.k, s.k, s.cin), 'B', regime, 2 + s.salt, pw, (-3, 3), hi)
    x = _operand((s.B, s.H, s.W, s.cin), 'B', regime, 1 + s.salt, px, (-3, 3), hi)
    arith = conv_bwd_arith(s, min_flops)
    dx, dw, db = cr.conv_bwd(x, w, dy, s.stride, s.pad, arith)
    ex_dx, ex_dw, _ = cr.conv_bwd(x, w, dy, s.stride, s.pad)
    bound = cr.assert_exact_model(cr.conv_bwd(x, w, dy, s.stride, s.pad, arith, mag=True), extra=9)   # (9: what an accumulating call finds)
    return _frozen(dict(x=x, w=w, dy=dy, dx=dx, dw=dw, db=db, dx_exact=ex_dx, dw_exact=ex_dw, arith=arith, bound=bound))


def _keep_mask(B, A, density):
    """The anchors that carry a gradient: the scattered pattern of test_conv_exact_gpu._heads_problem, moved by 16 -- of the twenty
    offsets one of the few that leave every anchor type of the 3 x 3 levels (nine pixels, 54 anchors) a live anchor at a pixel with most
    of its taps, which `both` needs to show the arithmetic in every weight-gradient tensor."""
    a = np.arange(A, dtype=np.int64)[None, :]
    b = np.arange(B, dtype=np.int64)[:, None]
    return np.ones((B, A), bool) if density >= 1.0 else ((b * 7 + a * 13 + (a * a) // 5 + 16) % int(round(1 / density)) == 0)


def _head_levels(defs, B, regime, backward, density):
    """The levels of a heads call as test_conv_exact_gpu._head_array takes them.  Forward: x is A, the weights B.  Backward: x and the
    weights are the B operands of dy, which lives on `density` of the anchors."""
    C_ = defs[0].classes
    levels, a_off = [], 0
    for i, h in enumerate(defs):
        ns, nl = h.types * h.classes, 4 * h.types if h.loc else 0
        xs, K = (B, h.H, h.W, h.cin), 9 * h.cin
        if backward:
            k_dx, rows = 9 * (ns + nl) * density, B * h.H * h.W * density
            pa, (pw, px) = _densities(regime, min(k_dx, rows), [k_dx, rows], rows)
            if regime == 'both':
                # (dy dense on its anchors; where few anchors live, one anchor's C + 4 columns alone give a data-gradient element four products)
                pa, pw, px = 1.0, min(1.0, max(PRODUCTS / k_dx, 4.0 / (C_ + 4) if density < 1.0 else 0.0)), min(1.0, PRODUCTS / rows)
            hi = _two_piece_hi(max(9 * (ns + nl), B * h.H * h.W))
            x = _operand(xs, 'B', regime, 31 + i, px, (-3, 3), hi)
        else:
            pa, (pw,) = _densities(regime, K, [K])
            hi = _two_piece_hi(K)
            x = _operand(xs, 'A', regime, 31 + i, pa, (-3, 3), hi)
        lv = dict(x=x, w_score=_operand((ns, 3, 3, h.cin), 'B', regime, 32 + i, pw, (-3, 3), hi),
                  b_score=cr.int_pattern((ns,), -2, 2, 33 + i) if h.bias else None,
                  w_loc=_operand((nl, 3, 3, h.cin), 'B', regime, 34 + i, pw, (-3, 3), hi) if nl else None,
                  b_loc=cr.int_pattern((nl,), -2, 2, 35 + i) if nl and h.bias else None,
                  scores_offset=a_off * C_, locs_offset=a_off * 4, a_off=a_off, anchors=h.H * h.W * h.types, ns=ns, nl=nl, pa=pa, hi=hi)
        a_off += lv['anchors'] + h.gap
        levels.append(lv)
    return levels, a_off, C_


@functools.lru_cache(maxsize=None)
def heads_forward_case(defs, B, regime):
    levels, A, C_ = _head_levels(defs, B, regime, False, 1.0)
    out = dict(levels=levels, A=A, sb=A * C_, lb=A * 4)
    for key, arith in (('', 'split3'), ('_exact', 'exact')):   # the rows as the library must leave them: sentinel wherever no level lives
        scores, locs = np.full((B, out['sb']), SENTINEL64), np.full((B, out['lb']), SENTINEL64)
        cr.heads_fwd(levels, B, out['sb'], out['lb'], scores, locs, arith)
        out['scores' + key], out['locs' + key] = scores, locs
    ms, ml = np.zeros((B, out['sb'])), np.zeros((B, out['lb']))
    cr.heads_fwd(levels, B, out['sb'], out['lb'], ms, ml, 'split3', mag=True)
    out['bound'] = cr.assert_exact_model([ms, ml])
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def heads_backward_case(defs, B, regime, density, arith):
    """dscores / dlocs (the A operand: the regime's values on the kept anchors, zeros on the others, NaN in the gaps of the rows), the
    truthful row mask and the gradients with (dx, dw) in `arith`."""
    levels, A, C_ = _head_levels(defs, B, regime, True, density)
    live = np.zeros((A,), bool)
    ds, dl = np.zeros((B, A, C_), np.int64), np.zeros((B, A, 4), np.int64)
    for i, lv in enumerate(levels):
        sl = slice(lv['a_off'], lv['a_off'] + lv['anchors'])
        live[sl] = True
        ds[:, sl] = _operand((B, lv['anchors'], C_), 'A', regime, 41 + i, lv['pa'], (-3, 3), lv['hi'])
        dl[:, sl] = _operand((B, lv['anchors'], 4), 'A', regime, 51 + i, lv['pa'], (-3, 3), lv['hi'])
    keep = _keep_mask(B, A, density) & live[None, :]
    ds = np.where(keep[..., None], ds, 0).astype(np.float64)
    dl = np.where(keep[..., None], dl, 0).astype(np.float64)
    out = dict(levels=levels, A=A, sb=A * C_, lb=A * 4, mask=keep.astype(np.uint8))
    flat = (ds.reshape(B, -1), dl.reshape(B, -1))
    out['grads'] = cr.heads_bwd(levels, B, flat[0], flat[1], arith)
    out['grads_exact'] = cr.heads_bwd(levels, B, flat[0], flat[1])
    mags = cr.heads_bwd(levels, B, flat[0], flat[1], arith, mag=True)
    out['bound'] = cr.assert_exact_model([m[k] for m in mags for k in ('dx', 'dw_score', 'db_score', 'dw_loc', 'db_loc')])
    ds[~np.broadcast_to(live[None, :, None], ds.shape)] = np.nan   # the gaps of the gradient rows: nothing may read them
    dl[~np.broadcast_to(live[None, :, None], dl.shape)] = np.nan
    out['ds'], out['dl'] = ds.reshape(B, -1), dl.reshape(B, -1)
    for g in out['grads'] + out['grads_exact']:
        _frozen(g)
    return _frozen(out)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# Forward (tn = 32-column tiles per workgroup = tiles / ceil(tiles / 4)): (a) cout 256: tn 4, Cin 32, 1 x 1, pad 0; (b) ReLU, tn 2, Cin 64;
# (c) stride 2, Cin 128; (d) as (b) without the ReLU; (e) Cin 512, 8 192 rows; (f40) 243 rows (M % 128 != 0), cout 40: 64 weight rows of which
# 24 are zero padding, the last column tile cut at n < N; (f48) 1 x 1, cut at 16.  GROUP8: cout 96 (tn 3), 160 (tn 3 + 2), 32 and 8 (tn 1), both
# strides, pads 0, 1, 2, maps of fewer than 128 rows.
FWD_CASES = dict(ex.DMA_CASES)
FWD_GROUPS = {'group8': (tuple(ex.GROUP8), False),
              'shared_w': (tuple(ex.GROUP8[:1] + [ex.GROUP8[1], ex.GROUP8[7]._replace(salt=0)] + ex.GROUP8[2:7]), True)}
# stats: 2 x 5 x 5 = 50 rows, y at most 2 x 287 = 574: 50 x 574^2 = 16.5 M < 2^24
FWD_STATS = spec(32, 40, 3, 1, 1, 5, 2, bias=0, stats=1)

# Backward.  Stride-1 dx with cout % 32 == 0 runs on igemm_bf16x3_kernel with the flipped-tap planes (tap_len = cout); cin 4 and 24: weight
# rows padded to 32.  Every dw runs on igemm_wgrad_bf16x3_kernel: 75 rows (no multiple of 32), 1 728 rows (K splits), cin 160 / cout 160
# (two channel / row blocks), stride 2 and every border-tap combination of BWD_S1 / BWD_S2.
BWD_CASES = dict(ex.BWD_S1)
BWD_CASES.update(ex.BWD_S2)
BWD_CASES.update({'small3': ex.SMALL3, 'rows_75': ex.WGRAD_ONE['rows_not_a_multiple_of_32'], 'k_splits': ex.WGRAD_ONE['one_problem'],
                  'cout_160': ex.WGRAD_ONE['cout_above_128'], 'cin_160': ex.WGRAD_ONE['cin_above_128'],
                  'cin_4': spec(4, 128, 1, 1, 0, 9, 5), 'cin_24': spec(24, 64, 3, 1, 1, 9, 3, W=6)})
BWD_GROUP = tuple(s for s in ex.WGRAD_GROUP8 if s.cin % 32 == 0 and s.cout % 32 == 0)
# the FLOP threshold: 2 x 2 x H x W x 128 x 9 x 128 = 9.92e8 at 41 x 41, 1.04e9 at 42 x 42
THRESHOLD = {41: spec(128, 128, 3, 1, 1, 41, 2), 42: spec(128, 128, 3, 1, 1, 42, 2)}

HEADS_FWD = {'two': (ex.HEADS_TWO, 3), 'tiny': (ex.HEADS_TINY, 1), 'n340': (ex.HEADS_340, 3)}
HEADS_BWD = {'two': (ex.HEADS_TWO, 3), 'single': (ex.HEADS_SINGLE, 3)}
HEADS_MODES = (None, '0', '1', '2')
DENSITIES = (1.0, 0.05)


def all_cases():
    """Every (kind, case, regime, ...) this file runs: tests/test_conv_reference.py checks the conditions on their operands without a GPU."""
    out = []
    for regime in REGIMES:
        specs = set(FWD_CASES.values()) | {s for g, _ in FWD_GROUPS.values() for s in g}
        out += [('fwd', s, regime) for s in sorted(specs)]
        out += [('fwd', s._replace(relu=1), regime) for s in sorted(specs) if regime == 'both' and s in FWD_CASES.values()]
        out += [('bwd', s, regime, 0.0) for s in sorted(set(BWD_CASES.values()) | set(BWD_GROUP))]
        out += [('heads_fwd', defs, B, regime) for defs, B in HEADS_FWD.values()]
        out += [('heads_bwd', defs, B, regime, d, heads_bwd_arith(m, det)) for defs, B in HEADS_BWD.values() for d in DENSITIES
                for m in ('0', '1', '2') for det in (False, True)]
    out += [('fwd', FWD_STATS, 'a2')]
    out += [('bwd', s, 'both', DEFAULT_MIN_FLOPS) for s in THRESHOLD.values()]
    return sorted(set(out), key=repr)


def case_of(c):
    return {'fwd': forward_case, 'bwd': backward_case, 'heads_fwd': heads_forward_case, 'heads_bwd': heads_backward_case}[c[0]](*c[1:])


# ---- ssdk_conv2d_fwd_fast -------------------------------------------------------------------------------------------------------------------

def _equal(got, want, what):
    want = np.asarray(want, np.float64).ravel()
    assert np.array_equal(got, want), (what, int((got != want).sum()), 'differ,', int(np.isnan(got).sum()), 'NaN')


def _run_forward(specs, regime, share_w=False):
    lib, st = _lib.lib(), _lib.current_stream()
    B, n = specs[0].B, len(specs)
    descs = (_lib.ConvDesc * n)()
    outs, w_of = [], {}
    for d, s in zip(descs, specs):
        f = forward_case(s, regime)
        d.x, d.hin, d.win, d.cin = _guarded_input(f['x'], _slack(s)), s.H, s.W, s.cin
        key = (s.cout, s.k, s.cin, s.salt)
        if share_w and key in w_of:
            d.w, d.bias = w_of[key]
        else:
            d.w = _guarded_input(f['w'], _slack(s))
            d.bias = _guarded_input(f['b'], 0) if s.bias else None
            w_of[key] = (d.w, d.bias)
        d.cout, d.ksize, d.stride, d.pad, d.relu = s.cout, s.k, s.stride, s.pad, s.relu
        y = _Output(f['y'].size)
        d.y = y.ptr
        stats = None
        if s.stats:
            stats = _Output(2 * s.cout + 2, ex._stats_prior(s.cout), dtype=np.float64, slack=4)
            d.stats = stats.ptr
        outs.append((y, stats))
    assert not share_w or len(w_of) < n
    size = lib.ssdk_conv2d_fwd_fast_workspace_bytes(descs, n)
    wp, wcheck = _workspace(size)
    rc = lib.ssdk_conv2d_fwd_fast(descs, n, B, 3, wp, size, st)
    assert rc == OK, (rc, _err())
    for i, (s, (y, stats)) in enumerate(zip(specs, outs)):
        f = forward_case(s, regime)
        _equal(y.read(), f['y'], ('y of descriptor', i, s, regime))
        if stats is not None:
            assert np.array_equal(stats.read(), ex._stats_prior(s.cout) + cr.stats(f['y'])), ('stats of descriptor', i, s)
    wcheck()


@pytest.fixture
def every_launch_is_fast(monkeypatch):
    monkeypatch.setenv('SSDK_FAST_MIN_FLOPS', '0')


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', sorted(FWD_CASES))
def test_forward(name, regime, every_launch_is_fast):
    s = FWD_CASES[name]
    _run_forward([s], regime)
    if regime == 'both' and not s.relu:   # (with a ReLU, which negative sums need: case b)
        _run_forward([s._replace(relu=1)], regime)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', sorted(FWD_GROUPS))
def test_forward_grouped(name, regime, every_launch_is_fast):
    """Eight problems in one call: of different weights, and with two descriptors sharing a weight tensor (split once)."""
    specs, share = FWD_GROUPS[name]
    _run_forward(list(specs), regime, share_w=share)


def test_forward_with_statistics(every_launch_is_fast):
    _run_forward([FWD_STATS], 'a2')


# ---- ssdk_heads_fwd_fast --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', sorted(HEADS_FWD))
def test_heads_forward(name, regime, every_launch_is_fast):
    """'two': score and loc weights in ONE plane with no padding between them (84 + 16 = 100 rows of 128), a last tile of 4 columns;
    'tiny': three levels at batch 1; 'n340': 324 + 16 columns, three column blocks."""
    lib, st = _lib.lib(), _lib.current_stream()
    defs, B = HEADS_FWD[name]
    P = heads_forward_case(defs, B, regime)
    arr, _ = ex._head_array(defs, P, B)
    scores = _Output(B * P['sb'], np.where(P['scores'] == SENTINEL64, SENTINEL64, np.nan))
    locs = _Output(B * P['lb'], np.where(P['locs'] == SENTINEL64, SENTINEL64, np.nan))
    size = lib.ssdk_heads_fwd_fast_workspace_bytes(arr, len(defs))
    wp, wcheck = _workspace(size)
    rc = lib.ssdk_heads_fwd_fast(arr, len(defs), B, C.c_void_p(scores.ptr), P['sb'], C.c_void_p(locs.ptr), P['lb'], 3, wp, size, st)
    assert rc == OK, (rc, _err())
    _equal(scores.read(), P['scores'], ('scores', name, regime))
    _equal(locs.read(), P['locs'], ('locs', name, regime))
    wcheck()


# ---- ssdk_conv2d_bwd_fast -------------------------------------------------------------------------------------------------------------------

def _run_backward(specs, regime, accumulate, min_flops=0.0):
    """One grouped ssdk_conv2d_bwd_fast call: dx, dw, db must equal the model in the arithmetic of ARITH.  Returns the results' bits."""
    lib, st = _lib.lib(), _lib.current_stream()
    n, B = len(specs), specs[0].B
    descs = (_lib.ConvDesc * n)()
    prior_dw = lambda s: cr.int_pattern((s.cout, s.k, s.k, s.cin), -9, 9, 21)
    prior_db = lambda s: cr.int_pattern((s.cout,), -9, 9, 22)
    outs = []
    for d, s in zip(descs, specs):
        f = backward_case(s, regime, min_flops)
        d.x, d.hin, d.win, d.cin = _guarded_input(f['x'], _slack(s)), s.H, s.W, s.cin
        d.cout, d.ksize, d.stride, d.pad, d.relu = s.cout, s.k, s.stride, s.pad, 0
        d.dy, d.w = _guarded_input(f['dy'], _slack(s)), _guarded_input(f['w'], _slack(s))
        o = dict(dx=_Output(f['x'].size), dw=_Output(f['w'].size, prior_dw(s) if accumulate else np.nan),
                 db=_Output(s.cout, prior_db(s) if accumulate else np.nan))
        d.dx, d.dw, d.db = o['dx'].ptr, o['dw'].ptr, o['db'].ptr
        outs.append(o)
    size = lib.ssdk_conv2d_bwd_fast_workspace_bytes(descs, n, B)
    wp, wcheck = _workspace(size)
    rc = lib.ssdk_conv2d_bwd_fast(descs, n, B, accumulate, 3, wp, size, st)
    assert rc == OK, (rc, _err())
    bits = []
    for i, (s, o) in enumerate(zip(specs, outs)):
        f = backward_case(s, regime, min_flops)
        want = dict(dx=f['dx'], dw=f['dw'] + (prior_dw(s) if accumulate else 0), db=f['db'] + (prior_db(s) if accumulate else 0))
        for key in ('dx', 'dw', 'db'):
            got = o[key].read()
            _equal(got, want[key], (key, 'of descriptor', i, s, regime, f['arith']))
            bits.append(got.view(np.uint32))
    wcheck()
    return bits


def _backward_in_every_mode(specs, regime, min_flops=0.0):
    """accumulate 0 and 1, the default mode once and deterministic mode twice with equal bits."""
    for accumulate in (0, 1):
        _run_backward(specs, regime, accumulate, min_flops)
        with _deterministic(True):
            a = _run_backward(specs, regime, accumulate, min_flops)
            b = _run_backward(specs, regime, accumulate, min_flops)
        assert len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b)), 'deterministic mode: two runs differ'


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', sorted(BWD_CASES))
def test_backward(name, regime, every_launch_is_fast):
    _backward_in_every_mode([BWD_CASES[name]], regime)


@pytest.mark.parametrize('regime', REGIMES)
def test_backward_grouped(regime, every_launch_is_fast):
    """Four problems in one call: 2 880 and 80 rows side by side (the launch-wide K-split rule), stride 1 and 2."""
    _backward_in_every_mode(list(BWD_GROUP), regime)


@pytest.mark.parametrize('side', sorted(THRESHOLD))
def test_backward_flop_threshold(side, monkeypatch):
    """SSDK_FAST_MIN_FLOPS unset: the data-gradient launch of 9.92e8 FLOPs (41 x 41) stays fp32 -- the exact products --, the one of 1.04e9
    (42 x 42) is three-term; the weight gradient has no such rule and is three-term at both sizes."""
    monkeypatch.delenv('SSDK_FAST_MIN_FLOPS', raising=False)
    s = THRESHOLD[side]
    assert backward_case(s, 'both', DEFAULT_MIN_FLOPS)['arith'] == (('exact', 'split3') if side == 41 else ('split3', 'split3'))
    for det in (False, True):
        with _deterministic(det):
            _run_backward([s], 'both', 0, DEFAULT_MIN_FLOPS)


# ---- ssdk_heads_bwd_fast, ssdk_heads_bwd_ex(fast_terms = 3) ------------------------------------------------------------------------------------

def _run_heads_backward(defs, B, regime, density, arith, entry):
    """entry: 'fast' (ssdk_heads_bwd_fast), 'ex' (ssdk_heads_bwd_ex, fast_terms = 3, no mask), 'ex_mask' (with the truthful row mask)."""
    lib, st = _lib.lib(), _lib.current_stream()
    P = heads_backward_case(defs, B, regime, density, arith)
    arr, outs = ex._head_array(defs, P, B, with_grads=True)
    ds = _guarded_input(P['ds'], PAGE)
    dl = _guarded_input(P['dl'], PAGE) if any(lv['nl'] for lv in P['levels']) else None
    size = lib.ssdk_heads_bwd_fast_workspace_bytes(arr, len(defs), B)
    wp, wcheck = _workspace(size)
    if entry == 'fast':
        rc = lib.ssdk_heads_bwd_fast(arr, len(defs), B, ds, P['sb'], dl, P['lb'], 3, wp, size, st)
    else:
        mask = C.c_void_p(_keep(torch.from_numpy(P['mask'].copy()).cuda()).data_ptr()) if entry == 'ex_mask' else None
        rc = lib.ssdk_heads_bwd_ex(arr, len(defs), B, ds, P['sb'], dl, P['lb'], mask, P['A'] if mask else 0, 3, wp, size, st)
    assert rc == OK, (rc, _err())
    bits = []
    for i, (o, want) in enumerate(zip(outs, P['grads'])):
        for key in ('dx', 'dw_score', 'db_score', 'dw_loc', 'db_loc'):
            if o[key] is None:
                continue
            got = o[key].read()
            _equal(got, want[key], (key, 'of level', i, regime, density, arith, entry))
            bits.append(got.view(np.uint32))
    wcheck()
    return bits


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('density', DENSITIES)
@pytest.mark.parametrize('mode', HEADS_MODES)
@pytest.mark.parametrize('name', sorted(HEADS_BWD))
def test_heads_backward(name, mode, density, regime, every_launch_is_fast, monkeypatch):
    """Every form SSDK_HEADS_BWD_MODE selects (unset: the device picks anchor rows at these sizes; 0 dense; 1 the legacy pipeline: pixel
    rows, dense in deterministic mode; 2 anchor rows), dense gradients and one anchor in twenty, through the three entry points."""
    ex._heads_mode(monkeypatch, mode)
    defs, B = HEADS_BWD[name]
    for entry in ('fast', 'ex_mask', 'ex'):
        _run_heads_backward(defs, B, regime, density, heads_bwd_arith(mode, False), entry)
    with _deterministic(True):
        arith = heads_bwd_arith(mode, True)
        a = _run_heads_backward(defs, B, regime, density, arith, 'ex_mask')
        b = _run_heads_backward(defs, B, regime, density, arith, 'ex_mask')
    assert all(np.array_equal(p, q) for p, q in zip(a, b)), 'deterministic mode: two runs differ'
