"""Inputs of the strict postprocess tests (tests/test_postprocess_cases.py on the CPU, tests/test_postprocess_exact_gpu.py on the GPU) and
the rule that makes them DECIDABLE: selection, order and suppression of a case never depend on the last ulp of an exp(), so the library
must give the oracle's detections row for row, with no selection boundary to excuse a difference.  numpy only; nothing here touches a GPU.

How the inputs are built
  * locs = 0 and priors in centroid form whose corners are integers below 2^11 (integer centres and even sizes; the hand-made on-threshold
    pairs have half-integer centres under odd sizes, with integer corners all the same).  decode_box gives cx + w * 0 / 10 = cx and
    w * exp(0) = w, to_corners cx -+ w / 2: corners, areas (< 2^22), intersections and unions (< 2^23) are exact integers in fp32, so
    inter / union is ONE correctly rounded division of the same two integers on both sides.
  * Logit rows are dealt from a small set of prototype rows (or, for the list-length cases, from a few logit levels per class).  Equal rows
    give bit-equal probabilities on the device -- the row pass does the same operations on the same values wherever the row sits -- and a
    sigmoid probability is a function of its one logit, so equal logits do as well.  Among equal probabilities the order is the key's: lower
    anchor first, which is the oracle's stable order.

assert_decidable(case) checks, in float64 on the CPU and for every image:
  (a) no probability is within 1e-3 relative of the score threshold;
  (b) within a class, two candidate probabilities are equal by construction (softmax: identical rows; sigmoid: identical logits) or at least
      1e-4 relative apart;
  (c) every pair of boxes has |inter / union - nms_thr| > 1e-4 (inter and union are integers, the test is |inter - thr * union| >
      1e-4 * union in float64, whose error is 1e-16) -- except the pairs built to sit ON the threshold, whose fate is worked out by hand
      (ON_THRESHOLD below, tests/test_postprocess_cases.py);
  (d) with max_total = mt the oracle is also run with mt + 8: that list holds at most mt rows, or its rows mt - 1 and mt differ by at least
      1e-4 relative in score, or they are two rows of ONE class with equal scores by construction (bit-equal on the device; both sides then
      take the one NMS kept first).
1e-3 and 1e-4 are 100x and 10x the 1e-5 relative score tolerance of the suite (Boundaries.near): conditions on the inputs, not measurements
of the library.  A generator reseeds until they hold (at most 128 seeds; 45 were the most any case below needed).

Every case pins the plan with SSDK_POST_SAMPLE or SSDK_POST_NO_SAMPLE (without either the plan depends on what the previous call of the
process left), and carries `expect`: what ssdk_debug_postprocess_plan must say of it, with the arithmetic in the comment of its family.
The arithmetic's ingredients (csrc/postprocess.hip):
  tiles = ceil(A / 64);  ns0 = ceil(tiles / 8);  ns = ns0 if the sample pass is wanted and ns0 * 64 >= 4 K and tiles > ns0, else 0
  per_image = clamp(ceil(WGS / B), 1, 64), WGS = SSDK_POST_WGS or 768;  tm = tiles - ns;  Tm = ceil(tm / min(tm, per_image))
  JMAX = 6 / 12 / 21 / 24 for ceil(C / 4) <= 6 / 12 / 21 / else;  pad = C even
  khead: h = max(16, 8 ceil(5 mt / (2 ncls) / 8)) (integer division inside); 0 if no mt, h > 64, 2 h > K, ncls h <= mt or ncls h > 6144
  v2 needs C <= 96, K <= 128, ncls K <= 8192, mt <= 256; K None or > 256 is the greedy path; everything else the general pipeline
  tie_up = the last mantissa bit of the fp32 nms threshold: 0.35f 0x3eb33333, 0.4f 0x3ecccccd, 0.55f 0x3f0ccccd, 0.7f 0x3f333333 odd;
  0.3f 0x3e99999a, 0.45f 0x3ee66666, 0.5f 0x3f000000 even
"""
import collections
import functools

import numpy as np

F32 = np.float32
V2, GREEDY, GENERAL = 0, 1, 2   # ssdk_debug_postprocess_plan out[0]
PLAN_FIELDS = ('pipeline', 'softmax', 'pad', 'jmax', 'tiles', 'ns', 'Gs', 'Ts', 'Gm', 'Tm', 'nseg', 'list_cap', 'khead', 'tie_up', 'fold')

SAMPLE = (('SSDK_POST_SAMPLE', '1'),)
NO_SAMPLE = (('SSDK_POST_NO_SAMPLE', '1'),)
ALL_KNOBS = ('SSDK_POST_SAMPLE', 'SSDK_POST_NO_SAMPLE', 'SSDK_POST_WGS', 'SSDK_POST_NO_FOLD', 'SSDK_NMS_ONE_PASS', 'SSDK_POST_OLD',
             'SSDK_POST_NO_HOT', 'SSDK_POST_STOP', 'SSDK_NMS_STOP')   # a test clears these before it sets a case's own

# name B A C softmax K mt nms_thr thr env shift: the call (K / mt None as in the Python API; shift: floats the scores pointer is moved off
# 16-byte alignment).  gen, gen_kw: the logits; boxes: 'cluster' | 'spread'; pairs: the on-threshold pairs are put in; expect: plan fields.
Spec = collections.namedtuple('Spec', 'name B A C softmax K mt nms_thr thr env shift gen gen_kw boxes pairs expect')
Case = collections.namedtuple('Case', 'spec seed logits ident locs priors pair_anchors')

SPECS = collections.OrderedDict()


def _add(name, B, A, C, softmax, K, mt, nms_thr, env, gen='deal', gen_kw=(), boxes='cluster', pairs=False, shift=0, thr=0.01, **expect):
    assert name not in SPECS, name
    expect.setdefault('softmax', int(softmax))
    expect.setdefault('tiles', -(-A // 64))
    expect.setdefault('tie_up', TIE_UP[nms_thr])
    SPECS[name] = Spec(name, B, A, C, bool(softmax), K, mt, nms_thr, thr, tuple(env), shift, gen, tuple(sorted(dict(gen_kw).items())), boxes, pairs,
                       tuple(sorted(expect.items())))


TIE_UP = {0.35: 1, 0.4: 1, 0.55: 1, 0.7: 1, 0.3: 0, 0.45: 0, 0.5: 0}   # bit 0 of the fp32 value (checked in test_postprocess_cases.py)

# ---- the pairs that sit on a threshold -----------------------------------------------------------------------------------------------------
# (corner boxes a, b, inter, union): inter / union in lowest terms on the right.  All lie left of / above x, y = 330, every other box of a
# case right of / below 360: a pair only ever meets its own partner.
PAIRS = (
    ((0, 0, 10, 10), (0, 0, 9, 5), 45, 100),                 # 9 / 20: RN = 0.45f = 0.449999988 < 9 / 20
    ((100, 100, 110, 110), (100, 100, 107, 110), 70, 100),   # 7 / 10: RN = 0.7f = 0.699999988 < 7 / 10
    ((200, 200, 220, 220), (200, 200, 214, 210), 140, 400),  # 7 / 20: RN = 0.35f = 0.349999994 < 7 / 20
    ((300, 300, 320, 320), (300, 300, 320, 311), 220, 400),  # 11 / 20: RN = 0.55f = 0.550000012 > 11 / 20
)
# The fate of b at the threshold its pair sits on, by hand: hard NMS drops b iff RN(inter / union) > thr in fp32.  In all four the
# quotient rounds to the threshold ITSELF, so the comparison is false and b is KEPT -- although for the first three the exact quotient lies
# above the float threshold (a comparison of exact values, or inter > (double)thr * union, would drop b), and for the last it lies below.
ON_THRESHOLD = {0.45: (0, True), 0.7: (1, True), 0.35: (2, True), 0.55: (3, True)}   # thr: (index into PAIRS, b kept)
PAIR_CLASS = 1          # the pairs' class, as an index into the non-background classes
PAIR_LOGITS = (7.0, 6.6, 6.2, 5.8, 5.4, 5.0, 4.6, 4.2)   # a then b of pair 0, 1, 2, 3: above every dealt logit, 0.4 apart (>= 2.7e-4 relative in p)


def _corner_to_centroid(b):
    return ((b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0, b[2] - b[0], b[3] - b[1])


# ---- generators ------------------------------------------------------------------------------------------------------------------------------

def _priors(boxes, A, rng):
    if boxes == 'cluster':   # heavy overlap: centres in a 120 x 120 window, sizes 16 .. 78
        c = rng.integers(400, 520, (A, 2))
        wh = 2 * rng.integers(8, 40, (A, 2))
    else:                    # 'spread': a 32-wide grid of pitch 12 with sizes 16 .. 46 -- a box meets its neighbours only, most boxes survive NMS
        a = np.arange(A)
        c = np.stack([400 + 12 * (a % 32), 400 + 12 * (a // 32)], 1)
        wh = 2 * rng.integers(8, 24, (A, 2))
    return np.concatenate([c, wh], 1).astype(F32)


def _gen_deal(spec, rng, protos=12, scale=2.0, bias=0.0, bg=0.0, dense_rows=0, sparse_bias=-9.0):
    """Rows dealt from `protos` prototype rows.  dense_rows > 0: rows r of a 64-row tile with r % 64 >= dense_rows come from a second set of
    prototypes shifted by sparse_bias instead (the select kernel's wave w takes rows 16 w .. 16 w + 15 of a tile)."""
    B, A, C = spec.B, spec.A, spec.C
    P = rng.standard_normal((protos, C)) * scale + bias
    if spec.softmax:
        P[:, 0] += bg
    P = P.astype(F32)
    ident = rng.integers(0, protos, (B, A))
    if dense_rows:
        P2 = (rng.standard_normal((protos, C)) * scale + bias + sparse_bias).astype(F32)
        P = np.concatenate([P, P2], 0)
        ident = np.where((np.arange(A) % 64 < dense_rows)[None, :], ident, ident + protos)
    return P[ident], ident


def _gen_lengths(spec, rng, lengths=(), levels=8):
    """Sigmoid: class c of image i holds exactly lengths[(c + i) % ncls] candidates, their logits cycling through `levels` values of the class
    (runs of equal scores); every other logit is -10 (p = 4.5e-5, far below the threshold)."""
    B, A, C = spec.B, spec.A, spec.C
    assert not spec.softmax and len(lengths) == C
    x = np.full((B, A, C), -10.0, F32)
    lv = np.sort(rng.uniform(-2.0, 4.0, (C, levels)).astype(F32), 1)
    for i in range(B):
        for c in range(C):
            n = lengths[(c + i) % C]
            at = rng.permutation(A)[:n]
            x[i, at, c] = lv[c, rng.integers(0, levels, n)]
    return x, None


GENERATORS = {'deal': _gen_deal, 'lengths': _gen_lengths}


def _generate(spec, seed):
    rng = np.random.default_rng(seed)
    priors = _priors(spec.boxes, spec.A, rng)
    logits, ident = GENERATORS[spec.gen](spec, rng, **dict(spec.gen_kw))
    pair_anchors = ()
    if spec.pairs:
        # the eight boxes at anchors drawn at random: spread over the tiles, b in front of a as often as behind it
        at = rng.permutation(spec.A)[:8]
        cls = PAIR_CLASS + (1 if spec.softmax else 0)
        ident = ident.copy()   # (the pairs' rows are no prototype rows: an identity of their own each)
        for k in range(8):
            a, b = PAIRS[k // 2][0], PAIRS[k // 2][1]
            priors[at[k]] = _corner_to_centroid(b if k & 1 else a)
            row = np.full(spec.C, -3.0, F32)
            if spec.softmax:
                row[0] = 0.0
            row[cls] = PAIR_LOGITS[k]
            logits[:, at[k]] = row
            ident[:, at[k]] = 1000 + k
        pair_anchors = tuple((int(at[2 * k]), int(at[2 * k + 1])) for k in range(4))
    locs = np.zeros((spec.B, spec.A * 4), F32)
    return Case(spec, seed, np.ascontiguousarray(logits.reshape(spec.B, -1)), ident, locs, priors, pair_anchors)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------

def probabilities(case):
    """float64 [B, A, ncls]"""
    s = case.spec
    x = case.logits.astype(np.float64).reshape(s.B, s.A, s.C)
    if s.softmax:
        e = np.exp(x - x.max(2, keepdims=True))
        return (e / e.sum(2, keepdims=True))[:, :, 1:]
    return 1.0 / (1.0 + np.exp(-x))


def corners(case):
    """int64 [A, 4]; asserts that the fp32 decode of the priors gives exactly these integers."""
    p = case.priors
    half_w, half_h = p[:, 2] / F32(2), p[:, 3] / F32(2)
    c32 = np.stack([p[:, 0] - half_w, p[:, 1] - half_h, p[:, 0] + half_w, p[:, 1] + half_h], 1)
    assert c32.dtype == F32
    c = np.rint(c32).astype(np.int64)
    assert np.array_equal(c.astype(F32), c32) and c.min() >= 0 and c.max() < 2048, 'corners are not integers below 2^11'
    assert ((c[:, 2] > c[:, 0]) & (c[:, 3] > c[:, 1])).all()
    return c


def _iou_margin_ok(c, thr, exempt):
    """(c): |inter - thr * union| > 1e-4 * union for every pair of boxes but `exempt` (a set of frozenset anchor pairs)."""
    t = float(F32(thr))
    area = (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])
    for lo in range(0, len(c), 256):
        blk = c[lo:lo + 256]
        iw = np.clip(np.minimum(blk[:, None, 2], c[None, :, 2]) - np.maximum(blk[:, None, 0], c[None, :, 0]), 0, None)
        ih = np.clip(np.minimum(blk[:, None, 3], c[None, :, 3]) - np.maximum(blk[:, None, 1], c[None, :, 1]), 0, None)
        inter = iw * ih
        union = area[lo:lo + 256, None] + area[None, :] - inter
        bad = np.abs(inter - t * union) <= 1e-4 * union
        for r, q in zip(*np.nonzero(bad)):
            if frozenset((int(r) + lo, int(q))) not in exempt:
                return False
    return True


def _identity(case, i, c):
    """What makes two probabilities of class c (index among the non-background classes) of image i equal by construction."""
    s = case.spec
    if s.softmax:
        assert case.ident is not None
        return case.ident[i]
    return case.logits.reshape(s.B, s.A, s.C)[i, :, c].view(np.uint32).astype(np.int64)


def on_threshold_pair(spec):
    """Index into PAIRS of the pair that sits on this case's NMS threshold, or None."""
    return ON_THRESHOLD[spec.nms_thr][0] if spec.pairs and spec.nms_thr in ON_THRESHOLD else None


def oracle_rows(case, max_total='same', nms_thr=None):
    import oracle
    s = case.spec
    return oracle.postprocess(case.logits, case.locs, case.priors, softmax=s.softmax, score_thr=s.thr, max_per_class=s.K,
                              nms_thr=s.nms_thr if nms_thr is None else nms_thr, max_total=s.mt if max_total == 'same' else max_total,
                              return_cand=True)


def why_undecidable(case):
    """None when (a) .. (d) hold, else a string that says which does not."""
    s = case.spec
    p = probabilities(case)
    if (np.abs(p - s.thr) <= 1e-3 * s.thr).any():
        return '(a) a probability within 1e-3 of the score threshold'
    ncls = p.shape[2]
    for i in range(s.B):
        for c in range(ncls):
            idn = _identity(case, i, c)
            pc = p[i, :, c]
            cand = np.nonzero(pc > s.thr)[0]
            order = cand[np.argsort(-pc[cand], kind='stable')]
            hi, lo = order[:-1], order[1:]
            close = (pc[hi] - pc[lo]) < 1e-4 * pc[hi]
            if (close & (idn[hi] != idn[lo])).any():
                return '(b) two candidates of image %d class %d closer than 1e-4 and not equal by construction' % (i, c)
            if (idn[hi] == idn[lo]).any() and not (pc[hi] == pc[lo])[idn[hi] == idn[lo]].all():
                return '(b) equal by construction but different in float64'
    k = on_threshold_pair(s)
    exempt = {frozenset(case.pair_anchors[k])} if k is not None else set()
    if not _iou_margin_ok(corners(case), s.nms_thr, exempt):
        return '(c) a pair of boxes within 1e-4 of the NMS threshold'
    if s.mt:
        rows, _ = oracle_rows(case, max_total=s.mt + 8)
        for i, r in enumerate(rows):
            if len(r) <= s.mt:
                continue
            r = r[np.argsort(-r[:, 5], kind='stable')]   # (a list the mt + 8 did not cut is in class order)
            a, b = r[s.mt - 1], r[s.mt]
            if a[5] - b[5] >= 1e-4 * a[5]:
                continue
            if not (a[4] == b[4] and a[5] == b[5]):
                return '(d) rows mt - 1 and mt of image %d closer than 1e-4 and not one class with equal scores' % i
    return None


def assert_decidable(case):
    why = why_undecidable(case)
    assert why is None, (case.spec.name, case.seed, why)


@functools.lru_cache(maxsize=None)
def build(name):
    """The case of SPECS[name]: the first of 128 seeds whose inputs are decidable."""
    import zlib
    spec = SPECS[name]
    base = zlib.crc32(name.encode()) % 100000 * 128
    for seed in range(base, base + 128):
        case = _generate(spec, seed)
        if why_undecidable(case) is None:
            for a in (case.logits, case.locs, case.priors):
                a.setflags(write=False)
            return case
    raise AssertionError('no decidable inputs within 128 seeds for ' + name)


def set_env(monkeypatch, spec):
    """The environment of the case, and none of the other knobs (monkeypatch: pytest's)."""
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in spec.env:
        monkeypatch.setenv(k, v)


def plan(lib, spec, sample=-1):
    """(status, fields) of ssdk_debug_postprocess_plan for the call of `spec` under the CURRENT environment (lib: _lib.lib())."""
    import ctypes
    out = (ctypes.c_longlong * 16)()
    rc = lib.ssdk_debug_postprocess_plan(spec.B, spec.A, spec.C, int(spec.softmax), spec.K or 0, spec.nms_thr, 0, spec.mt or 0, sample, out)
    return rc, dict(zip(PLAN_FIELDS, list(out)))


def out_cap(spec):
    """The smallest out_cap include/ssdk.h allows."""
    ncls = spec.C - 1 if spec.softmax else spec.C
    return spec.mt if spec.mt else ncls * (min(spec.K, spec.A) if spec.K else spec.A)


def jmax_of(C):
    return 6 if C <= 24 else 12 if C <= 48 else 21 if C <= 84 else 24


# ==== the cases ======================================================================================================================================

# ---- 1. every class count: C = 1 .. 97 sigmoid, 2 .. 97 softmax; A = 130 (two full tiles and a 2-row tile), B = 2, K = 16, mt = 40 -------------
# tiles = 3.  Sample plan: ns0 = 1, 64 >= 4 * 16 and 3 > 1, so ns = 1, tm = 2; without: ns = 0, tm = 3.  per_image = min(64, 768 / 2) = 64 >=
# tm: Tm = 1.  khead: 2 h >= 32 > K = 16, one pass (MODE 0) + post_merge2_kernel.  C <= 96: v2 with JMAX 6 (C <= 24), 12 (<= 48), 21 (<= 84),
# 24 (<= 96), pad = C even; C = 97: the general pipeline (C > kSelMaxC).  ncls K <= 1536, mt <= 256.
SWEEP = []
for _soft in (0, 1):
    for _C in range(2 if _soft else 1, 98):
        for _env, _tag in ((SAMPLE, 'sample'), (NO_SAMPLE, 'nosample')):
            _n = 'sweep-%s-C%d-%s' % ('softmax' if _soft else 'sigmoid', _C, _tag)
            if _C <= 96:
                _add(_n, 2, 130, _C, _soft, 16, 40, 0.5, _env, pipeline=V2, jmax=jmax_of(_C), pad=int(_C % 2 == 0), ns=1 if _env is SAMPLE else 0,
                     Tm=1, khead=0, fold=0)
            else:
                _add(_n, 2, 130, _C, _soft, 16, 40, 0.5, _env, pipeline=GENERAL)
            SWEEP.append(_n)

# ---- 2. alignment and tile edges: C in {3, 21, 25, 80, 95} x A in {64, 65, 127, 128, 129, 777}, B = 3, K = 16, mt = 40, SSDK_POST_WGS = 3 ----------
# per_image = ceil(3 / 3) = 1: ONE workgroup per image walks every tile, Tm = tiles - ns (the register prefetch crosses tiles for the unpadded
# odd C = 3, 21, 25, 95; the padded row index arithmetic for C = 80).  No sample pass: Tm = 1, 2, 2, 2, 3, 13.  A = 65 / 129: a last tile of ONE
# row, with C = 3 of 3 floats (rows * C < 4: no float4 at all).  Odd A * C (A = 65, 127, 129, 777 with odd C): images 1 and 2 start off 16-byte
# alignment (777 * 3 * 4 = 9 324 = 12 mod 16), vec and pre_valid false.  A = 777 with the sample pass: tiles = 13, ns0 = 2, 128 >= 64: ns = 2
# (Gs = 1, Ts = 2), Tm = 11.  Shifted `scores` pointers (4, 8, 12 bytes) at A = 129: every image unaligned.
ALIGN = []
for _C in (3, 21, 25, 80, 95):
    _soft = int(_C in (21, 25, 95))
    for _A in (64, 65, 127, 128, 129, 777):
        _variants = [(NO_SAMPLE, 0, 'nosample', 0, -(-_A // 64))]
        if _A == 777:
            _variants.append((SAMPLE, 0, 'sample', 2, 11))
        if _A == 129 and _C in (3, 25, 80):
            _variants += [(NO_SAMPLE, sh, 'shift%d' % (4 * sh), 0, 3) for sh in (1, 2, 3)]
        for _env, _sh, _tag, _ns, _Tm in _variants:
            _n = 'align-C%d-A%d-%s' % (_C, _A, _tag)
            _add(_n, 3, _A, _C, _soft, 16, 40, 0.45, _env + (('SSDK_POST_WGS', '3'),), shift=_sh, boxes='spread' if _A == 777 else 'cluster', pipeline=V2, jmax=jmax_of(_C), pad=int(_C % 2 == 0),
                 ns=_ns, Gm=1, Tm=_Tm, khead=0, fold=0)
            ALIGN.append(_n)

# ---- 3. the select kernel's survivor queue (256 entries per wave of 16 rows): sigmoid, 20 classes, A = 200, B = 2, K = 32, mt = 100 ----------------
# dense: every logit is N(0.5, 1) (p > 0.01 needs x > -4.6), every pair passes: 16 * 20 = 320 survivors per wave > 256, the per-thread loop.  sparse (softmax, C = 21,
# background + 6): a few per wave, the queue.  mixed: rows 0 .. 15 of every tile dense, the others N(-8.5, 1): wave 0 overflows, waves 1 .. 3 do not.
# khead: h = max(16, 8 ceil((500 / 40 = 12) / 8)) = 16, 2 h = 32 <= K, 20 * 16 = 320 > 100: head + finish.
QUEUE = ['queue-dense', 'queue-sparse', 'queue-mixed']
_add('queue-dense', 2, 200, 20, 0, 32, 100, 0.5, NO_SAMPLE, gen_kw=dict(scale=1.0, bias=0.5), pipeline=V2, jmax=6, pad=1, ns=0, Tm=1, khead=16, fold=1)
_add('queue-sparse', 2, 200, 21, 1, 32, 100, 0.5, NO_SAMPLE, gen_kw=dict(bg=6.0), pipeline=V2, jmax=6, pad=0, ns=0, Tm=1, khead=16, fold=1)
_add('queue-mixed', 2, 200, 20, 0, 32, 100, 0.5, NO_SAMPLE, gen_kw=dict(scale=1.0, bias=0.5, dense_rows=16), pipeline=V2, jmax=6, pad=1, ns=0, Tm=1,
     khead=16, fold=1)

# ---- 4. list lengths -----------------------------------------------------------------------------------------------------------------------------
# lengths: sigmoid, 12 classes, A = 300, K = 64, mt = 60: h = max(16, 8 ceil((300 / 24 = 12) / 8)) = 16, 2 h <= 64, 12 * 16 = 192 > 60: Khead = 16.
# Per-class lists of 0, 1, Khead, Khead + 1, 64, 65, 128, 129 keys (and 30, 200, 5, 100), rotated by one class in image 1.
# long: sigmoid, 3 classes, A = 1500 dense: 1500 keys per list, past the 1024-key LDS cache of the NMS waves.  K = 128, mt = 40:
# h = 8 ceil((200 / 6 = 33) / 8) = 40, 2 h = 80 <= 128, 3 * 40 = 120 > 40: Khead = 40.  tiles = 24, per_image = 64: Tm = 1.
LENGTHS = ['lengths', 'long']
_add('lengths', 2, 300, 12, 0, 64, 60, 0.45, NO_SAMPLE, gen='lengths', gen_kw=dict(lengths=(0, 1, 16, 17, 64, 65, 128, 129, 30, 200, 5, 100)),
     boxes='spread', pipeline=V2, jmax=6, pad=1, ns=0, Tm=1, khead=16, fold=1)
_add('long', 2, 1500, 3, 0, 128, 40, 0.45, NO_SAMPLE, gen_kw=dict(scale=1.5, bias=1.0), boxes='spread', pipeline=V2, jmax=6, pad=0, ns=0, Tm=1,
     khead=40, fold=1)

# ---- 5. NMS thresholds, odd and even last mantissa bit, with the on-threshold pairs among ordinary boxes: softmax, C = 5, A = 200, B = 2 -------------
# mode0: K = 64, no max_total: one pass, post_nms_wave_kernel<TIE, 0>.  head: mt = 40: h = 8 ceil((200 / 8 = 25) / 8) = 32, 2 h = 64 <= K,
# 4 * 32 = 128 > 40: post_nms_wave_kernel<TIE, 1> + post_finish_kernel<TIE>.  nofold: the same under SSDK_POST_NO_FOLD: <TIE, 1>,
# post_img_tau_kernel, <TIE, 2>, post_merge2_kernel.  onepass: the same under SSDK_NMS_ONE_PASS: <TIE, 0> with a max_total.
# general: K = 200 > 128.  greedy: K = None.
THRESHOLDS = []
for _t in (0.35, 0.4, 0.55, 0.7, 0.3, 0.45, 0.5):
    for _tag, _K, _mt, _env, _exp in (
            ('mode0', 64, None, NO_SAMPLE, dict(pipeline=V2, jmax=6, pad=0, ns=0, Tm=1, khead=0, fold=0)),
            ('head', 64, 40, NO_SAMPLE, dict(pipeline=V2, jmax=6, pad=0, ns=0, Tm=1, khead=32, fold=1)),
            ('nofold', 64, 40, NO_SAMPLE + (('SSDK_POST_NO_FOLD', '1'),), dict(pipeline=V2, jmax=6, pad=0, ns=0, Tm=1, khead=32, fold=0)),
            ('onepass', 64, 40, NO_SAMPLE + (('SSDK_NMS_ONE_PASS', '1'),), dict(pipeline=V2, jmax=6, pad=0, ns=0, Tm=1, khead=0, fold=0)),
            ('general', 200, 40, NO_SAMPLE, dict(pipeline=GENERAL)),
            ('greedy', None, 40, NO_SAMPLE, dict(pipeline=GREEDY))):
        _n = 'thr%g-%s' % (_t, _tag)
        _add(_n, 2, 200, 5, 1, _K, _mt, _t, _env, pairs=True, **_exp)
        THRESHOLDS.append(_n)

# ---- 6. max_per_class and max_total edges ----------------------------------------------------------------------------------------------------------
# K: sigmoid, 8 classes, A = 300, mt = 100: h = 8 ceil((500 / 16 = 31) / 8) = 32, 8 * 32 = 256 > 100; 2 h = 64 > K for K < 64: one pass; K = 64 .. 128:
# Khead = 32; K = 129 .. 256 > kWaveK: the general pipeline; K = 257 > kMaxPerClass: greedy.  tiles = 5: with the sample pass ns0 = 1 and 64 >= 4 K
# for K <= 16: ns = 1 (K = 1, 15, 16 run under both plans).
K_EDGES = []
for _K in (1, 15, 16, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257):
    _exp = dict(pipeline=V2, jmax=6, pad=1, ns=0, Tm=1, khead=32 if _K >= 64 else 0, fold=int(_K >= 64)) if _K <= 128 else \
        dict(pipeline=GENERAL if _K <= 256 else GREEDY)
    _add('K%d' % _K, 2, 300, 8, 0, _K, 100, 0.5, NO_SAMPLE, gen_kw=dict(scale=1.5, bias=1.0), boxes='spread', **_exp)
    K_EDGES.append('K%d' % _K)
    if _K <= 16:
        _add('K%d-sample' % _K, 2, 300, 8, 0, _K, 100, 0.5, SAMPLE, gen_kw=dict(scale=1.5, bias=1.0), boxes='spread', **dict(_exp, ns=1))
        K_EDGES.append('K%d-sample' % _K)
# mt: softmax, C = 21, A = 300, K = 100.  mt = 1: h = 16, 32 <= 100, 320 > 1: Khead = 16.  mt = 255: h = 8 ceil((1275 / 40 = 31) / 8) = 32;
# mt = 256: 1280 / 40 = 32: 32; 64 <= 100, 640 > 256.  mt = 257, 1024 > kMergeCap: the general pipeline (1024 = kSortCap, the largest it takes).
MT_EDGES = []
for _mt, _exp in ((1, dict(pipeline=V2, jmax=6, pad=0, ns=0, Tm=1, khead=16, fold=1)), (255, dict(pipeline=V2, jmax=6, pad=0, ns=0, Tm=1, khead=32, fold=1)),
                  (256, dict(pipeline=V2, jmax=6, pad=0, ns=0, Tm=1, khead=32, fold=1)), (257, dict(pipeline=GENERAL)), (1024, dict(pipeline=GENERAL))):
    _add('mt%d' % _mt, 2, 300, 21, 1, 100, _mt, 0.5, NO_SAMPLE, gen_kw=dict(scale=1.5), boxes='spread', **_exp)
    MT_EDGES.append('mt%d' % _mt)
# ncls * K at kMergeSlots = 8192 (64 sigmoid classes, K = 128: v2, JMAX 21 = ceil(64 / 4) = 16 <= 21; h = max(16, 8 ceil((500 / 128 = 3) / 8)) = 16,
# 32 <= 128, 1024 > 100) and one class beyond it (65: general).
SLOT_EDGES = ['slots-C64', 'slots-C65']
_add('slots-C64', 2, 200, 64, 0, 128, 100, 0.5, NO_SAMPLE, gen_kw=dict(protos=8, scale=1.5), pipeline=V2, jmax=21, pad=1, ns=0, Tm=1, khead=16, fold=1)
_add('slots-C65', 2, 200, 65, 0, 128, 100, 0.5, NO_SAMPLE, gen_kw=dict(protos=8, scale=1.5), pipeline=GENERAL)

# ---- 7. heavy ties across boundaries: A = 700 rows dealt from SIX prototype rows, sigmoid, 6 classes, spread boxes, SSDK_POST_WGS = 8 ----------------
# ~117 anchors share every score: the per-class top-K and the max_total cut fall inside runs of equal scores that span tiles, segments and the
# head.  tiles = 11 (the last of 60 rows), per_image = 8 / 2 = 4.  ties: K = 64, mt = 60, no sample pass: Tm = ceil(11 / 4) = 3, Gm = 4;
# h = 8 ceil((300 / 12 = 25) / 8) = 32, 64 <= 64, 192 > 60: Khead = 32.  ties-sample: K = 32: ns0 = 2, 128 >= 128: ns = 2 (Gs = 2, Ts = 1), tm = 9,
# Tm = 3, Gm = 3; 2 h = 64 > 32: one pass.
TIES = ['ties', 'ties-sample']
_add('ties', 2, 700, 6, 0, 64, 60, 0.45, NO_SAMPLE + (('SSDK_POST_WGS', '8'),), gen_kw=dict(protos=6, scale=1.5), boxes='spread', pipeline=V2, jmax=6, pad=1,
     ns=0, Gm=4, Tm=3, khead=32, fold=1)
_add('ties-sample', 2, 700, 6, 0, 32, 60, 0.45, SAMPLE + (('SSDK_POST_WGS', '8'),), gen_kw=dict(protos=6, scale=1.5), boxes='spread', pipeline=V2, jmax=6,
     pad=1, ns=2, Gs=2, Ts=1, Gm=3, Tm=3, khead=0, fold=0)

# ---- 8. more than 96 classes: the general pipeline with hard NMS, K = 100, mt = 200 -------------------------------------------------------------------
WIDE = []
for _C in (97, 130):
    for _soft in (0, 1):
        _n = 'wide-%s-C%d' % ('softmax' if _soft else 'sigmoid', _C)
        _add(_n, 2, 200, _C, _soft, 100, 200, 0.5, NO_SAMPLE, gen_kw=dict(protos=8, scale=1.5), pipeline=GENERAL)
        WIDE.append(_n)

# through the Python wrapper (its `cap` and workspace sizing) as well
WRAPPER = ['sweep-softmax-C25-sample', 'sweep-sigmoid-C96-nosample', 'thr0.7-mode0', 'thr0.35-greedy', 'K256', 'mt1024', 'wide-softmax-C97', 'lengths']
# called twice in a row and once more after a call of another shape (the hot bound of the plan without a sample pass)
HOT = ['lengths', 'long', 'ties']
