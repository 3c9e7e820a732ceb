"""CPU: the cases of tests/postprocess_cases.py are what their comments say -- decidable (the rule of that file), on the dispatch path the
comment's arithmetic puts them on (ssdk_debug_postprocess_plan: the functions ssdk_postprocess launches by, no device), and the pairs built
onto an NMS threshold end as worked out by hand.  tests/test_postprocess_exact_gpu.py runs the same cases on the GPU."""
import ctypes

import numpy as np
import pytest

import postprocess_cases as pc
from single_shot_detection_amd import _lib

E_UNSUPPORTED = -3


def case_plan(monkeypatch, spec):
    pc.set_env(monkeypatch, spec)
    rc, plan = pc.plan(_lib.lib(), spec)
    assert rc == 0, _lib.lib().ssdk_last_error_string()
    return plan


CHUNKS = [list(pc.SPECS)[i:i + 64] for i in range(0, len(pc.SPECS), 64)]


@pytest.mark.parametrize('chunk', range(len(CHUNKS)))
def test_every_case_is_decidable(chunk):
    for name in CHUNKS[chunk]:
        case = pc.build(name)          # (the first seed for which the rule holds ...)
        pc.assert_decidable(case)      # ... and the rule itself, said once more on what the tests will use
        assert case.logits.shape == (case.spec.B, case.spec.A * case.spec.C) and not case.locs.any()


def test_the_rule_rejects_what_it_should():
    """The checker is not vacuous: inputs bent onto each boundary are refused."""
    case = pc.build('thr0.5-head')
    s = case.spec
    p = pc.probabilities(case)
    # (a) a probability on the score threshold
    x = case.logits.reshape(s.B, s.A, s.C).copy()
    x[0, 5] = 0.0
    x[0, 5, 0] = np.float32(np.log(96.0))   # softmax over (x0, 0, 0, 0, 0): p of each class = 1 / (e^x0 + 4) = 0.01 up to the rounding of x0
    bent = case._replace(logits=x.reshape(s.B, -1))
    assert abs(pc.probabilities(bent)[0, 5, 0] - 0.01) < 1e-3 * 0.01 and pc.why_undecidable(bent).startswith('(a)')
    # (b) two different rows 1e-6 apart in one class
    i, c = 0, 2
    cand = np.nonzero(p[i, :, c] > 0.5)[0]
    x = case.logits.reshape(s.B, s.A, s.C).copy()
    x[i, cand[1]] = x[i, cand[0]]
    x[i, cand[1], c + 1] += np.float32(2e-6)
    ident = case.ident.copy()
    ident[i, cand[1]] = 777
    assert pc.why_undecidable(case._replace(logits=x.reshape(s.B, -1), ident=ident)).startswith('(b)')
    # (c) the 7 / 10 pair at threshold 0.7 is exempt only as THE on-threshold pair of a case: at 0.5 the case holds a pair at 1 / 2
    pri = case.priors.copy()
    pri[0] = (410, 410, 20, 20)
    pri[1] = (410, 405, 20, 10)
    assert pc.why_undecidable(case._replace(priors=pri)).startswith('(c)')
    # (d) two classes' best rows 5e-7 apart with max_total = 1 (three disjoint boxes, sigmoid, everything else far below the threshold)
    tiny = pc.Spec('tiny', 1, 3, 2, False, 16, 1, 0.5, 0.01, (), 0, 'deal', (), 'spread', False, ())
    x = np.full((1, 3, 2), -10.0, np.float32)
    x[0, 0, 0], x[0, 1, 1] = 2.0, np.float32(2.0) + np.float32(5e-6)
    pri = np.array([[410, 410, 20, 20], [510, 410, 20, 20], [610, 410, 20, 20]], np.float32)
    bent = pc.Case(tiny, 0, x.reshape(1, -1), None, np.zeros((1, 12), np.float32), pri, ())
    assert pc.why_undecidable(bent).startswith('(d)')
    x[0, 1, 1] = 2.5
    assert pc.why_undecidable(bent._replace(logits=x.reshape(1, -1))) is None


def test_threshold_parities():
    for thr, odd in pc.TIE_UP.items():
        assert int(np.float32(thr).view(np.uint32)) & 1 == odd, thr
    assert sum(pc.TIE_UP.values()) == 4 and len(pc.TIE_UP) == 7


@pytest.mark.parametrize('chunk', range(len(CHUNKS)))
def test_plan_of_every_case(chunk, monkeypatch):
    """pipeline, JMAX, pad, ns, Tm, khead, tie_up, fold (and whatever else a case states) as the comments of postprocess_cases.py work out."""
    for name in CHUNKS[chunk]:
        spec = pc.SPECS[name]
        plan = case_plan(monkeypatch, spec)
        want = dict(spec.expect)
        assert {k: plan[k] for k in want} == want, (name, plan)
        assert 'pipeline' in want and 'tie_up' in want
        if want['pipeline'] == pc.V2:
            assert {'jmax', 'pad', 'ns', 'Tm', 'khead', 'fold'} <= set(want), name
            assert plan['nseg'] == plan['Gs'] + plan['Gm'] and plan['list_cap'] == (plan['Gs'] * plan['Ts'] + plan['Gm'] * plan['Tm']) * 64
            assert plan['Gm'] * plan['Tm'] >= plan['tiles'] - plan['ns'] > (plan['Gm'] - 1) * plan['Tm']
    # the prefetch loop crosses tiles
    for name in pc.ALIGN:
        if pc.SPECS[name].A in (129, 777):
            assert dict(pc.SPECS[name].expect)['Tm'] >= 3


def test_plan_coverage(monkeypatch):
    """What the case list reaches, counted on the plans: every select instantiation, both tie_up values on each NMS launch form, the other
    two pipelines, both plans, a workgroup of several tiles."""
    plans = {name: case_plan(monkeypatch, spec) for name, spec in pc.SPECS.items()}
    v2 = [p for p in plans.values() if p['pipeline'] == pc.V2]
    assert {(p['softmax'], p['pad'], p['jmax']) for p in v2} == {(s, d, j) for s in (0, 1) for d in (0, 1) for j in (6, 12, 21, 24)}
    # ... each of them under both plans
    assert {(p['softmax'], p['pad'], p['jmax'], p['ns'] > 0) for p in v2} == {(s, d, j, n) for s in (0, 1) for d in (0, 1) for j in (6, 12, 21, 24)
                                                                           for n in (False, True)}
    mode0 = {p['tie_up'] for p in v2 if p['khead'] == 0}
    mode0_mt = {p['tie_up'] for n, p in plans.items() if p['pipeline'] == pc.V2 and p['khead'] == 0 and pc.SPECS[n].mt and 'onepass' in n}
    folded = {p['tie_up'] for p in v2 if p['khead'] > 0 and p['fold'] == 1}
    unfolded = {p['tie_up'] for p in v2 if p['khead'] > 0 and p['fold'] == 0}
    assert mode0 == mode0_mt == folded == unfolded == {0, 1}
    assert {p['tie_up'] for p in plans.values() if p['pipeline'] == pc.GENERAL} == {0, 1}
    assert {p['tie_up'] for p in plans.values() if p['pipeline'] == pc.GREEDY} == {0, 1}
    assert any(p['Tm'] > 1 and p['ns'] > 0 for p in v2) and any(p['Tm'] > 1 and p['ns'] == 0 for p in v2)
    assert {p['khead'] for p in v2} >= {0, 16, 32, 40}


def test_plan_query_honours_the_knobs_and_refuses_like_the_entry_point(monkeypatch):
    lib = _lib.lib()
    spec = pc.SPECS['ties-sample']
    out = (ctypes.c_longlong * 16)()
    args = (spec.B, spec.A, spec.C, 0, spec.K, spec.nms_thr, 0, spec.mt)
    for k in pc.ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    # no knob: the `sample` argument decides; 768 workgroups over 2 images: one tile per workgroup
    assert lib.ssdk_debug_postprocess_plan(*args, 1, out) == 0 and (out[5], out[9]) == (2, 1)
    assert lib.ssdk_debug_postprocess_plan(*args, 0, out) == 0 and (out[5], out[9]) == (0, 1)
    # < 0: the choice of the next call of this process; nothing has run in it, or the hint left by a call that has: either way a valid plan
    assert lib.ssdk_debug_postprocess_plan(*args, -1, out) == 0 and out[5] in (0, 2)
    monkeypatch.setenv('SSDK_POST_NO_SAMPLE', '1')
    assert lib.ssdk_debug_postprocess_plan(*args, 1, out) == 0 and out[5] == 0
    monkeypatch.delenv('SSDK_POST_NO_SAMPLE')
    monkeypatch.setenv('SSDK_POST_SAMPLE', '1')
    assert lib.ssdk_debug_postprocess_plan(*args, 0, out) == 0 and out[5] == 2
    monkeypatch.setenv('SSDK_POST_OLD', '1')
    assert lib.ssdk_debug_postprocess_plan(*args, 0, out) == 0 and out[0] == pc.GENERAL
    monkeypatch.delenv('SSDK_POST_OLD')
    # soft-NMS: never the v2 pipeline; max_per_class None or above 256: greedy, soft or not
    assert lib.ssdk_debug_postprocess_plan(spec.B, spec.A, spec.C, 0, spec.K, spec.nms_thr, 1, spec.mt, 0, out) == 0 and out[0] == pc.GENERAL
    assert lib.ssdk_debug_postprocess_plan(spec.B, spec.A, spec.C, 0, 0, spec.nms_thr, 1, spec.mt, 0, out) == 0 and out[0] == pc.GREEDY
    # refusals of the entry point that depend on the shape alone
    assert lib.ssdk_debug_postprocess_plan(spec.B, spec.A, spec.C, 0, spec.K, spec.nms_thr, 0, 1025, 0, out) == E_UNSUPPORTED
    assert b'1025' in lib.ssdk_last_error_string()
    assert lib.ssdk_debug_postprocess_plan(spec.B, spec.A, 1, 1, spec.K, spec.nms_thr, 0, spec.mt, 0, out) < 0   # softmax needs a class besides the background
    assert lib.ssdk_debug_postprocess_plan(*args, 0, None) < 0


# ---- the on-threshold pairs ----------------------------------------------------------------------------------------------------------------------

def _pair_case(k, thr):
    """The two boxes of PAIRS[k] alone: one class, a scores higher than b."""
    a, b = pc.PAIRS[k][0], pc.PAIRS[k][1]
    pri = np.array([pc._corner_to_centroid(a), pc._corner_to_centroid(b)], np.float32)
    import oracle
    rows = oracle.postprocess(np.array([[3.0, 2.0]], np.float32), np.zeros((1, 8), np.float32), pri, softmax=False, score_thr=0.01, max_per_class=100,
                              nms_thr=thr, max_total=200)[0]
    assert np.array_equal(rows[0, :4], np.array(a, np.float32))
    return len(rows) == 2


def test_on_threshold_pairs_by_hand():
    for (a, b, inter, union) in pc.PAIRS:
        iw, ih = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
        area = lambda r: (r[2] - r[0]) * (r[3] - r[1])   # noqa: E731
        assert iw * ih == inter and area(a) + area(b) - inter == union
    f = np.float32
    # 9 / 20: the quotient rounds to 0.45f, which lies BELOW 9 / 20 -- kept at 0.45 (RN(q) > thr is false), suppressed at 0.44
    assert f(45) / f(100) == f(0.45) and float(f(0.45)) < 45 / 100
    assert _pair_case(0, 0.45) and not _pair_case(0, 0.44)
    # 7 / 10: rounds to 0.7f (odd last bit) < 7 / 10 -- kept at 0.7, suppressed at 0.69
    assert f(70) / f(100) == f(0.7) and float(f(0.7)) < 70 / 100 and pc.TIE_UP[0.7] == 1
    assert _pair_case(1, 0.7) and not _pair_case(1, 0.69)
    # 7 / 20: rounds to 0.35f (odd) < 7 / 20 -- kept at 0.35, suppressed at 0.34
    assert f(140) / f(400) == f(0.35) and float(f(0.35)) < 140 / 400 and pc.TIE_UP[0.35] == 1
    assert _pair_case(2, 0.35) and not _pair_case(2, 0.34)
    # 11 / 20: rounds to 0.55f (odd) > 11 / 20: the exact quotient lies below the float threshold -- kept at 0.55, suppressed at 0.54
    assert f(220) / f(400) == f(0.55) and float(f(0.55)) > 220 / 400 and pc.TIE_UP[0.55] == 1
    assert _pair_case(3, 0.55) and not _pair_case(3, 0.54)
    assert pc.ON_THRESHOLD == {0.45: (0, True), 0.7: (1, True), 0.35: (2, True), 0.55: (3, True)}


@pytest.mark.parametrize('name', pc.THRESHOLDS)
def test_pairs_inside_the_threshold_cases(name):
    """Among ordinary boxes: a of every pair is in the oracle's output (mode0: no max_total cuts it), b exactly when RN(inter / union) > thr
    is false -- for the pair ON the case's threshold that is the hand-worked answer above."""
    case = pc.build(name)
    s = case.spec
    rows, _ = pc.oracle_rows(case, max_total=None)
    cor = pc.corners(case)
    for i in range(s.B):
        have = {tuple(int(v) for v in r[:4]) for r in rows[i] if r[4] == pc.PAIR_CLASS + 1}
        for k, (ia, ib) in enumerate(case.pair_anchors):
            assert tuple(cor[ia]) == pc.PAIRS[k][0] and tuple(cor[ib]) == pc.PAIRS[k][1]
            kept = not (np.float32(pc.PAIRS[k][2]) / np.float32(pc.PAIRS[k][3]) > np.float32(s.nms_thr))
            if pc.on_threshold_pair(s) == k:
                assert kept == pc.ON_THRESHOLD[s.nms_thr][1] is True
            assert tuple(cor[ia]) in have and (tuple(cor[ib]) in have) == kept, (name, i, k)


def test_tie_cases_cut_inside_runs_of_equal_scores():
    for name in pc.TIES:
        case = pc.build(name)
        s = case.spec
        rows, cand = pc.oracle_rows(case, max_total=s.mt + 8)
        assert any(len(r) > s.mt and r[s.mt - 1, 5] == r[s.mt, 5] and r[s.mt - 1, 4] == r[s.mt, 4] for r in rows), name   # the max_total cut
        p = pc.probabilities(case)
        for i in range(s.B):   # the per-class top-K: the K-th and the (K + 1)-th best candidate of every class are equal
            for c in range(p.shape[2]):
                v = np.sort(p[i, :, c][p[i, :, c] > s.thr])[::-1]
                assert len(v) > s.K and v[s.K - 1] == v[s.K], (name, i, c)


def test_list_lengths_are_what_the_case_says():
    case = pc.build('lengths')
    s = case.spec
    want = dict(s.gen_kw)['lengths']
    n = (pc.probabilities(case) > s.thr).sum(1)
    assert n[0].tolist() == list(want) and n[1].tolist() == [want[(c + 1) % s.C] for c in range(s.C)]
    khead = dict(s.expect)['khead']
    assert {0, 1, khead, khead + 1, 64, 65, 128, 129} <= set(want)
    assert ((pc.probabilities(pc.build('long')) > 0.01).sum(1) > 1024).all()
    dense = pc.probabilities(pc.build('queue-dense')) > 0.01
    assert dense.all()                                                   # every pair passes: 16 rows x 20 classes > 256 in every wave
    mixed = (pc.probabilities(pc.build('queue-mixed')) > 0.01).reshape(2, 200, 20)
    per_wave = [mixed[0, r:r + 16].sum() for r in range(0, 200, 16)]
    assert max(per_wave) > 256 and min(per_wave) <= 256 and per_wave[0] == 320
    sparse = (pc.probabilities(pc.build('queue-sparse')) > 0.01)
    assert max(sparse[0, r:r + 16].sum() for r in range(0, 200, 16)) <= 256
