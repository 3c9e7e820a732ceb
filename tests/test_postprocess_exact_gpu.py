"""csrc/postprocess.hip through the C ABI on the DECIDABLE inputs of tests/postprocess_cases.py: integer boxes (corners, areas,
intersections and unions exact in fp32) and logit rows dealt from a few prototypes (equal scores are bit-equal, unequal ones at least
1e-4 apart, none near the score threshold, no IoU near the NMS threshold but the pairs built onto it).  Nothing is then decided by the last
ulp of an exp(), so the result must be the oracle's row for row: compare() WITHOUT boundaries, class ids exact, boxes np.array_equal,
scores 1e-5 relative, nms_candidates equal.

Buffers as in test_conv_exact_gpu.py: scores, locs and priors inside allocations with NaN on both sides (scores also at pointers 4, 8 and 12
bytes off 16-byte alignment, which the ABI allows); out, counts and nms_candidates between sentinels that must keep their bits; out_cap the
smallest the header allows; the workspace exactly ssdk_postprocess_workspace_bytes_ex bytes with 0xA5 behind it.

Which select / NMS / merge instantiation a case runs is worked out in the comments of postprocess_cases.py and checked against the library's own
dispatch functions, without a device, by test_postprocess_cases.py (DESIGN.md section 27 has the table).  Every case pins the plan with
SSDK_POST_SAMPLE / SSDK_POST_NO_SAMPLE: without one of them the plan of a call depends on what ran before it in the process."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import postprocess_cases as pc
from single_shot_detection_amd import _lib
from single_shot_detection_amd.detection.box_coder import BoxCoder
from single_shot_detection_amd.detection.postprocessor import Postprocessor
from test_postprocess_gpu import compare

pytestmark = pytest.mark.gpu

OK, E_UNSUPPORTED = 0, -3   # include/ssdk.h
F32 = np.float32
PAGE = 1024   # elements
SENTINEL = {np.dtype(np.float32): F32(-1234.5), np.dtype(np.int32): np.int32(-1234567), np.dtype(np.int64): np.int64(-1234567)}

_alive = []


@pytest.fixture(autouse=True)
def _device_buffers_live_until_the_test_ends():
    """The library is handed raw pointers: everything made here stays alive until the test is over."""
    yield
    torch.cuda.synchronize()
    del _alive[:]


def _keep(t):
    _alive.append(t)
    return t


def _guarded_input(a, shift=0):
    """Device address of `a` (fp32) inside an allocation that is NaN for 4 KiB on both sides; `shift` floats off 16-byte alignment."""
    a = np.ascontiguousarray(a, F32).ravel()
    host = np.full(2 * PAGE + a.size + shift, np.nan, F32)
    host[PAGE + shift:PAGE + shift + a.size] = a
    t = _keep(torch.from_numpy(host).cuda())
    assert t.data_ptr() % 16 == 0
    return C.c_void_p(t.data_ptr() + 4 * (PAGE + shift))


class _Output(object):
    """`n` elements of `dtype` between sentinels, pre-filled with `fill` (None: the sentinel itself -- a call that must write nothing)."""

    def __init__(self, n, dtype, fill=None):
        self.n, self.dtype = int(n), np.dtype(dtype)
        host = np.full(self.n + 2 * PAGE, SENTINEL[self.dtype], self.dtype)
        if fill is not None:
            host[PAGE:PAGE + self.n] = fill
        self.before = host.copy()
        self.t = _keep(torch.from_numpy(host).cuda())
        self.ptr = C.c_void_p(self.t.data_ptr() + host.itemsize * PAGE)

    def read(self):
        """The payload, after checking that the bytes around it are the ones put there."""
        torch.cuda.synchronize()
        got = self.t.cpu().numpy()
        bits = {4: np.uint32, 8: np.uint64}[self.dtype.itemsize]
        assert np.array_equal(got[:PAGE].view(bits), self.before[:PAGE].view(bits)), 'bytes in front of an output were written'
        assert np.array_equal(got[PAGE + self.n:].view(bits), self.before[PAGE + self.n:].view(bits)), 'bytes behind an output were written'
        return got[PAGE:PAGE + self.n].copy()

    def untouched(self):
        bits = {4: np.uint32, 8: np.uint64}[self.dtype.itemsize]
        return np.array_equal(self.read().view(bits), self.before[PAGE:PAGE + self.n].view(bits))


def _workspace(nbytes):
    """A workspace of exactly nbytes with 4 KiB of 0xA5 behind it; returns (pointer, checker)."""
    t = _keep(torch.full((int(nbytes) + 4096,), 0xA5, dtype=torch.uint8, device='cuda'))

    def check():
        torch.cuda.synchronize()
        assert bool((t[int(nbytes):] == 0xA5).all().item()), 'bytes behind the workspace were written'
    return C.c_void_p(t.data_ptr()), check


def _err():
    return _lib.lib().ssdk_last_error_string().decode('utf-8', 'replace')


class _Call(object):
    """The device buffers of one case; run() may be repeated on them (the outputs are then overwritten)."""

    def __init__(self, case, max_total='same', sentinel_outputs=False):
        s = self.spec = case.spec
        self.mt = (s.mt or 0) if max_total == 'same' else max_total
        self.cap = pc.out_cap(s)
        self.scores = _guarded_input(case.logits, s.shift)
        self.locs = _guarded_input(case.locs)
        self.priors = _guarded_input(case.priors)
        self.out = _Output(s.B * self.cap * 6, np.float32, None if sentinel_outputs else np.nan)
        self.counts = _Output(s.B, np.int32, None if sentinel_outputs else -1)
        self.cand = _Output(s.B, np.int64, None if sentinel_outputs else -1)
        lib = _lib.lib()
        self.ws_bytes = lib.ssdk_postprocess_workspace_bytes_ex(s.B, s.A, s.C, int(s.softmax), s.K or 0, min(self.mt, 1024), 0)
        assert self.ws_bytes > 0
        self.ws, self.ws_check = _workspace(self.ws_bytes)

    def launch(self):
        s = self.spec
        return _lib.lib().ssdk_postprocess(self.scores, self.locs, self.priors, s.B, s.A, s.C, int(s.softmax), s.thr, s.K or 0, s.nms_thr, 0, 0.5, self.mt,
                                           10.0, 5.0, self.out.ptr, self.cap, self.counts.ptr, self.cand.ptr, self.ws, self.ws_bytes, _lib.current_stream())

    def run(self):
        rc = self.launch()
        assert rc == OK, (self.spec.name, rc, _err())
        counts = self.counts.read()
        assert ((counts >= 0) & (counts <= self.cap)).all(), (self.spec.name, counts)
        out = self.out.read().reshape(self.spec.B, self.cap, 6)
        cand = self.cand.read()
        self.ws_check()
        return [out[i, :counts[i]] for i in range(self.spec.B)], cand


@functools.lru_cache(maxsize=None)
def reference(name):
    """oracle.postprocess of the case, once per session."""
    rows, cand = pc.oracle_rows(pc.build(name))
    for r in rows:
        r.setflags(write=False)
    cand.setflags(write=False)
    return rows, cand


def _by_class_and_box(rows):
    return rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0], rows[:, 4]))]


def check(name, got, cand):
    ref, ref_cand = reference(name)
    for i, (o, r) in enumerate(zip(got, ref)):
        assert o.shape == r.shape, (name, i, o.shape, r.shape)
        assert not np.isnan(o).any(), (name, i, 'a row the count covers was not written')
    compare(got, ref)   # order, class ids, scores to 1e-5 relative: strict, no selection boundary is excused
    for i, (o, r) in enumerate(zip(got, ref)):
        a, b = _by_class_and_box(o), _by_class_and_box(r)
        assert np.array_equal(a[:, :5], b[:, :5]), (name, i, 'class ids / boxes differ', int((a[:, :5] != b[:, :5]).any(1).sum()))
        assert np.allclose(a[:, 5], b[:, 5], rtol=1e-5, atol=0), (name, i)
    assert np.array_equal(cand, ref_cand), (name, cand, ref_cand)


def run_case(name, monkeypatch):
    case = pc.build(name)
    pc.set_env(monkeypatch, case.spec)
    got, cand = _Call(case).run()
    check(name, got, cand)


# ---- every class count ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('first', range(1, 98, 16))
@pytest.mark.parametrize('plan', ['sample', 'nosample'])
@pytest.mark.parametrize('converter', ['sigmoid', 'softmax'])
def test_every_class_count(converter, plan, first, monkeypatch):
    """C = first .. first + 15 (1 .. 97 sigmoid, 2 .. 97 softmax): the four JMAX x pad x converter instantiations of post_select2_kernel under
    the sample plan (post_tau_kernel + the mode-1 / mode-2 select) and the plan without, and the hand-over to the general pipeline at C = 97."""
    for C_ in range(first, min(first + 16, 98)):
        name = 'sweep-%s-C%d-%s' % (converter, C_, plan)
        if name in pc.SPECS:   # (softmax has no C = 1)
            run_case(name, monkeypatch)
    assert converter == 'softmax' or 'sweep-sigmoid-C1-' + plan in pc.SPECS


# ---- alignment and tile edges --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C_', [3, 21, 25, 80, 95])
def test_alignment_and_tile_edges(C_, monkeypatch):
    """One workgroup per image walks all tiles (SSDK_POST_WGS = 3 at batch 3): full, one-row and partial last tiles; images that start off 16-byte
    alignment (odd A * C); a scores pointer 4, 8 and 12 bytes off; A = 777 also with the sample pass."""
    names = [n for n in pc.ALIGN if n.startswith('align-C%d-' % C_)]
    assert len(names) >= 7
    for name in names:
        run_case(name, monkeypatch)


# ---- the select kernel's survivor queue, list lengths, ties, class counts above 96 ------------------------------------------------------------------

@pytest.mark.parametrize('name', pc.QUEUE + pc.LENGTHS + pc.TIES + pc.WIDE + pc.SLOT_EDGES)
def test_case(name, monkeypatch):
    run_case(name, monkeypatch)


# ---- NMS thresholds with odd and even last mantissa bit, the on-threshold pairs among ordinary boxes -------------------------------------------------

@pytest.mark.parametrize('form', ['mode0', 'head', 'nofold', 'onepass', 'general', 'greedy'])
@pytest.mark.parametrize('thr', [0.35, 0.4, 0.55, 0.7, 0.3, 0.45, 0.5])
def test_nms_threshold(thr, form, monkeypatch):
    name = 'thr%g-%s' % (thr, form)
    run_case(name, monkeypatch)
    if form == 'mode0':   # no max_total: the fate of every pair's b is in the output itself (the oracle's is checked by hand on the CPU)
        case = pc.build(name)
        cor = pc.corners(case)
        pc.set_env(monkeypatch, case.spec)
        got, _ = _Call(case).run()
        for rows in got:
            have = {tuple(int(v) for v in r[:4]) for r in rows if r[4] == pc.PAIR_CLASS + 1}
            for k, (ia, ib) in enumerate(case.pair_anchors):
                kept = not (F32(pc.PAIRS[k][2]) / F32(pc.PAIRS[k][3]) > F32(thr))
                assert tuple(cor[ia]) in have and (tuple(cor[ib]) in have) == kept, (name, k)


# ---- max_per_class and max_total edges -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', pc.K_EDGES + pc.MT_EDGES)
def test_max_per_class_and_max_total_edges(name, monkeypatch):
    run_case(name, monkeypatch)


def test_max_total_above_the_sort_capacity_is_refused_and_nothing_is_written(monkeypatch):
    case = pc.build('mt1024')
    pc.set_env(monkeypatch, case.spec)
    call = _Call(case, max_total=1025, sentinel_outputs=True)
    call.cap = 1025
    assert call.launch() == E_UNSUPPORTED and '1025' in _err()
    assert call.out.untouched() and call.counts.untouched() and call.cand.untouched()
    call.ws_check()
    out = (C.c_longlong * 16)()
    s = case.spec
    assert _lib.lib().ssdk_debug_postprocess_plan(s.B, s.A, s.C, 1, s.K, s.nms_thr, 0, 1025, 0, out) == E_UNSUPPORTED


# ---- the hot bound a call leaves for the next one ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', pc.HOT)
def test_hot_bound_of_the_previous_call_never_changes_results(name, monkeypatch):
    """The plan without a sample pass files keys by the per-class bound the previous call on the stream left (HotState): first call (no
    bound), the same call again (its own bound: the hot view holds exactly the head), a call of another shape (re-keys the state), then once
    more (no bound again) and again -- every result is the oracle's."""
    case, other = pc.build(name), pc.build('K64')
    pc.set_env(monkeypatch, case.spec)
    assert dict(case.spec.env).get('SSDK_POST_NO_SAMPLE') == '1' and dict(case.spec.expect)['khead'] > 0 and dict(other.spec.expect)['khead'] > 0
    call, call_other = _Call(case), _Call(other)
    for c in (call, call, call_other, call, call):
        got, cand = c.run()
        check(c.spec.name, got, cand)


# ---- through the Python wrapper ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', pc.WRAPPER)
def test_through_the_postprocessor(name, monkeypatch):
    """Postprocessor sizes `cap` and the workspace itself."""
    case = pc.build(name)
    s = case.spec
    pc.set_env(monkeypatch, s)
    nms = {'overlap_threshold': s.nms_thr}
    if s.K is not None:
        nms['max_per_class'] = s.K
    post = Postprocessor(BoxCoder(10.0, 5.0), score_threshold=s.thr, nms=nms, score_converter='SOFTMAX' if s.softmax else 'SIGMOID', max_total=s.mt)
    out = post.postprocess((torch.tensor(case.logits).cuda(), torch.tensor(case.locs).cuda()), torch.tensor(case.priors).cuda())
    check(name, [o.cpu().numpy() for o in out], post.last_nms_candidates.cpu().numpy())
