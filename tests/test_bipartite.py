"""CPU: the numpy restatement of bipartite matching (tests/bipartite_cases.py) equals the reference's own outputs
(tests/golden/bipartite.npz), which is what lets the GPU tests check randomised cases against it; and the host-side argument checks
of the new entry points."""
import ctypes

import numpy as np
import pytest

import bipartite_cases as bc
from single_shot_detection_amd import _lib


@pytest.fixture(scope='module')
def golden():
    return bc.load_golden()


@pytest.mark.parametrize('name', list(bc.MATRIX_CASES))
def test_matrix_restatement_equals_the_reference(golden, name):
    w = bc.MATRIX_CASES[name]()
    anchor_idx, left = bc.match_bipartite_np(w)
    ref = golden[f'matrix/{name}/anchor_idx']
    assert np.array_equal(golden[f'matrix/{name}/box_idx'], np.arange(w.shape[0]))
    if name in bc.EXHAUSTED:
        defined = golden[f'matrix/{name}/defined']
        assert not defined.all() and defined[0] and ref[0] == 0     # the reference's quirk: the left-over rounds land on (0, 0)
        assert np.array_equal(anchor_idx[defined], ref[defined])
        assert (anchor_idx[~defined] == -1).all()
    else:
        assert np.array_equal(anchor_idx, ref)
        assert len(set(anchor_idx.tolist())) == w.shape[0]          # every box an anchor of its own
    assert np.array_equal(left.view(np.uint32), golden[f'matrix/{name}/inplace'].view(np.uint32))


@pytest.mark.parametrize('name', list(bc.FUSED_CASES))
def test_fused_restatement_equals_the_reference(golden, name):
    gt, anchors, mt, ut = bc.fused_inputs(name)
    assert np.array_equal(bc.encode_bipartite_np(gt, anchors, mt, ut), golden[f'fused/{name}/box_idx'])


def test_fused_restatement_stops_at_exhaustion_and_leaves_box_0_alone():
    iou = np.array([[0.1, 0.9, 0, 0], [0, 0, 0.6, 0], [0, 0, 0.4, 0]], np.float32)
    assert bc.force_bipartite_np(iou).tolist() == [1, 2, -1]
    assert bc.match_bipartite_np(iou)[0].tolist() == [0, 2, -1]     # the matrix form: box 0 is moved to anchor 0


def test_unknown_force_match_is_refused_at_construction():
    from single_shot_detection_amd.detection.target_assigner import TargetAssigner
    with pytest.raises(ValueError):
        TargetAssigner(.5, .5, force_match='x')
    assert TargetAssigner(.5, .5).force_match == 'per_prediction'
    assert TargetAssigner(.5, .4, force_match='bipartite').force_match == 'bipartite'


def _refused(status, entry):
    assert status < 0
    assert entry.encode() in _lib.lib().ssdk_last_error_string()


def test_match_bipartite_refuses_bad_arguments_before_any_launch():
    """Host-only, as tests/test_abi.py: the pointers are never dereferenced."""
    lib = _lib.lib()
    p = ctypes.c_void_p(256)   # a non-null pointer that is never used
    need = lib.ssdk_match_bipartite_workspace_bytes(3, 5)
    assert need >= 3 * 5 * 4 + 3 * 8 + 3 * 4
    _refused(lib.ssdk_match_bipartite(None, 3, 5, 0, p, p, p, need, None), 'ssdk_match_bipartite')
    _refused(lib.ssdk_match_bipartite(p, 3, 5, 0, None, p, p, need, None), 'ssdk_match_bipartite')
    _refused(lib.ssdk_match_bipartite(p, 3, 5, 0, p, None, p, need, None), 'ssdk_match_bipartite')
    _refused(lib.ssdk_match_bipartite(p, 0, 5, 0, p, p, p, need, None), 'ssdk_match_bipartite')
    _refused(lib.ssdk_match_bipartite(p, -1, 5, 1, p, p, p, need, None), 'ssdk_match_bipartite')
    _refused(lib.ssdk_match_bipartite(p, 3, 0, 0, p, p, p, need, None), 'ssdk_match_bipartite')
    _refused(lib.ssdk_match_bipartite(p, 3, 5, 0, p, p, p, need - 1, None), 'ssdk_match_bipartite')
    _refused(lib.ssdk_match_bipartite(p, 3, 5, 0, p, p, None, need, None), 'ssdk_match_bipartite')


def test_encode_ground_truth_ex_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)
    for mode in (0, 1):
        need = lib.ssdk_encode_ground_truth_ex_workspace_bytes(2, 7, mode)
        assert need >= lib.ssdk_encode_ground_truth_workspace_bytes(2, 7)

        def call(rows=p, stride=6, offs=p, batch=2, total=7, anchors=p, num_anchors=100, mt=.5, ut=.5, force=mode, target=p, ws=p, nbytes=need):
            return lib.ssdk_encode_ground_truth_ex(rows, stride, offs, batch, total, anchors, num_anchors, mt, ut, force, target, None, ws, nbytes, None)
        entry = 'ssdk_encode_ground_truth_ex' if mode else 'ssdk_encode_ground_truth'   # (mode 0 IS ssdk_encode_ground_truth)
        _refused(call(rows=None), entry)
        _refused(call(offs=None), entry)
        _refused(call(anchors=None), entry)
        _refused(call(target=None), entry)
        _refused(call(batch=0), entry)
        _refused(call(num_anchors=0), entry)
        _refused(call(total=-1), entry)
        _refused(call(stride=5), entry)
        _refused(call(mt=.4, ut=.5), entry)
        _refused(call(ws=None), entry)
        _refused(call(nbytes=need - 1), entry)
    _refused(call(force=2), 'ssdk_encode_ground_truth_ex')
    _refused(call(num_anchors=262145), 'ssdk_encode_ground_truth_ex')
    assert lib.ssdk_encode_ground_truth_ex_workspace_bytes(2, 7, 1) > lib.ssdk_encode_ground_truth_ex_workspace_bytes(2, 7, 0)
