"""CPU: the float64 model of bilinear resizing (tests/bilinear_reference.py) against torch's own F.interpolate and its backward for every
pair of sizes 1..48, within the bounds the GPU kernels are held to; the two libssdk entry points refuse bad arguments on the host, before
any launch; ops refuses a mode that is not on libssdk; the reference-golden file holds what tests/bilinear_cases.py writes."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bilinear_cases
import bilinear_reference as br
from conftest import GOLDEN
from single_shot_detection_amd import _lib, ops
from single_shot_detection_amd.bf.modules import features

SIZES = range(1, 49)


def _pairs(axis):
    """Every pair 1..48 (both directions) along `axis`, the other axis small: 1 -> 4 and 7 -> 10.  Yields hc, wc, hf, wf."""
    for other_in, other_out in ((1, 4), (7, 10)):
        for n_in in SIZES:
            for n_out in SIZES:
                yield (n_in, other_in, n_out, other_out) if axis == 0 else (other_in, n_in, other_out, n_out)


@pytest.mark.parametrize('axis', [0, 1])
def test_model_equals_torch_cpu_forward_and_backward_for_every_size_pair(axis):
    """torch's fp32 CPU kernels stay inside the bounds the GPU kernels get (measured: below 0.31 of the forward and 0.02 of the backward
    bound), so the model is torch's function and the bounds are not loose by orders of magnitude in the other direction."""
    rng = np.random.default_rng(11 + axis)
    worst_f = worst_b = 0.0
    for hc, wc, hf, wf in _pairs(axis):
        x = rng.standard_normal((1, 2, hc, wc), dtype=np.float32)
        g = rng.standard_normal((1, 2, hf, wf), dtype=np.float32)
        xt = torch.from_numpy(x).requires_grad_(True)
        yt = F.interpolate(xt, size=(hf, wf), mode='bilinear')
        yt.backward(torch.from_numpy(g))
        ef = np.abs(yt.detach().numpy() - br.forward(x, hf, wf)).max() / br.forward_bound(hc, wc, np.abs(x).max())
        eb = np.abs(xt.grad.numpy() - br.backward(g, hc, wc)).max() / br.backward_bound(hc, wc, hf, wf, np.abs(g).max())
        assert ef <= 1.0 and eb <= 1.0, (hc, wc, hf, wf, ef, eb)
        worst_f, worst_b = max(worst_f, ef), max(worst_b, eb)
    print(f'axis {axis}: worst forward {worst_f:.3f}, worst backward {worst_b:.3f} of the bound')


def test_model_weights_sum_to_one_and_the_identity_is_exact():
    for n_in in SIZES:
        for n_out in SIZES:
            w = br.axis_matrix(n_in, n_out)
            assert np.abs(w.sum(axis=1) - 1.0).max() <= 1e-15 and (w >= 0).all()
        assert np.array_equal(br.axis_matrix(n_in, n_in), np.eye(n_in))
    assert np.array_equal(br.axis_matrix(2, 4), np.array([[1, 0], [.75, .25], [.25, .75], [0, 1]]))   # exact 2 x: weights 1/4 and 3/4


def _buf(n=4096):
    b = np.zeros(n, np.float32)
    return b, ctypes.c_void_p(b.ctypes.data)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    keep, p = _buf()
    keep2, q = _buf()
    fwd, bwd = lib.ssdk_upsample_bilinear_add_fwd, lib.ssdk_upsample_bilinear_add_bwd
    assert lib.ssdk_linspace_f32(0.0, 1.0, 0, None) < 0          # (another entry point's message is the last error now)
    assert fwd(p, p, 2, 4, 4, 2, 2, 6, q, None) < 0               # channels % 4
    assert b'ssdk_upsample_bilinear_add_fwd' in lib.ssdk_last_error_string()
    assert bwd(p, 2, 4, 4, 2, 2, 6, q, None) < 0
    assert b'ssdk_upsample_bilinear_add_bwd' in lib.ssdk_last_error_string()
    for sizes in ((0, 4, 2, 2), (4, 0, 2, 2), (4, 4, 0, 2), (4, 4, 2, 0), (-1, 4, 2, 2)):   # a zero / negative size
        assert fwd(p, p, 2, *sizes, 8, q, None) < 0, sizes
        assert bwd(p, 2, *sizes, 8, q, None) < 0, sizes
    assert fwd(p, p, 0, 4, 4, 2, 2, 8, q, None) < 0 and bwd(p, 0, 4, 4, 2, 2, 8, q, None) < 0   # batch
    assert fwd(p, p, 2, 4, 4, 2, 2, 0, q, None) < 0 and bwd(p, 2, 4, 4, 2, 2, 0, q, None) < 0   # channels
    assert fwd(p, None, 2, 4, 4, 2, 2, 8, q, None) < 0            # null pointers (fine alone may be NULL)
    assert fwd(p, p, 2, 4, 4, 2, 2, 8, None, None) < 0
    assert bwd(None, 2, 4, 4, 2, 2, 8, q, None) < 0
    assert bwd(p, 2, 4, 4, 2, 2, 8, None, None) < 0
    assert b'ssdk_upsample_bilinear_add_bwd' in lib.ssdk_last_error_string()


def test_ops_names_the_modes_that_exist():
    f, c = torch.zeros((1, 4, 4, 4)), torch.zeros((1, 4, 2, 2))
    for call in (lambda: ops.upsample_add(f, c, mode='bicubic'), lambda: ops.upsample(c, (4, 4), mode='bicubic'),
                 lambda: ops.upsample_add(f, c, 'area')):
        with pytest.raises(ValueError, match="'nearest' and 'bilinear'"):
            call()
    assert ops.UPSAMPLE_MODES == ('nearest', 'bilinear')


def test_golden_file_holds_what_the_cases_write():
    z = np.load(os.path.join(GOLDEN, 'necks_bilinear.npz'))
    assert sorted(z['cases']) == sorted(bilinear_cases.CASES)
    mods = types.SimpleNamespace(FeaturePyramid=features.FeaturePyramid, ThinnedUshapeModule=features.ThinnedUshapeModule,
                                 MultilevelFeaturePyramid=features.MultilevelFeaturePyramid)
    have = set()
    for k in z.files:
        if k == 'cases':
            continue
        for suffix in bilinear_cases.SUFFIXES:
            if k.endswith(suffix):
                k = k[:-len(suffix)]
        have.add(k)
        assert z[k if k in z.files else k + '__samples'].dtype != object
    want = set()
    for name in bilinear_cases.CASES:
        want |= bilinear_cases.expected_keys(name, mods)   # (our module tree: the state_dict names are the reference's)
    assert have == want, sorted(have ^ want)[:10]
    for k in z.files:   # a sampled array comes with its checksums and its shape
        if k.endswith('__samples'):
            assert k[:-9] + '__sum_l2' in z.files and k[:-9] + '__shape' in z.files and z[k].size == bilinear_cases.N_SAMPLES
    assert os.path.getsize(os.path.join(GOLDEN, 'necks_bilinear.npz')) < 1 << 20
