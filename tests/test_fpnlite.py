"""CPU: the FPN-lite neck's depthwise Conv2dBn blocks (bf/modules/features.py:79-98) pick the libssdk line, the variants outside the stencils are
still named, the two entry points behind the blocks refuse bad arguments on the host before any launch, and the golden file holds what
tests/fpnlite_cases.py writes (no GPU needed)."""
import ctypes
import os
import types

import numpy as np
import pytest

import fpnlite_cases
from blocks_cases import _StubBase
from conftest import GOLDEN
from single_shot_detection_amd import _lib
from single_shot_detection_amd.bf.modules import conv, features

MODS = types.SimpleNamespace(FeaturePyramid=features.FeaturePyramid)
INVALID = -1


def _buf(n=4096, dtype=np.float32):
    b = np.zeros(n, dtype)
    return b, ctypes.c_void_p(b.ctypes.data)


def _off(p, nbytes):
    return ctypes.c_void_p(p.value + nbytes)


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    keep, p = _buf()
    keep_q, q = _buf()
    keep_s, s = _buf(64, np.float64)
    stats, norm = lib.ssdk_depthwise_conv2d_stats_fwd, lib.ssdk_depthwise_conv2d_norm_fwd
    name_s, name_n = b'ssdk_depthwise_conv2d_stats_fwd', b'ssdk_depthwise_conv2d_norm_fwd'
    # (x, w, bias, batch, hin, win, channels, ksize, stride, pad, ...)
    bad_shapes = [(2, 5, 5, 6, 3, 1, 1),    # channels % 4
                  (2, 5, 5, 8, 7, 1, 3),    # ksize <= 5
                  (2, 5, 5, 8, 3, 0, 1),    # stride >= 1
                  (2, 2, 5, 8, 3, 2, 0),    # a kernel larger than the unpadded map
                  (0, 5, 5, 8, 3, 1, 1)]    # empty batch
    for shape in bad_shapes:
        assert stats(p, p, None, *shape, q, s, None) == INVALID, shape
        assert name_s in lib.ssdk_last_error_string()
        assert norm(p, p, None, *shape, p, p, p, p, 1e-5, 1, q, None) == INVALID, shape
        assert name_n in lib.ssdk_last_error_string()
    ok = (2, 5, 5, 8, 3, 1, 1)
    # null y / sums / running statistics, null x and w
    assert stats(p, p, None, *ok, None, s, None) == INVALID and name_s in lib.ssdk_last_error_string()
    assert stats(p, p, None, *ok, q, None, None) == INVALID and name_s in lib.ssdk_last_error_string()
    assert stats(None, p, None, *ok, q, s, None) == INVALID and stats(p, None, None, *ok, q, s, None) == INVALID
    assert norm(p, p, None, *ok, p, p, p, p, 1e-5, 1, None, None) == INVALID and name_n in lib.ssdk_last_error_string()
    assert norm(p, p, None, *ok, p, p, None, p, 1e-5, 1, q, None) == INVALID and norm(p, p, None, *ok, p, p, p, None, 1e-5, 1, q, None) == INVALID
    assert norm(None, p, None, *ok, p, p, p, p, 1e-5, 1, q, None) == INVALID
    # 16-byte alignment of the maps, the bias and the per-channel vectors
    assert stats(_off(p, 4), p, None, *ok, q, s, None) == INVALID and stats(p, p, None, *ok, _off(q, 8), s, None) == INVALID
    assert stats(p, p, _off(p, 4), *ok, q, s, None) == INVALID and name_s in lib.ssdk_last_error_string()
    assert norm(p, p, None, *ok, _off(p, 4), p, p, p, 1e-5, 1, q, None) == INVALID and norm(p, p, None, *ok, p, p, p, _off(p, 8), 1e-5, 1, q, None) == INVALID
    assert norm(p, p, None, *ok, p, p, p, p, 1e-5, 1, _off(q, 4), None) == INVALID and name_n in lib.ssdk_last_error_string()
    # nothing was written
    assert not keep.any() and not keep_q.any() and not keep_s.any()


def test_golden_file_holds_what_the_cases_write():
    path = os.path.join(GOLDEN, 'fpn_lite.npz')
    z = np.load(path)
    assert sorted(z['cases']) == sorted(fpnlite_cases.CASES)
    have = set()
    for k in z.files:
        if k == 'cases':
            continue
        for suffix in fpnlite_cases.SUFFIXES:
            if k.endswith(suffix):
                k = k[:-len(suffix)]
        have.add(k)
        assert z[k if k in z.files else k + '__samples'].dtype != object
    want = set()
    for name in fpnlite_cases.CASES:
        want |= fpnlite_cases.expected_keys(name, MODS)   # (our module tree: the state_dict names are the reference's)
    assert have == want, sorted(have ^ want)[:10]
    for k in z.files:   # a sampled array comes with its checksums and its shape
        if k.endswith('__samples'):
            assert k[:-9] + '__sum_l2' in z.files and k[:-9] + '__shape' in z.files
    for name, sizes in fpnlite_cases.LEVEL_SIZES.items():   # every level's size as the cases file states it
        for mode in ('eval', 'train'):
            for i, (h, w) in enumerate(sizes):
                key = f'{name}/{mode}/y{i}'
                shape = tuple(z[key + '__shape']) if key + '__shape' in z.files else z[key].shape
                assert shape == (2, 32, h, w), (key, shape)
    assert os.path.getsize(path) < 1_000_000


def _blk(cin=16, cout=16, k=3, groups=None, **kw):
    return conv.Conv2dBn(cin, cout, kernel_size=k, groups=cin if groups is None else groups, **kw)


@pytest.mark.parametrize('kw', [dict(padding=1), dict(stride=2), dict(stride=2, padding=1), dict(k=5, padding=2), dict(k=1), dict(padding=1, use_bn=False),
                                dict(padding=1, activation_params=None), dict(padding=1, bias=True), dict(cin=132, cout=132, padding=1)])
def test_depthwise_blocks_take_the_libssdk_line(kw):
    b = _blk(**kw)
    assert b._is_depthwise() and b._why_not_hip() is None and b._hip_ok()
    assert b.conv.weight.is_contiguous()   # [C][1][k][k] as torch made it: what the stencil reads


def test_every_block_of_the_fpn_lite_neck_takes_the_libssdk_line():
    for mode in ('nearest', 'bilinear'):
        m = features.FeaturePyramid(_StubBase(), (1, 3, 4), pyramid_layers=5, pyramid_channels=32, use_depthwise=True, interpolation_mode=mode)
        assert len(m.pyramid_output) == 5
        for i, b in enumerate(m.pyramid_output):
            assert b.conv.groups == 32 and b.conv.stride == ((1, 1) if i < 3 else (2, 2)) and b.conv.padding == (1, 1)
            assert b._why_not_hip() is None, (i, b._why_not_hip())


@pytest.mark.parametrize('kw,why', [(dict(groups=2, padding=1), 'groups=2'),
                                    (dict(cout=32, padding=1), 'groups=16 with a channel multiplier'),
                                    (dict(padding=1, activation_params={'name': 'ReLU6', 'args': {'inplace': True}}), 'activation ReLU6'),
                                    (dict(k=7, padding=3), 'kernel_size=(7, 7)'),
                                    (dict(cin=6, cout=6, padding=1), 'channels 6->6 not multiples of 4')])
def test_variants_outside_the_stencils_are_named(kw, why):
    b = _blk(**kw)
    assert not b._hip_ok() and b._why_not_hip().startswith(why), b._why_not_hip()


def test_dense_blocks_keep_their_rules():
    assert conv.Conv2dBn(16, 32, kernel_size=3, padding=1)._why_not_hip() is None
    assert conv.Conv2dBn(16, 32, kernel_size=5, padding=2)._why_not_hip().startswith('kernel_size=(5, 5)')   # (5 x 5 is the stencil's alone)
    assert conv.Conv2dBn(16, 32, kernel_size=3, padding=1).conv.weight.is_contiguous(memory_format=__import__('torch').channels_last)
