"""CPU: DepthwiseFeaturePyramid (Tiny-DSOD D-FPN, bf/modules/features.py:123-212) builds with the reference's module tree, and the three
libssdk entry points behind it refuse bad arguments on the host, before any launch (no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import dfpn_cases
from blocks_cases import _StubBase
from conftest import GOLDEN
from single_shot_detection_amd import _lib
from single_shot_detection_amd.bf.modules import conv, features
from single_shot_detection_amd.detection import detector_builder


@pytest.fixture(scope='module')
def golden_dfpn():
    return np.load(os.path.join(GOLDEN, 'dfpn_small.npz'))


def test_builder_resolves_the_class_by_name():
    from single_shot_detection_amd import synthetic
    cfg = {'name': 'DepthwiseFeaturePyramid', 'out_layers': (1, 3, 4), 'pyramid_layers': 6, 'pyramid_channels': 32}
    det = detector_builder.build(_StubBase(), dict(synthetic.CONFIGS['ssd_mb2_voc']['anchor']), 21, cfg, use_depthwise=True)
    neck = det.predictor.features
    assert isinstance(neck, features.DepthwiseFeaturePyramid)
    assert neck.num_outputs == 6 and neck.get_out_channels() == [32] * 6
    assert len(neck.downsample) == 3 and len(neck.up_conv) == 5


@pytest.mark.parametrize('case', sorted(dfpn_cases.CASES))
def test_state_dict_names_and_shapes_are_the_references(case, golden_dfpn):
    m = dfpn_cases.build(features.DepthwiseFeaturePyramid, case)
    shapes = {n: tuple(t.shape) for n, t in m.state_dict().items() if not n.startswith('base.')}
    assert sorted(shapes) == list(golden_dfpn[f'{case}/state_names'])
    assert [str(shapes[n]) for n in sorted(shapes)] == list(golden_dfpn[f'{case}/state_shapes'])


def test_module_tree_outputs_and_reference_quirks():
    m = features.DepthwiseFeaturePyramid(_StubBase(), (1, 3, 4), pyramid_layers=6, pyramid_channels=32, initializer={'name': 'zeros_'})
    assert m.num_outputs == 6 and m.get_out_channels() == [32] * 6
    assert len(m.pyramid_lateral) == 3 and len(m.downsample) == 3 and len(m.up_conv) == 5
    assert [lat.in_channels for lat in m.pyramid_lateral] == [16, 24, 40] and all(lat.bias is not None for lat in m.pyramid_lateral)
    for paths in m.downsample:
        assert isinstance(paths[0][0], nn.MaxPool2d) and isinstance(paths[0][1], conv.Conv2dBn) and isinstance(paths[1], conv.DepthwiseConv2dBn)
        assert paths[0][1].conv.out_channels == 16 and paths[1].pointwise_conv.out_channels == 16
    for uc in m.up_conv:
        assert uc.conv.groups == 32 and uc.conv.kernel_size == (3, 3) and uc.conv.padding == (1, 1) and uc.conv.bias is None
    # features.py:133 does not hand `initializer` to Features: the weights are xavier_normal_, never the configured zeros_
    assert all(float(p.detach().abs().max()) > 0 for n, p in m.named_parameters() if n.endswith('conv.weight') or n.startswith('pyramid_lateral.') and n.endswith('weight'))
    assert m._stock_reason is None


@pytest.mark.parametrize('kw,why', [(dict(activation={'name': 'ReLU6', 'args': {'inplace': True}}), 'activation ReLU6'),
                                    (dict(interpolation_mode='bilinear'), "interpolation_mode='bilinear'"),
                                    (dict(pyramid_channels=12), 'pyramid_channels=12')])
def test_variants_outside_the_kernels_are_named(kw, why):
    args = dict(out_layers=(1, 3, 4), pyramid_layers=4, pyramid_channels=16)
    args.update(kw)
    m = features.DepthwiseFeaturePyramid(_StubBase(), **args)
    assert m._stock_reason is not None and m._stock_reason.startswith(why)


def _buf(n=4096):
    b = np.zeros(n, np.float32)
    return b, ctypes.c_void_p(b.ctypes.data)


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    keep, p = _buf()
    _, q = _buf()
    # channels % 4
    assert lib.ssdk_maxpool2x2_fwd(p, 2, 8, 8, 6, 1, 1, q, None) < 0
    assert b'ssdk_maxpool2x2_fwd' in lib.ssdk_last_error_string()
    assert lib.ssdk_maxpool2x2_bwd(p, p, 2, 8, 8, 6, 1, 1, q, None) < 0
    # a zero-sized pooled output: a 1-row map without a pad row (features.py pads only maps larger than 2)
    assert lib.ssdk_maxpool2x2_fwd(p, 2, 1, 8, 8, 0, 1, q, None) < 0
    assert b'zero-sized' in lib.ssdk_last_error_string()
    assert lib.ssdk_maxpool2x2_fwd(p, 2, 8, 1, 8, 1, 0, q, None) < 0
    assert lib.ssdk_maxpool2x2_bwd(p, p, 2, 1, 1, 8, 0, 0, q, None) < 0
    assert lib.ssdk_maxpool2x2_fwd(p, 2, 8, 8, 8, 2, 1, q, None) < 0   # pads are 0 or 1
    # concat: channels % 4, piece count
    ptrs = (ctypes.c_void_p * 2)(p.value, p.value)
    assert lib.ssdk_concat_channels_fwd(ptrs, (ctypes.c_int * 2)(16, 6), 2, 10, q, None) < 0
    assert b'ssdk_concat_channels_fwd' in lib.ssdk_last_error_string()
    assert lib.ssdk_concat_channels_fwd(ptrs, (ctypes.c_int * 2)(16, 16), 0, 10, q, None) < 0
    assert lib.ssdk_concat_channels_bwd(p, (ctypes.c_int * 2)(16, 10), 2, 10, ptrs, None) < 0
    nine = (ctypes.c_void_p * 9)(*([p.value] * 9))
    assert lib.ssdk_concat_channels_fwd(nine, (ctypes.c_int * 9)(*([4] * 9)), 9, 10, q, None) < 0
    # up-sampled depthwise: channels % 4, empty maps
    assert lib.ssdk_depthwise_upsample_conv2d_fwd(p, p, None, 2, 5, 5, 10, 10, 6, q, None) < 0
    assert b'ssdk_depthwise_upsample_conv2d_fwd' in lib.ssdk_last_error_string()
    assert lib.ssdk_depthwise_upsample_conv2d_fwd(p, p, None, 2, 0, 5, 10, 10, 8, q, None) < 0
    assert lib.ssdk_depthwise_upsample_conv2d_bwd(p, p, p, 2, 5, 5, 10, 10, 6, q, q, None, None) < 0
    assert lib.ssdk_depthwise_upsample_conv2d_bwd(p, p, p, 2, 5, 5, 10, 10, 8, None, None, None, None) < 0   # nothing to compute


def test_python_op_refuses_a_map_without_a_window():
    from single_shot_detection_amd import ops
    with pytest.raises(ValueError, match='zero-sized'):
        ops.maxpool2x2(torch.zeros((1, 8, 1, 4)), 0, 1)
