"""CPU: the grid of the BatchNorm statistics launches (csrc/norm.hip bn_reduce_plan, asked through the host-only
ssdk_debug_batchnorm_plan) for every map the three VGG configurations and RetinaNet's tower normalise.

  * the workgroups' (rows x float4 columns), laid out as include/ssdk.h documents them, cover every (row, column) exactly once;
  * the number of workgroups that add to one address of `sums` -- the row blocks -- is not above what the rule before the column slabs gave
    for the same map: max(64, min(4096, rows / 128 rounded up to 16)) rows per workgroup, every workgroup owning every channel."""
import ctypes as C

import numpy as np
import pytest

from single_shot_detection_amd import _lib, synthetic as syn

BATCH = {'ssd_300_vgg16_voc': 32, 'ssd_512_vgg16_coco': 16, 'm2det_512_vgg16_coco': 16, 'retina_rn50_500_coco': 32}


def _maps():
    """(rows, channels) of every normalised map: the SSD tails (1 x 1 to half the channels on the level before, then 3 x 3 / 2 onto the
    level), the maps of the M2Det neck (128 ... 1024 channels, 896 = the seven stacked reducers, on its six scales and the 1 x 1 bottom of a
    TUM), the five levels of the RetinaNet tower."""
    out = set()
    for name in ('ssd_300_vgg16_voc', 'ssd_512_vgg16_coco'):
        levels, B = syn.CONFIGS[name]['levels'], BATCH[name]
        for (_, h_in, _), (cout, h_out, _) in zip(levels[1:], levels[2:]):
            out.add((B * h_in * h_in, cout // 2))
            out.add((B * h_out * h_out, cout))
    B = BATCH['m2det_512_vgg16_coco']
    for h in [l[1] for l in syn.CONFIGS['m2det_512_vgg16_coco']['levels']] + [1]:
        for ch in (128, 256, 512, 896, 1024):
            out.add((B * h * h, ch))
    for ch, h, _ in syn.CONFIGS['retina_rn50_500_coco']['levels']:
        out.add((BATCH['retina_rn50_500_coco'] * h * h, ch))
    return sorted(out)


MAPS = _maps()


def _plan(rows, channels):
    out = (C.c_longlong * 4)()
    assert _lib.lib().ssdk_debug_batchnorm_plan(rows, channels, out) == 0
    return tuple(out)


def _rows_per_block_before(rows):
    r = -(-(-(-rows // 128)) // 16) * 16
    return max(64, min(4096, r))


def test_the_map_list_holds_the_flagship_tail():
    assert {(10368, 256), (2592, 512), (2592, 128), (800, 256), (800, 128), (288, 256), (288, 128), (128, 256)} <= set(MAPS)
    assert (32 * 63 * 63, 256) in MAPS and (16 * 64 * 64, 896) in MAPS


@pytest.mark.parametrize('slab', [None, 0, 16, 32, 64])
def test_grid_covers_every_element_once_and_adds_no_contention(slab, monkeypatch):
    for knob in ('SSDK_BN_ROWS', 'SSDK_BN_WGS', 'SSDK_BN_SLAB'):
        monkeypatch.delenv(knob, raising=False)
    if slab is not None:
        monkeypatch.setenv('SSDK_BN_SLAB', str(slab))
    for rows, channels in MAPS:
        rpb, row_blocks, width, slabs = _plan(rows, channels)
        C4 = channels // 4
        assert width in (1, 2, 4, 8, 16, 32, 64) and slabs >= 1 and row_blocks * slabs < 2 ** 31, (rows, channels)
        row_hits, col_hits = np.zeros(rows, np.int64), np.zeros(C4, np.int64)
        for b in range(row_blocks):
            assert b * rpb < rows, ('an empty row block', rows, channels)
            row_hits[b * rpb:min(rows, (b + 1) * rpb)] += 1
        for s in range(slabs):
            for base in range(s * width, C4, slabs * width):
                col_hits[base:min(C4, base + width)] += 1
        assert (row_hits == 1).all() and (col_hits == 1).all(), (rows, channels)
        assert row_blocks <= -(-rows // _rows_per_block_before(rows)), (rows, channels)
        if slab is None:
            assert width == min(16, 1 << (C4 - 1).bit_length()) and slabs == -(-C4 // width), (rows, channels)


def test_refusals():
    out = (C.c_longlong * 4)()
    lib = _lib.lib()
    assert lib.ssdk_debug_batchnorm_plan(0, 64, out) == -1 and lib.ssdk_debug_batchnorm_plan(64, 6, out) == -1
    assert lib.ssdk_debug_batchnorm_plan(64, 64, None) == -1
