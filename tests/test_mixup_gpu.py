"""GPU: ssdk_mixup_images / ssdk_mixup_ground_truth (csrc/metrics.hip) called directly -- index, roll and lam are chosen, not drawn --
and compared BIT FOR BIT with numpy float32:  lam_f = float32(lam), oml_f = float32(1 - lam),
out = fl(fl(lam_f * a) + fl(oml_f * b)) for a mixed image, a plain copy for the others; a mixed score is fl(v * lam_f) or fl(v * oml_f).
Shapes: the float4 kernel with several workgroups and a ragged last stride, the scalar kernel over several workgroups (a size that is no
multiple of 4, and a misaligned base pointer), batches of 300 images with up to 70 rows each for the ragged concatenation."""
import ctypes as C

import numpy as np
import pytest
import torch

from single_shot_detection_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD = 64                       # guard floats on either side of every output
GUARD = F32(-12345.5)
E_INVALID = -1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mix_images_reference(imgs, index, roll, lam):
    lam_f, oml_f = F32(lam), F32(1.0 - lam)
    out = imgs.copy()
    for b in range(len(imgs)):
        if roll[b]:
            out[b] = lam_f * imgs[b] + oml_f * imgs[index[b]]      # float32 arrays: the products and the sum round separately
    assert out.dtype == F32
    return out


def mix_images_device(imgs, index, roll, lam, misalign_in=0, misalign_out=0):
    """-> (status, out); in / out start `misalign_*` floats behind a 256-byte aligned allocation; guards around out are checked"""
    B, per = imgs.shape[0], int(np.prod(imgs.shape[1:]))
    src = torch.zeros((B * per + 8,), dtype=torch.float32, device='cuda')
    src[misalign_in:misalign_in + B * per] = _dev(imgs.reshape(-1))
    dst = torch.full((B * per + 2 * PAD + 8,), float(GUARD), dtype=torch.float32, device='cuda')
    lo = PAD + misalign_out
    d_index, d_roll = _dev(np.asarray(index, np.int32)), _dev(np.asarray(roll, np.uint8))   # (named: they must outlive the launch)
    rc = _lib.lib().ssdk_mixup_images(C.c_void_p(src.data_ptr() + 4 * misalign_in), C.c_void_p(dst.data_ptr() + 4 * lo), B, per,
                                      _lib.ptr(d_index), _lib.ptr(d_roll), float(lam), _lib.current_stream())
    torch.cuda.synchronize()
    full = dst.cpu().numpy()
    assert np.all(full[:lo] == GUARD) and np.all(full[lo + B * per:] == GUARD), 'ssdk_mixup_images wrote outside its output'
    return rc, full[lo:lo + B * per].reshape(imgs.shape)


def roll_patterns(rng, B):
    perm = rng.permutation(B)
    yield 'mixed', perm, (np.arange(B) % 2 == 0)
    yield 'none', perm, np.zeros(B, bool)
    yield 'all', perm, np.ones(B, bool)
    yield 'identity', np.arange(B), np.ones(B, bool)               # index[b] == b: lam * a + (1 - lam) * a, two roundings
    yield 'one_source', np.zeros(B, np.int64), np.ones(B, bool)


@pytest.mark.parametrize('shape,B,mis_in,mis_out', [
    ((3, 52, 53), 4, 0, 0),      # 2067 float4: gx = 2 workgroups of 256, five strides of 512, the last one ragged
    ((3, 64, 64), 5, 0, 0),      # 3072 float4: gx = 3, four exact strides
    ((3, 37, 41), 3, 0, 0),      # 4551 floats, not a multiple of 4: the scalar kernel, 18 workgroups
    ((3, 64, 64), 3, 1, 0),      # divisible by 4, but `in` starts one float off a 16-byte boundary: the scalar kernel
    ((3, 64, 64), 3, 0, 3),      # ... and the same for `out`
    ((3, 300, 300), 3, 0, 0),    # the training shape: 67 500 float4, gx = 65, a ragged last stride
    ((1, 5, 5), 1, 0, 0),        # batch 1
    ((3, 52, 53), 1, 0, 0),
])
def test_mixup_images_bit_exact(shape, B, mis_in, mis_out):
    rng = np.random.default_rng(B * 1000 + shape[1])
    imgs = rng.standard_normal((B,) + shape).astype(F32)
    for lam in (0.37251234567, 0.5, 1.0 / 3.0):
        for tag, index, roll in roll_patterns(rng, B):
            rc, out = mix_images_device(imgs, index, roll, lam, mis_in, mis_out)
            assert rc == 0, (tag, rc)
            want = mix_images_reference(imgs, index, roll, lam)
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (shape, tag, lam, int(np.count_nonzero(out.view(np.uint32) != want.view(np.uint32))))


def test_mixup_images_in_place_is_refused():
    lib = _lib.lib()
    buf = torch.full((3 * 48,), 2.5, dtype=torch.float32, device='cuda')
    idx, roll = _dev(np.array([1, 2, 0], np.int32)), _dev(np.ones(3, np.uint8))
    rc = lib.ssdk_mixup_images(_lib.ptr(buf), _lib.ptr(buf), 3, 48, _lib.ptr(idx), _lib.ptr(roll), 0.3, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == E_INVALID and b'ssdk_mixup_images' in lib.ssdk_last_error_string()
    assert bool((buf == 2.5).all())


# ---- ground truth --------------------------------------------------------------------------------------------------------------------
def mix_gt_reference(rows, offs, stride, index, roll, lam):
    lam_f, oml_f = F32(lam), F32(1.0 - lam)
    out, out_offs = [], [0]
    for b in range(len(offs) - 1):
        own = rows[offs[b]:offs[b + 1]].copy()
        parts = [own]
        if roll[b]:
            other = rows[offs[index[b]]:offs[index[b] + 1]].copy()
            own[:, 5] = own[:, 5] * lam_f
            other[:, 5] = other[:, 5] * oml_f
            parts.append(other)
        out += parts
        out_offs.append(out_offs[-1] + sum(len(p) for p in parts))
    return (np.concatenate(out, 0) if out_offs[-1] else np.zeros((0, stride), F32)), np.array(out_offs, np.int32)


def mix_gt_device(rows, offs, stride, index, roll, lam):
    B, total = len(offs) - 1, len(rows)
    cap = 2 * total * stride
    dst = torch.full((cap + 2 * PAD,), float(GUARD), dtype=torch.float32, device='cuda')
    d_offs_out = torch.full((B + 1 + 2,), -5, dtype=torch.int32, device='cuda')
    d_rows = _dev(rows.reshape(-1)) if total else torch.zeros((4,), dtype=torch.float32, device='cuda')
    d_offs, d_index, d_roll = _dev(offs), _dev(np.asarray(index, np.int32)), _dev(np.asarray(roll, np.uint8))   # (named: they must outlive the launch)
    rc = _lib.lib().ssdk_mixup_ground_truth(_lib.ptr(d_rows), stride, _lib.ptr(d_offs), B, _lib.ptr(d_index), _lib.ptr(d_roll), float(lam),
                                            C.c_void_p(dst.data_ptr() + 4 * PAD), C.c_void_p(d_offs_out.data_ptr() + 4), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    o = d_offs_out.cpu().numpy()
    assert o[0] == -5 and o[-1] == -5, 'ssdk_mixup_ground_truth wrote outside offsets_out'
    o = o[1:-1]
    full = dst.cpu().numpy()
    used = int(o[-1]) * stride
    assert 0 <= used <= cap
    assert np.all(full[:PAD] == GUARD) and np.all(full[PAD + used:] == GUARD), 'ssdk_mixup_ground_truth wrote outside the rows it reports'
    return full[PAD:PAD + used].reshape(-1, stride), o


def make_gt(rng, B, stride, max_rows):
    counts = rng.integers(0, max_rows + 1, B)
    counts[rng.random(B) < 0.15] = 0                               # empty images, on either side of a mix
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows = rng.uniform(0, 300, (int(offs[-1]), stride)).astype(F32)
    rows[:, 4] = rng.integers(0, 21, len(rows))
    rows[:, 5] = rng.uniform(0.01, 1.0, len(rows)).astype(F32)     # already-mixed weights, not just 1.0: the product rounds
    return rows, offs, counts


@pytest.mark.parametrize('stride', [6, 9])
def test_mixup_ground_truth_bit_exact(stride):
    rng = np.random.default_rng(500 + stride)
    B = 300
    rows, offs, counts = make_gt(rng, B, stride, 70)
    assert counts.max() * 2 * stride > 3 * 256 and len(rows) > 8000           # several strides of the 256 threads per image
    index = rng.permutation(B)
    roll = rng.random(B) < 0.6
    own_empty, other_empty = counts == 0, counts[index] == 0
    for a in (False, True):                                        # every combination of an empty image on either side of a mix occurs
        for b in (False, True):
            assert np.any(roll & (own_empty == a) & (other_empty == b)), (a, b)
    for lam in (0.37251234567, 0.9):
        for idx, rl in ((index, roll), (index, np.ones(B, bool)), (index, np.zeros(B, bool)), (np.arange(B), np.ones(B, bool))):
            got, got_offs = mix_gt_device(rows, offs, stride, idx, rl, lam)
            want, want_offs = mix_gt_reference(rows, offs, stride, idx, rl, lam)
            assert np.array_equal(got_offs, want_offs)
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            keep = [c for c in range(stride) if c != 5]
            src = np.concatenate([np.concatenate([np.arange(offs[b], offs[b + 1])] + ([np.arange(offs[idx[b]], offs[idx[b] + 1])] if rl[b] else []))
                                  for b in range(B)]).astype(np.int64)
            assert np.array_equal(got[:, keep].view(np.uint32), rows[src][:, keep].view(np.uint32))   # every other column: the input's bits


def test_mixup_ground_truth_without_any_row():
    for B in (1, 7, 300):
        offs = np.zeros(B + 1, np.int32)
        rng = np.random.default_rng(B)
        got, got_offs = mix_gt_device(np.zeros((0, 6), F32), offs, 6, rng.permutation(B), np.ones(B, bool), 0.25)
        assert got.shape == (0, 6) and np.array_equal(got_offs, offs)


def test_mixup_ground_truth_small_batches():
    rng = np.random.default_rng(77)
    for B in (1, 2, 5):
        rows, offs, _ = make_gt(rng, B, 7, 4)
        index, roll = rng.permutation(B), np.ones(B, bool)
        got, got_offs = mix_gt_device(rows, offs, 7, index, roll, 0.61)
        want, want_offs = mix_gt_reference(rows, offs, 7, index, roll, 0.61)
        assert np.array_equal(got_offs, want_offs) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
