"""GPU: ssdk_augment_boxes / ssdk_augment_images (csrc/augment.hip) called directly -- parameters are chosen, not drawn -- and
DeviceAugmentation end to end.  Every output has guard values on both sides.

Boxes and window choice: bit for bit against the float32 restatement (augment_reference.boxes_reference), equal attempt indices and windows.

Pixel geometry, exact: colour off, mean 0, std 1, no /255, uint8 sources whose mean is an integer, scales 1, 2 and 1/2 -- every weight is
0, .25, .5, .75 or 1, every product and sum is exact in float32 -- bit for bit against the fp64 restatement rounded to float32.

Pixels, general: against the fp64 restatement with the tolerance 8 * max|float32 restatement - fp64 restatement| of the same case (floor: one
float32 ulp at the output's largest magnitude).  Measured on an MI355X (largest over the cases of each test; the output is normalised,
magnitude <= 2.64; on every case the device's deviation from fp64 EQUALS the float32 restatement's, the kernel rounds in the same order):
    test_pixels_general (28 cases, 21 x 13)        device-vs-fp64 3.1e-7 .. 1.9e-6   tolerance 2.5e-6 .. 1.5e-5
    test_pixels_general_500x375_to_300x300         device-vs-fp64 8.8e-7, 4.5e-6     tolerance 7.1e-6, 3.6e-5
    test_device_augmentation_end_to_end (8 images) device-vs-fp64 5.4e-7 .. 3.0e-6   tolerance 4.3e-6 .. 2.4e-5
"""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_cases as cases
import augment_reference as R
from single_shot_detection_amd import _lib
from single_shot_detection_amd.bf.preprocessing import DeviceAugmentation, IMAGE_DTYPE, PARAMS_DTYPE

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD = 64
GUARD = F32(-12345.5)
IGUARD = -77


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(a):
    return _dev(np.ascontiguousarray(a).view(np.uint8).reshape(-1))


def to_records(dicts):
    rec = np.zeros(len(dicts), PARAMS_DTYPE)
    for i, d in enumerate(dicts):
        for k in PARAMS_DTYPE.names:
            rec[k][i] = d[k]
    return rec


def descriptors(sizes):
    desc = np.zeros(len(sizes), IMAGE_DTYPE)
    nbytes = np.array([3 * h * w for h, w in sizes], np.int64)
    desc['offset'] = np.concatenate([[0], np.cumsum(nbytes)[:-1]])
    desc['height'], desc['width'] = [s[0] for s in sizes], [s[1] for s in sizes]
    return desc, int(nbytes.sum())


def _iguarded(n):
    return torch.full((n + 8,), IGUARD, dtype=torch.int32, device='cuda')


def _icheck(t, n, what):
    a = t.cpu().numpy()
    assert np.all(a[:4] == IGUARD) and np.all(a[4 + n:] == IGUARD), f'ssdk_augment_boxes wrote outside {what}'
    return a[4:4 + n]


def run_boxes(targets, sizes, recs, cands, out_size):
    """-> (rows [m, K], offsets, attempts, windows); checks the guards and that no row past offsets[-1] was written"""
    B = len(targets)
    K = targets[0].shape[1]
    counts = [len(t) for t in targets]
    total = sum(counts)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows = np.concatenate(targets, axis=0).astype(F32) if total else np.zeros((0, K), F32)
    cands = np.ascontiguousarray(cands, np.int32)
    T = cands.shape[1]
    desc, _ = descriptors(sizes)
    d_desc, d_rec, d_cand = _bytes(desc), _bytes(to_records(recs)), _dev(cands.reshape(-1))
    d_rows = _dev(rows.reshape(-1)) if total else torch.zeros((4,), dtype=torch.float32, device='cuda')
    d_offs = _dev(offs)
    dst = torch.full((total * K + 2 * PAD,), float(GUARD), dtype=torch.float32, device='cuda')
    d_offs_out, d_att, d_win = _iguarded(B + 1), _iguarded(B), _iguarded(4 * B)
    lib = _lib.lib()
    need = lib.ssdk_augment_boxes_workspace_bytes(B)
    ws = torch.empty((need + 256,), dtype=torch.uint8, device='cuda')
    rc = lib.ssdk_augment_boxes(_lib.ptr(d_desc), _lib.ptr(d_rec), _lib.ptr(d_cand), T, _lib.ptr(d_rows), K, _lib.ptr(d_offs), B, total,
                                out_size[0], out_size[1], C.c_void_p(dst.data_ptr() + 4 * PAD), C.c_void_p(d_offs_out.data_ptr() + 16),
                                C.c_void_p(d_att.data_ptr() + 16), C.c_void_p(d_win.data_ptr() + 16), _lib.ptr(ws), need, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.ssdk_last_error_string())
    o = _icheck(d_offs_out, B + 1, 'offsets_out')
    att = _icheck(d_att, B, 'attempt_out')
    win = _icheck(d_win, 4 * B, 'windows_out').reshape(B, 4)
    full = dst.cpu().numpy()
    used = int(o[-1]) * K
    assert 0 <= used <= total * K
    assert np.all(full[:PAD] == GUARD) and np.all(full[PAD + used:] == GUARD), 'ssdk_augment_boxes wrote outside the rows it reports'
    return full[PAD:PAD + used].reshape(-1, K), o, att, win


def check_boxes(targets, sizes, recs, cands, out_size):
    got = run_boxes(targets, sizes, recs, cands, out_size)
    want = R.batch_boxes_reference(targets, sizes, recs, cands, out_size)
    assert np.array_equal(got[2], want[2]), ('attempts', got[2].tolist(), want[2].tolist())
    assert np.array_equal(got[3], want[3]), 'windows'
    assert np.array_equal(got[1], want[1]), 'offsets'
    assert got[0].shape == want[0].reshape(-1, got[0].shape[1]).shape
    assert np.array_equal(got[0].view(np.uint32), want[0].reshape(got[0].shape).view(np.uint32)), 'rows'
    return got, want


def run_images(imgs, recs, windows, out_size, divide_255=False, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), misalign=0):
    """-> out [B, 3, out_h, out_w]; the output starts `misalign` floats behind a 256-byte boundary"""
    B = len(imgs)
    ow, oh = out_size
    desc, nbytes = descriptors([im.shape[:2] for im in imgs])
    d_src = _dev(np.concatenate([im.reshape(-1) for im in imgs]))
    d_desc, d_rec, d_win = _bytes(desc), _bytes(to_records(recs)), _dev(np.asarray(windows, np.int32).reshape(-1))
    n = B * 3 * oh * ow
    dst = torch.full((n + 2 * PAD + 8,), float(GUARD), dtype=torch.float32, device='cuda')
    lo = PAD + misalign
    lib = _lib.lib()
    need = lib.ssdk_augment_images_workspace_bytes(B)
    ws = torch.empty((need + 256,), dtype=torch.uint8, device='cuda')
    mean_std = np.array(list(mean) + list(std), F32)
    rc = lib.ssdk_augment_images(_lib.ptr(d_src), nbytes, _lib.ptr(d_desc), _lib.ptr(d_rec), _lib.ptr(d_win), B, ow, oh, int(divide_255),
                                 mean_std.ctypes.data_as(C.c_void_p), C.c_void_p(dst.data_ptr() + 4 * lo), _lib.ptr(ws), need, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.ssdk_last_error_string())
    full = dst.cpu().numpy()
    assert np.all(full[:lo] == GUARD) and np.all(full[lo + n:] == GUARD), 'ssdk_augment_images wrote outside its output'
    return full[lo:lo + n].reshape(B, 3, oh, ow)


# ---- boxes and window choice ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out_size', [(16, 16), (21, 13)])
def test_hand_worked_cases_in_one_batch(out_size):
    cs = cases.box_cases()
    names = sorted(cs)
    cands = cases.pad_candidates([cs[n]['candidates'] for n in names], 50)
    got, _ = check_boxes([cs[n]['target'] for n in names], [cs[n]['size'] for n in names], [cs[n]['p'] for n in names], cands, out_size)
    assert got[2].tolist() == [cs[n]['attempt'] for n in names]      # ... and the attempts are the hand-worked ones


def test_hand_worked_boxes_at_their_own_output_size():
    cs = cases.box_cases()
    for name in sorted(cs):
        c = cs[name]
        got, _ = check_boxes([c['target']], [c['size']], [c['p']], cases.pad_candidates([c['candidates']], len(c['candidates'])), c['out_size'])
        assert got[0][:, :4].tolist() == np.asarray(c['boxes'], F32).reshape(-1, 4).tolist(), name
        assert int(got[2][0]) == c['attempt'], name


@pytest.mark.parametrize('width', [6, 7])
def test_counts_0_1_3_70_in_one_batch(width):
    t, s, p, c = cases.random_box_batch(11 + width, 8, 0, width, 12, counts=[0, 1, 3, 70, 70, 3, 0, 65])
    for i in range(8):
        p[i]['flags'] |= R.CROP
    p[3]['flags'] &= ~R.KEEP_IOU
    p[4]['flags'] |= R.KEEP_IOU                                     # both keep criteria on an image wider than a wavefront
    got, want = check_boxes(t, s, p, c, (16, 16))
    if width == 7:                                                  # column 6 survives: the input's bits of the rows that stayed
        ids = got[0][:, 6]
        assert len(ids) and np.all(ids >= 600) and np.array_equal(ids, want[0][:, 6])


def test_acceptance_at_attempt_0_at_49_and_at_none():
    miss = [[30 + (i % 5), 30, 20, 20] for i in range(50)]
    hit = [0, 0, 24, 24]
    cands = np.array([[hit] + miss[1:], miss[:49] + [hit], miss], np.int32)
    t = [cases.rows([[2, 2, 10, 12], [4, 3, 9, 9]])] * 3
    p = [R.params(R.CROP, min_iou=0.5, min_objects_kept=1)] * 3
    got, _ = check_boxes(t, [(64, 64)] * 3, p, cands, (32, 32))
    assert got[2].tolist() == [0, 49, -1]
    assert got[3].tolist() == [[0, 0, 24, 24], [0, 0, 24, 24], [0, 0, 64, 64]]


def test_a_single_attempt():
    t, s, p, c = cases.random_box_batch(23, 40, 9, 6, 1)
    got, _ = check_boxes(t, s, p, c, (20, 12))
    assert set(got[2].tolist()) <= {-2, -1, 0} and 0 in got[2] and -2 in got[2]


def test_300_images_with_ragged_counts():
    t, s, p, c = cases.random_box_batch(31, 300, 70, 7, 6)
    got, _ = check_boxes(t, s, p, c, (21, 13))
    att = got[2]
    assert got[1][-1] > 1000 and (att == -1).any() and (att == -2).any() and (att == 0).any() and (att >= 3).any()
    flags = np.array([q['flags'] for q in p])
    for f in (R.EXPAND, R.HFLIP, R.VFLIP, R.KEEP_IOU):
        assert (flags & f).any() and not (flags & f).all()


def test_boxes_refuses_bad_arguments():
    lib = _lib.lib()
    one = torch.zeros((64,), dtype=torch.int32, device='cuda')
    rc = lib.ssdk_augment_boxes(_lib.ptr(one), _lib.ptr(one), _lib.ptr(one), 1, None, 6, _lib.ptr(one), 1, 0, 16, 16, None, _lib.ptr(one),
                                _lib.ptr(one), _lib.ptr(one), None, 0, _lib.current_stream())
    assert rc == -2 and b'ssdk_augment_boxes' in lib.ssdk_last_error_string()       # SSDK_E_WORKSPACE
    rc = lib.ssdk_augment_boxes(_lib.ptr(one), _lib.ptr(one), _lib.ptr(one), 1, None, 3, _lib.ptr(one), 1, 0, 16, 16, None, _lib.ptr(one),
                                _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), 256, _lib.current_stream())
    assert rc == -1                                                                  # gt_stride 3
    torch.cuda.synchronize()
    assert bool((one == 0).all())


# ---- pixel geometry, exact -------------------------------------------------------------------------------------------------------------
def check_exact(cs, out_size, misalign=0):
    out = run_images([c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs], out_size, misalign=misalign)
    for i, (name, img, p, win) in enumerate(cs):
        want = R.image_reference(img, p, win, out_size, dtype=np.float64)
        w32 = want.astype(F32)
        assert np.array_equal(w32.astype(np.float64), want), name    # the case IS exact in float32
        bad = out[i].view(np.uint32) != w32.view(np.uint32)
        assert not bad.any(), (name, out_size, int(bad.sum()), out[i][bad][:4].tolist(), w32[bad][:4].tolist())


@pytest.mark.parametrize('out_size', cases.GEOMETRY_OUTPUTS)
def test_geometry_exact(out_size):
    cs = cases.geometry_cases(out_size)
    assert len(cs) >= 28
    check_exact(cs, out_size)


def test_geometry_exact_with_an_unaligned_output():
    check_exact(cases.geometry_cases((16, 16), seed=1), (16, 16), misalign=1)     # a row length of 4 n, but no float4 store is possible


def test_crop_2x2_upsampled_to_4x4_does_not_leak():
    img = np.full((4, 6, 3), 255, np.uint8)
    img[1:3, 2:4] = [[[10, 20, 30], [20, 40, 60]], [[30, 60, 90], [40, 80, 120]]]
    out = run_images([img], [R.params(0)], [(2, 1, 2, 2)], (4, 4))[0]
    assert out[0].tolist() == [[10, 12.5, 17.5, 20], [15, 17.5, 22.5, 25], [25, 27.5, 32.5, 35], [30, 32.5, 37.5, 40]]
    assert np.array_equal(out[1], 2 * out[0]) and np.array_equal(out[2], 3 * out[0])
    check_exact([('crop2x2', img, R.params(R.HFLIP | R.VFLIP), (2, 1, 2, 2))], (4, 4))


# ---- pixels, general -------------------------------------------------------------------------------------------------------------------
def check_general(cs, out_size, label):
    out = run_images([c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs], out_size, **cases.NORMALISE)
    worst = (0.0, 0.0, 0.0)
    failed = []
    for i, (name, img, p, win) in enumerate(cs):
        want, tol, diff = cases.tolerance(img, p, win, out_size, **cases.NORMALISE)
        err = float(np.abs(out[i].astype(np.float64) - want).max())
        print(f'{label} {name}: device-vs-fp64 {err:.3e}  float32-vs-fp64 {diff:.3e}  tolerance {tol:.3e}')
        worst = max(worst, (err, diff, tol))
        if not err <= tol:
            failed.append((name, err, tol))
    print(f'{label} WORST: device-vs-fp64 {worst[0]:.3e}  float32-vs-fp64 {worst[1]:.3e}  tolerance {worst[2]:.3e}')
    assert not failed, failed
    return out


def test_pixels_general():
    check_general(cases.general_cases(), (21, 13), 'general')


def test_pixels_general_500x375_to_300x300():
    """An image that spans many workgroups in both statistics passes (128 per image) and in the gather (88)."""
    rng = np.random.default_rng(99)
    base = rng.integers(0, 256, (47, 63, 3), dtype=np.uint8)
    img = np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), np.uint8))[:375, :500])       # blocky, with sharp edges
    img = (img.astype(np.int16) + rng.integers(-9, 10, img.shape)).clip(0, 255).astype(np.uint8)
    every = R.HUE_SATURATION | R.BRIGHTNESS | R.CONTRAST | R.EXPAND
    cs = [('voc_all', img, R.params(every | R.HFLIP, hue_delta=0.05, saturation=1.2, brightness=12.75, contrast=1.3, expand=(900, 700, 130, 80)),
           (-50, -30, 610, 433)),
          ('voc_plain', img, R.params(0), (0, 0, 500, 375))]
    check_general(cs, (300, 300), 'voc')


def test_statistics_are_the_same_bits_run_to_run():
    cs = cases.general_cases()
    args = ([c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs], (20, 12))
    a, b = run_images(*args, **cases.NORMALISE), run_images(*args, **cases.NORMALISE)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_device_augmentation_end_to_end():
    from single_shot_detection_amd.detection.target_assigner import PackedGroundTruth, TargetAssigner
    rng = np.random.default_rng(2024)
    aug = DeviceAugmentation(cases.SSD_AUGMENTATIONS, cases.SSD_PREPROCESSING, (64, 48))
    targets, sizes, _, _ = cases.random_box_batch(5, 8, 6, 6, 1, size_range=(24, 80), counts=[0, 1, 2, 3, 4, 5, 6, 2])
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    params = aug.draw(sizes, rng=np.random.default_rng(77))
    assert len(set(params.records['flags'].tolist())) > 3
    imgs, rows, offs = aug.augment_padded([torch.from_numpy(im) for im in images], [torch.from_numpy(t) for t in targets], params=params)
    again = aug.augment_padded([torch.from_numpy(im).cuda() for im in images], [torch.from_numpy(t).cuda() for t in targets], params=params)
    torch.cuda.synchronize()
    want = R.batch_boxes_reference(targets, sizes, params.records, params.candidates, (64, 48))
    o = offs.cpu().numpy()
    assert np.array_equal(o, want[1]) and np.array_equal(aug.last_attempts.cpu().numpy(), want[2])
    got_rows = rows.cpu().numpy()[:o[-1]]
    assert np.array_equal(got_rows.view(np.uint32), want[0].reshape(got_rows.shape).view(np.uint32))
    windows = aug.last_windows.cpu().numpy()
    assert np.array_equal(windows, want[3])
    out = imgs.cpu().numpy()
    assert out.shape == (8, 3, 48, 64)
    for i in range(8):
        ref, tol, diff = cases.tolerance(images[i], params.records[i], windows[i], (64, 48), **cases.NORMALISE)
        err = float(np.abs(out[i].astype(np.float64) - ref).max())
        print(f'end-to-end image {i}: flags {int(params.records["flags"][i])} device-vs-fp64 {err:.3e}  float32-vs-fp64 {diff:.3e}  tolerance {tol:.3e}')
        assert err <= tol, (i, err, tol)
    # images and targets that are already on the device give the same bits
    assert torch.equal(again[0], imgs) and torch.equal(again[2], offs) and torch.equal(again[1][:o[-1]], rows[:o[-1]])
    # the packed form goes straight into the target assigner
    g = torch.Generator().manual_seed(3)
    anchors = torch.cat([torch.rand((400, 2), generator=g) * torch.tensor([64.0, 48.0]), torch.rand((400, 2), generator=g) * 30 + 4], dim=1).cuda()
    assigner = TargetAssigner(0.5, 0.4)
    packed = assigner.encode_ground_truth(PackedGroundTruth(rows, offs), anchors)
    listed = assigner.encode_ground_truth([rows[o[i]:o[i + 1]] for i in range(8)], anchors)
    assert torch.equal(packed, listed) and bool((packed[..., 4] > 0).any())
    # __call__: the list form, after its one copy of the offsets
    imgs2, views = aug([torch.from_numpy(im) for im in images], [torch.from_numpy(t) for t in targets], rng=np.random.default_rng(77))
    assert torch.equal(imgs2, imgs) and [len(v) for v in views] == np.diff(o).tolist()
    assert all(torch.equal(v, rows[o[i]:o[i + 1]]) for i, v in enumerate(views))
