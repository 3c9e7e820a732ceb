"""CPU: the numpy restatement of the augmentation against hand-worked values (cv2 is not available to pin it), the plan parser of
DeviceAugmentation, and its draws.  Nothing here touches the GPU."""
import numpy as np
import pytest

import augment_cases as cases
import augment_reference as R
from single_shot_detection_amd.bf.preprocessing import DeviceAugmentation, PARAMS_DTYPE, IMAGE_DTYPE
from single_shot_detection_amd.bf import preprocessing as P

F32 = np.float32


def resize_row(values, n_out, dtype=np.float64):
    img = np.zeros((1, len(values), 3), np.uint8)
    img[0, :, :] = np.asarray(values, np.uint8)[:, None]
    return R.image_reference(img, R.params(0), (0, 0, len(values), 1), (n_out, 1), dtype=dtype)


# ---- the restatement against hand-worked values --------------------------------------------------------------------------------------
def test_flags_and_records_match_the_header():
    import os
    import re
    from conftest import REPO
    text = open(os.path.join(REPO, 'include', 'ssdk.h')).read()
    for name in ('HUE_SATURATION', 'BRIGHTNESS', 'CONTRAST', 'EXPAND', 'CROP', 'HFLIP', 'VFLIP', 'KEEP_IOU'):
        value = int(re.search(r'#define\s+SSDK_AUG_%s\s+(\d+)' % name, text).group(1))
        assert getattr(R, name) == value == getattr(P, name), name
    assert PARAMS_DTYPE.itemsize == 48 and IMAGE_DTYPE.itemsize == 16
    struct = re.search(r'typedef struct ssdk_augment_params \{(.*?)\}', text, flags=re.S).group(1)
    struct = re.sub(r'/\*.*?\*/', '', struct, flags=re.S)
    fields = [f.strip() for decl in struct.split(';') for f in re.sub(r'^\s*(int|float)\s', '', decl.strip()).split(',') if f.strip()]
    assert fields == list(PARAMS_DTYPE.names)


def test_resize_2_to_4():
    a, b = 40, 200
    out = resize_row([a, b], 4)
    assert out.shape == (3, 1, 4)
    for c in range(3):
        assert out[c, 0].tolist() == [a, .75 * a + .25 * b, .25 * a + .75 * b, b]


def test_resize_4_to_2_gives_the_pair_means():
    out = resize_row([10, 20, 60, 200], 2)
    assert out[0, 0].tolist() == [15.0, 130.0]


def test_resize_identity():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    out = R.image_reference(img, R.params(0), (0, 0, 7, 5), (7, 5))
    assert np.array_equal(out, img.transpose(2, 0, 1).astype(np.float64))
    low = R.image_reference(img, R.params(0), (0, 0, 7, 5), (7, 5), dtype=np.float32)
    assert low.dtype == F32 and np.array_equal(low, out.astype(F32))


def test_flip_of_a_1x3_image():
    img = np.array([[[1, 2, 3], [4, 5, 6], [7, 8, 9]]], np.uint8)
    out = R.image_reference(img, R.params(R.HFLIP), (0, 0, 3, 1), (3, 1))
    assert out[:, 0, :].tolist() == [[7, 4, 1], [8, 5, 2], [9, 6, 3]]
    col = img.transpose(1, 0, 2)                                   # 3 x 1
    out = R.image_reference(col, R.params(R.VFLIP), (0, 0, 1, 3), (1, 3))
    assert out[:, :, 0].tolist() == [[7, 4, 1], [8, 5, 2], [9, 6, 3]]


def test_expand_fills_with_the_mean_and_shifts_the_boxes():
    img = np.array([[[10, 20, 30], [50, 60, 70]]], np.uint8)       # 1 x 2, mean over all six values = 40
    p = R.params(R.EXPAND, expand=(4, 3, 1, 1))
    out = R.image_reference(img, p, (-1, -1, 4, 3), (4, 3))
    want = np.full((3, 3, 4), 40.0)
    want[:, 1, 1], want[:, 1, 2] = [10, 20, 30], [50, 60, 70]
    assert np.array_equal(out, want)
    rows, attempt, win = R.boxes_reference(cases.rows([[0, 0, 1, 0.5]]), (1, 2), p, [[0, 0, 0, 0]], (4, 3))
    assert attempt == -2 and win == (-1, -1, 4, 3)
    assert rows[:, :4].tolist() == [[1, 1, 2, 1.5]]


def test_window_taps_do_not_leak_past_the_window():
    img = np.zeros((4, 4, 3), np.uint8)
    img[1:3, 1:3] = [[[10, 10, 10], [20, 20, 20]], [[30, 30, 30], [40, 40, 40]]]
    img[0], img[3], img[:, 0], img[:, 3] = 255, 255, 255, 255      # whatever surrounds the 2 x 2 window must not show
    out = R.image_reference(img, R.params(0), (1, 1, 2, 2), (4, 4))[0]
    assert out[0].tolist() == [10, 12.5, 17.5, 20] and out[3].tolist() == [30, 32.5, 37.5, 40]
    assert out[:, 0].tolist() == [10, 15, 25, 30]


@pytest.mark.parametrize('name', sorted(cases.box_cases()))
def test_box_cases_by_hand(name):
    c = cases.box_cases()[name]
    rows, attempt, win = R.boxes_reference(c['target'], c['size'], c['p'], c['candidates'], c['out_size'])
    assert attempt == c['attempt'], name
    assert rows.dtype == F32 and rows[:, :4].tolist() == np.asarray(c['boxes'], F32).reshape(-1, 4).tolist(), name
    assert rows[:, 4].tolist() == [float(v) for v in c['classes']], name
    if attempt >= 0:
        assert win[2:] == tuple(c['candidates'][attempt][2:])


def test_fifty_rejected_windows_leave_the_window_whole():
    c = cases.box_cases()['fifty_rejected']
    assert len(c['candidates']) == 50
    _, attempt, win = R.boxes_reference(c['target'], c['size'], c['p'], c['candidates'], c['out_size'])
    assert attempt == -1 and win == (0, 0, 64, 64)


def test_extra_columns_travel():
    t = cases.rows([[1, 1, 5, 5], [2, 2, 2, 7], [3, 3, 8, 8]], width=7)
    rows, _, _ = R.boxes_reference(t, (16, 16), R.params(R.HFLIP), [[0, 0, 0, 0]], (16, 16))
    assert rows[:, 6].tolist() == [600.0, 602.0] and rows[:, 4].tolist() == [1.0, 3.0]


# ---- the plan parser ------------------------------------------------------------------------------------------------------------------
def test_the_ssd_pipeline_parses():
    aug = DeviceAugmentation(cases.SSD_AUGMENTATIONS, cases.SSD_PREPROCESSING, (300, 300))
    assert (aug.out_w, aug.out_h, aug.attempts) == (300, 300, 50)
    assert len(aug.members) == 7 and [m['crop'] for m in aug.members] == [False] + [True] * 6
    assert [m['min_iou'] for m in aug.members[1:]] == [.0, .1, .3, .5, .7, .9]
    assert aug.divide_255 and aug.mean_std.tolist() == [F32(v) for v in (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)]
    assert aug.hflip == .5 and aug.vflip is None
    ev = DeviceAugmentation([], cases.SSD_PREPROCESSING, (512, 300))
    assert (ev.out_w, ev.out_h) == (512, 300) and not ev.members and ev.expand is None


@pytest.mark.parametrize('name,augmentations,input_size', [
    ('RandomRotate', [{'name': 'RandomRotate'}], (300, 300)),
    ('RandomExpand', [{'name': 'RandomCrop'}, {'name': 'RandomExpand'}], (300, 300)),          # a crop placed before the expand
    ('RandomHorizontalFlip', [{'name': 'OneOf', 'args': {'transforms': [{'name': 'Identity'}, {'name': 'RandomHorizontalFlip'}]}}], (300, 300)),
    ('Resize', cases.SSD_AUGMENTATIONS, None),
    ('RandomAdjustBrightness', [{'name': 'RandomAdjustBrightness', 'args': {'max_brightness_delta': .1}}], (300, 300)),   # no ToFloat before it
    ('ToFloat', [{'name': 'RandomAdjustContrast', 'args': {'contrast_delta_range': (.5, 1.5)}}, {'name': 'ToFloat'}], (300, 300)),
])
def test_unsupported_plans_name_the_transform(name, augmentations, input_size):
    with pytest.raises(ValueError, match=name):
        DeviceAugmentation(augmentations, cases.SSD_PREPROCESSING, input_size)


def test_unsupported_preprocessing():
    with pytest.raises(ValueError, match='ToUint8'):
        DeviceAugmentation([], [{'name': 'ToUint8'}], (300, 300))
    with pytest.raises(ValueError, match='Normalize'):
        DeviceAugmentation([], [{'name': 'Normalize'}, {'name': 'ToFloatTensor'}], (300, 300))


# ---- the draws ------------------------------------------------------------------------------------------------------------------------
def _sizes(rng, n):
    return [(int(h), int(w)) for h, w in zip(rng.integers(200, 500, n), rng.integers(200, 500, n))]


def test_same_seed_same_records():
    aug = DeviceAugmentation(cases.SSD_AUGMENTATIONS, cases.SSD_PREPROCESSING, (300, 300))
    sizes = _sizes(np.random.default_rng(1), 64)
    a, b = aug.draw(sizes, rng=np.random.default_rng(5)), aug.draw(sizes, rng=np.random.default_rng(5))
    assert a.records.tobytes() == b.records.tobytes() and np.array_equal(a.candidates, b.candidates)
    c = aug.draw(sizes, rng=np.random.default_rng(6))
    assert a.records.tobytes() != c.records.tobytes()
    assert a.records.dtype == PARAMS_DTYPE and a.candidates.dtype == np.int32 and a.candidates.shape == (64, 50, 4)


def test_draws_respect_ranges_and_probabilities():
    aug = DeviceAugmentation(cases.SSD_AUGMENTATIONS, cases.SSD_PREPROCESSING, (300, 300))
    N = 4000
    sizes = _sizes(np.random.default_rng(2), N)
    d = aug.draw(sizes, rng=np.random.default_rng(3))
    rec, cand = d.records, d.candidates
    h, w = np.array(sizes)[:, 0], np.array(sizes)[:, 1]
    flags = rec['flags']
    ex = (flags & R.EXPAND) != 0
    assert 0.4 < ex.mean() < 0.6                                   # p = .5; a draw whose canvas falls short is retried up to 50 times
    assert np.all(rec['expand_w'][ex] >= w[ex]) and np.all(rec['expand_h'][ex] >= h[ex])
    area = rec['expand_w'][ex].astype(np.int64) * rec['expand_h'][ex]
    assert np.all(area <= 16.0 * (h * w)[ex]) and np.all(area >= 1.0 * (h * w)[ex])
    assert np.all(rec['expand_x'][ex] >= 0) and np.all(rec['expand_x'][ex] + w[ex] <= rec['expand_w'][ex])
    assert np.all(rec['expand_y'][ex] >= 0) and np.all(rec['expand_y'][ex] + h[ex] <= rec['expand_h'][ex])
    assert np.all(rec['expand_w'][~ex] == 0)
    cw, ch = np.where(ex, rec['expand_w'], w), np.where(ex, rec['expand_h'], h)
    crop = (flags & R.CROP) != 0
    valid = cand[:, :, 2] > 0
    assert not valid[~crop].any() and valid[crop].any(axis=1).all()
    x, y, nw, nh = (cand[:, :, k] for k in range(4))
    assert np.all((x >= 0) & (y >= 0))
    assert np.all((x + nw <= cw[:, None])[valid]) and np.all((y + nh <= ch[:, None])[valid]) and np.all(nh[valid] > 0)
    got = (nw.astype(np.int64) * nh)[valid] / np.broadcast_to((cw * ch)[:, None], nw.shape)[valid]
    assert got.max() <= 1.0 and got.min() > 0.05                   # area_range (0.1, 1), less what int() cuts off
    # each OneOf member appears: six crop thresholds (each with its own p = .5) and the identity
    seen = sorted(set(np.round(rec['min_iou'][crop].astype(np.float64), 3).tolist()))
    assert seen == [.0, .1, .3, .5, .7, .9]
    share = np.array([np.mean(crop & np.isclose(rec['min_iou'], v)) for v in seen])
    assert np.all(np.abs(share - 0.5 / 7) < 0.02)
    assert np.all(rec['min_objects_kept'][crop] == 1) and not np.any(flags & R.KEEP_IOU)
    assert 0.45 < ((flags & R.HFLIP) != 0).mean() < 0.55 and not np.any(flags & R.VFLIP)
    hs = (flags & R.HUE_SATURATION) != 0
    assert 0.70 < hs.mean() < 0.80                                 # hue or saturation, each with p = .5
    assert np.all(np.abs(rec['hue_delta']) <= 0.1) and np.all((rec['saturation'] >= 0.5) & (rec['saturation'] <= 1.5))
    br = (flags & R.BRIGHTNESS) != 0
    assert np.all(np.abs(rec['brightness']) <= 0.15 * 255 + 1e-3) and np.all(rec['brightness'][~br] == 0) and np.abs(rec['brightness'][br]).max() > 30
    assert np.all((rec['contrast'] >= 0.5) & (rec['contrast'] <= 1.5)) and np.all(rec['contrast'][(flags & R.CONTRAST) == 0] == 1)


def test_evaluation_pipeline_draws_nothing():
    aug = DeviceAugmentation([], cases.SSD_PREPROCESSING, (300, 300), attempts=1)
    d = aug.draw([(100, 200), (50, 60)], rng=np.random.default_rng(0))
    assert np.all(d.records['flags'] == 0) and not d.candidates.any() and d.candidates.shape == (2, 1, 4)


def test_keep_criterion_and_single_crop():
    aug = DeviceAugmentation([{'name': 'RandomCrop', 'args': {'min_iou': .3, 'keep_criterion': 'iou', 'min_objects_kept': 2, 'p': 1.0}},
                              {'name': 'RandomVerticalFlip', 'args': {'p': 1.0}}], [{'name': 'ToFloatTensor'}], (64, 32), attempts=5)
    d = aug.draw([(40, 50)] * 10, rng=np.random.default_rng(0))
    assert np.all(d.records['flags'] == R.CROP | R.KEEP_IOU | R.VFLIP) and np.all(d.records['min_objects_kept'] == 2)
    assert np.allclose(d.records['min_iou'], 0.3) and not aug.divide_255
    with pytest.raises(ValueError, match='keep_criterion'):
        DeviceAugmentation([{'name': 'RandomCrop', 'args': {'keep_criterion': 'area'}}], [{'name': 'ToFloatTensor'}], (64, 32))
