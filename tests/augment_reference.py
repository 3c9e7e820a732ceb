"""A numpy restatement of the SSD augmentation (include/ssdk.h, "device-side SSD augmentation"), written from its description.

Three parts:
  * ``boxes_reference``: window choice and boxes in float32, one rounding per operation, in the order of functional/box.py;
  * ``image_reference(..., dtype=np.float64)``: the pixels in fp64;
  * ``image_reference(..., dtype=np.float32)``: the same formulas evaluated in float32 -- used ONLY to size the tolerance of the general
    pixel test (it samples the rounding error of these formulas in one operation order).

A parameter record ``p`` is anything indexable by field name (a dict, or one element of the PARAMS_DTYPE array): flags, hue_delta,
saturation, brightness, contrast, expand_w, expand_h, expand_x, expand_y, min_iou, min_objects_kept.  Every float parameter is taken
as its float32 value.
"""
import numpy as np

F32 = np.float32
HUE_SATURATION, BRIGHTNESS, CONTRAST, EXPAND, CROP, HFLIP, VFLIP, KEEP_IOU = 1, 2, 4, 8, 16, 32, 64, 128


def params(flags=0, hue_delta=0.0, saturation=1.0, brightness=0.0, contrast=1.0, expand=(0, 0, 0, 0), min_iou=0.0, min_objects_kept=0):
    """expand = (canvas_w, canvas_h, xmin, ymin)"""
    return {'flags': int(flags), 'hue_delta': hue_delta, 'saturation': saturation, 'brightness': brightness, 'contrast': contrast,
            'expand_w': int(expand[0]), 'expand_h': int(expand[1]), 'expand_x': int(expand[2]), 'expand_y': int(expand[3]),
            'min_iou': min_iou, 'min_objects_kept': int(min_objects_kept), 'reserved': 0}


# ---- boxes --------------------------------------------------------------------------------------------------------------------------
def _area(b):
    return np.maximum(b[:, 2] - b[:, 0], F32(0)) * np.maximum(b[:, 3] - b[:, 1], F32(0))      # NaN propagates, as Tensor.clamp_(0)


def _iou_elementwise(a, b):
    mn, mx = np.maximum(a[:, :2], b[:, :2]), np.minimum(a[:, 2:4], b[:, 2:4])
    inter = _area(np.concatenate([mn, mx], axis=1))
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / (_area(a) + _area(b) - inter)


def crop_region(xmin, ymin, w, h):
    return np.array([xmin, ymin, xmin + w - 1, ymin + h - 1], F32)


def crop_boxes(target, xmin, ymin, w, h, min_iou, keep_iou, min_kept):
    """functional/box.py crop: None when the window is rejected, else the kept rows, shifted and clipped."""
    if len(target) == 0:
        return target
    region, min_iou = crop_region(xmin, ymin, w, h), F32(min_iou)
    t = target[:, :4]
    mn, mx = np.maximum(region[None, :2], t[:, :2]), np.minimum(region[None, 2:], t[:, 2:4])
    new = np.concatenate([mn, mx], axis=1).astype(F32)
    new[(mx < mn).any(axis=1)] = 0                                     # zero_incorrect
    iou = _iou_elementwise(t, new)
    assert iou.dtype == F32
    top = iou.max()                                                    # NaN as soon as one IoU is NaN
    if not top > min_iou:
        return None
    if keep_iou:
        keep = iou > min_iou
    else:
        centre = (t[:, :2] + t[:, 2:4]) / F32(2)
        keep = ((centre > region[:2]) & (centre < region[2:])).all(axis=1)
    if int(keep.sum()) < min_kept:
        return None
    out = target[keep].copy()
    nb = new[keep]
    nb[:, [0, 2]] -= F32(xmin)
    nb[:, [1, 3]] -= F32(ymin)
    nb[:, [0, 2]] = np.clip(nb[:, [0, 2]], F32(0), F32(w - 1))
    nb[:, [1, 3]] = np.clip(nb[:, [1, 3]], F32(0), F32(h - 1))
    out[:, :4] = nb
    return out


def boxes_reference(target, size, p, candidates, out_size):
    """target [n, K] float32, size (H, W), candidates int [attempts, 4] -> (rows [m, K], attempt, window (x, y, w, h) in source coordinates)"""
    target = np.array(target, F32, ndmin=2)
    target = target.copy() if target.size else np.zeros((0, max(target.shape[-1], 4)), F32)
    H, W = size
    out_w, out_h = out_size
    flags = int(p['flags'])
    cw, ch, ex, ey = W, H, 0, 0
    if flags & EXPAND:
        cw, ch, ex, ey = int(p['expand_w']), int(p['expand_h']), int(p['expand_x']), int(p['expand_y'])
        target[:, [0, 2]] += F32(ex)
        target[:, [1, 3]] += F32(ey)
    attempt, win = -2, (0, 0, cw, ch)
    if flags & CROP:
        attempt = -1
        for a, (x, y, w, h) in enumerate(np.asarray(candidates).reshape(-1, 4).tolist()):
            if w <= 0 or h <= 0 or x < 0 or y < 0 or x + w > cw or y + h > ch:
                continue
            new = crop_boxes(target, x, y, w, h, p['min_iou'], bool(flags & KEEP_IOU), int(p['min_objects_kept']))
            if new is not None:
                target, attempt, win = new, a, (x, y, w, h)
                break
    ww, wh = win[2], win[3]
    if flags & HFLIP:
        target[:, [0, 2]] = F32(ww - 1) - target[:, [2, 0]]
    if flags & VFLIP:
        target[:, [1, 3]] = F32(wh - 1) - target[:, [3, 1]]
    target[:, [0, 2]] *= F32(out_w / ww)
    target[:, [1, 3]] *= F32(out_h / wh)
    target[:, [0, 2]] = np.clip(target[:, [0, 2]], F32(0), F32(out_w - 1))
    target[:, [1, 3]] = np.clip(target[:, [1, 3]], F32(0), F32(out_h - 1))
    keep = ~((target[:, 0] == target[:, 2]) | (target[:, 1] == target[:, 3]))
    assert target.dtype == F32
    return target[keep], attempt, (win[0] - ex, win[1] - ey, ww, wh)


def batch_boxes_reference(targets, sizes, records, candidates, out_size):
    """-> (rows [sum m, K], offsets int32 [B + 1], attempts int32 [B], windows int32 [B, 4])"""
    rows, offs, att, wins = [], [0], [], []
    for t, s, p, c in zip(targets, sizes, records, candidates):
        r, a, w = boxes_reference(t, s, p, c, out_size)
        rows.append(r)
        offs.append(offs[-1] + len(r))
        att.append(a)
        wins.append(w)
    K = max([r.shape[1] for r in rows if r.ndim == 2] + [0])
    rows = np.concatenate([r.reshape(-1, K) for r in rows], axis=0) if rows else np.zeros((0, K), F32)
    return rows.astype(F32), np.array(offs, np.int32), np.array(att, np.int32), np.array(wins, np.int32).reshape(-1, 4)


# ---- pixels -------------------------------------------------------------------------------------------------------------------------
def _hsv_channel(n, h, v, vs, dt):
    k = dt(n) + h
    k = k - dt(6) * np.floor(k / dt(6))
    m = np.maximum(dt(0), np.minimum(np.minimum(k, dt(4) - k), dt(1)))
    return v - vs * m


def colour_pre(img, p, dt):
    """steps 1-3 on a uint8 [H, W, 3] image -> dt [H, W, 3]"""
    flags = int(p['flags'])
    x = img.astype(dt)
    if flags & HUE_SATURATION:
        r, g, b = x[..., 0], x[..., 1], x[..., 2]
        mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
        c = mx - mn
        cs = np.where(c > 0, c, dt(1))
        h = np.where(mx == r, (g - b) / cs, np.where(mx == g, dt(2) + (b - r) / cs, dt(4) + (r - g) / cs))
        h = np.where(c > 0, h, dt(0)).astype(dt)
        s = np.where(mx > 0, c / np.where(mx > 0, mx, dt(1)), dt(0)).astype(dt)
        h = h + dt(F32(p['hue_delta'])) * dt(6)
        s = np.clip(s * dt(F32(p['saturation'])), dt(0), dt(1))
        vs = mx * s
        x = np.stack([_hsv_channel(5, h, mx, vs, dt), _hsv_channel(3, h, mx, vs, dt), _hsv_channel(1, h, mx, vs, dt)], axis=-1)
    if flags & BRIGHTNESS:
        x = np.clip(x + dt(F32(p['brightness'])), dt(0), dt(255))
    assert x.dtype == dt
    return x


def colour(img, p, dt):
    """steps 1-4 -> (dt [H, W, 3], fill).  The means are fp64 sums, the quotient rounded to float32 once when dt is float32."""
    flags = int(p['flags'])
    x = colour_pre(img, p, dt)
    npx = img.shape[0] * img.shape[1]
    if flags & CONTRAST:
        mean = (x.reshape(-1, 3).astype(np.float64).sum(axis=0) / npx).astype(dt)
        x = np.clip(mean + dt(F32(p['contrast'])) * (x - mean), dt(0), dt(255))
    fill = dt(x.astype(np.float64).sum() / (3 * npx)) if flags & EXPAND else dt(0)
    assert x.dtype == dt
    return x, fill


def taps(n_out, win, origin, flip, dt):
    """Resize's two taps per output index, in source coordinates, and the weight of the second."""
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * (win / n_out) - 0.5
    f = np.floor(s)
    wgt = (s - f).astype(dt)
    a = np.clip(f.astype(np.int64), 0, win - 1)
    b = np.clip(f.astype(np.int64) + 1, 0, win - 1)
    if flip:
        a, b = win - 1 - a, win - 1 - b
    return a + origin, b + origin, wgt


def image_reference(img, p, window, out_size, divide_255=False, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype=np.float64):
    """img uint8 [H, W, 3]; window (x, y, w, h) in source coordinates -> dtype [3, out_h, out_w]"""
    dt = dtype
    flags = int(p['flags'])
    H, W = img.shape[:2]
    out_w, out_h = out_size
    x, fill = colour(img, p, dt)
    wx0, wy0, ww, wh = (int(v) for v in window)
    xa, xb, wgx = taps(out_w, ww, wx0, bool(flags & HFLIP), dt)
    ya, yb, wgy = taps(out_h, wh, wy0, bool(flags & VFLIP), dt)

    def read(ys, xs):
        inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
        v = x[np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]]
        return np.where(inside[:, :, None], v, fill).astype(dt)

    wx, wy = wgx[None, :, None], wgy[:, None, None]
    top = (dt(1) - wx) * read(ya, xa) + wx * read(ya, xb)
    bot = (dt(1) - wx) * read(yb, xa) + wx * read(yb, xb)
    v = (dt(1) - wy) * top + wy * bot
    if divide_255:
        v = v / dt(255)
    v = (v - np.array(mean, F32).astype(dt)) / np.array(std, F32).astype(dt)
    assert v.dtype == dt
    return np.ascontiguousarray(v.transpose(2, 0, 1))
