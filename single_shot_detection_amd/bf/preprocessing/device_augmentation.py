"""DeviceAugmentation -- bf/preprocessing/transforms.py of the reference as two libssdk calls per batch (csrc/augment.hip).

The reference augments one image at a time with cv2 / numpy in DataLoader workers.  Here the host only DRAWS: a few vectorised numpy
calls fill one parameter record per image; the raw ``uint8`` images travel to the device in one ragged buffer, and everything else --
the choice of the crop window, the boxes, the colour steps, expand, crop, flips, resize, ``/255`` and normalisation -- happens there.
Expand, crop, flip and resize each map one axis-aligned window onto another, so they compose into a single window in source
coordinates: the whole pipeline is one gather per output pixel, and the expanded canvas (up to 16 times the image) never exists.

One fixed order is supported, the order of every sample configuration of the reference; every step is optional::

    RandomAdjustHueSaturation, ToFloat, RandomAdjustBrightness, RandomAdjustContrast, RandomExpand,
    OneOf[Identity | RandomCrop...] or RandomCrop, RandomHorizontalFlip / RandomVerticalFlip          (augmentations)
    Resize(input_size), ToFloatTensor(normalize), Normalize(mean, std)                                 (preprocessing)

Anything else (``RandomRotate``, another order, ``OneOf`` over other members, no ``input_size``) raises ``ValueError`` naming the
transform.  The semantics are the reference's (the exact rules: ``ssdk_augment_boxes`` / ``ssdk_augment_images`` in include/ssdk.h), with
two deliberate deviations:

* Hue and saturation are adjusted in float HSV on the pixel value: hue is shifted by ``delta * 360`` degrees modulo 360, saturation is
  multiplied and clipped to [0, 1], and the result is not rounded back to 8 bits.  The reference round-trips through cv2's 8-bit HSV
  (hue in 2-degree steps); that quantisation is not reproduced.
* The random draws are made up front and vectorised from a ``numpy.random.Generator``, so the stream of random numbers differs from the
  reference's lazy ``random.*`` calls.  The distributions are the same: the same ranges, probabilities and rejection rules.
"""
import ctypes as C

import numpy as np

# SSDK_AUG_* (include/ssdk.h)
HUE_SATURATION, BRIGHTNESS, CONTRAST, EXPAND, CROP, HFLIP, VFLIP, KEEP_IOU = 1, 2, 4, 8, 16, 32, 64, 128

# ssdk_augment_image / ssdk_augment_params (include/ssdk.h)
IMAGE_DTYPE = np.dtype([('offset', '<i8'), ('height', '<i4'), ('width', '<i4')])
PARAMS_DTYPE = np.dtype([('flags', '<i4'), ('hue_delta', '<f4'), ('saturation', '<f4'), ('brightness', '<f4'), ('contrast', '<f4'),
                         ('expand_w', '<i4'), ('expand_h', '<i4'), ('expand_x', '<i4'), ('expand_y', '<i4'), ('min_iou', '<f4'),
                         ('min_objects_kept', '<i4'), ('reserved', '<i4')])
assert IMAGE_DTYPE.itemsize == 16 and PARAMS_DTYPE.itemsize == 48

_RANK = {'RandomAdjustHueSaturation': 0, 'ToFloat': 1, 'RandomAdjustBrightness': 2, 'RandomAdjustContrast': 3, 'RandomExpand': 4,
         'OneOf': 5, 'RandomCrop': 5, 'RandomHorizontalFlip': 6, 'RandomVerticalFlip': 6}
_KEEP = ('center_point', 'iou')


def _args(entry, allowed, who):
    args = dict(entry.get('args', {}) or {})
    unknown = sorted(set(args) - set(allowed))
    if unknown:
        raise ValueError(f'DeviceAugmentation: {who} does not take {unknown}')
    return args


def _range(value, who, what):
    lo, hi = (float(v) for v in value)
    if not lo <= hi:
        raise ValueError(f'DeviceAugmentation: {who}: {what}={value!r} is not a range')
    return lo, hi


def _crop_member(entry, who):
    a = _args(entry, ('min_iou', 'aspect_ratio_range', 'area_range', 'keep_criterion', 'min_objects_kept', 'p'), who)
    keep = a.get('keep_criterion', 'center_point')
    if keep not in _KEEP:
        raise ValueError(f'DeviceAugmentation: {who}: keep_criterion={keep!r}, expected one of {_KEEP}')
    return {'crop': True, 'min_iou': float(a.get('min_iou', .5)), 'aspect': _range(a.get('aspect_ratio_range', (0.5, 2.)), who, 'aspect_ratio_range'),
            'area': _range(a.get('area_range', (0.1, 1.)), who, 'area_range'), 'keep_iou': keep == 'iou',
            'min_kept': int(a.get('min_objects_kept', 1)), 'p': float(a.get('p', .5))}


_IDENTITY = {'crop': False, 'min_iou': 0.0, 'aspect': (1.0, 1.0), 'area': (1.0, 1.0), 'keep_iou': False, 'min_kept': 0, 'p': 0.0}


class AugmentParams(object):
    """What ``DeviceAugmentation.draw`` returns: ``records`` (PARAMS_DTYPE [B]), ``candidates`` (int32 [B, attempts, 4]: xmin, ymin, w, h
    relative to the image after its expand, all zero where the drawn window is larger than that image) and the ``sizes`` [(H, W)]."""

    def __init__(self, records, candidates, sizes):
        self.records, self.candidates, self.sizes = records, candidates, sizes

    def __len__(self):
        return len(self.records)


class DeviceAugmentation(object):
    """``DeviceAugmentation(augmentations, preprocessing, input_size, attempts=50)``: the two lists of ``{'name', 'args'}`` dicts and the
    ``input_size`` = (width, height) of a reference configuration.  An empty ``augmentations`` list is the evaluation pipeline."""

    def __init__(self, augmentations, preprocessing, input_size, attempts=50):
        if not input_size:
            raise ValueError('DeviceAugmentation: Resize is missing: input_size is required (every image of a batch becomes one tensor)')
        self.out_w, self.out_h = (int(v) for v in input_size)
        if self.out_w < 1 or self.out_h < 1:
            raise ValueError(f'DeviceAugmentation: Resize: input_size={input_size!r}')
        self.attempts = int(attempts)
        if self.attempts < 1:
            raise ValueError(f'DeviceAugmentation: attempts={attempts!r}')
        self.hue = self.saturation = self.brightness = self.contrast = self.expand = self.hflip = self.vflip = None
        self.members = []          # the OneOf's members (a single RandomCrop is a OneOf of one)
        rank, seen, to_float = -1, set(), False
        for entry in augmentations:
            name = entry['name']
            if name not in _RANK:
                raise ValueError(f'DeviceAugmentation: {name} is not supported on the device')
            if name in seen or _RANK[name] < rank or (_RANK[name] == 5 and rank == 5):
                raise ValueError(f'DeviceAugmentation: {name} is out of order: the one supported order is RandomAdjustHueSaturation, ToFloat, '
                                 'RandomAdjustBrightness, RandomAdjustContrast, RandomExpand, OneOf / RandomCrop, the flips')
            seen.add(name)
            rank = _RANK[name]
            if name == 'RandomAdjustHueSaturation':
                a = _args(entry, ('max_hue_delta', 'saturation_delta_range', 'p'), name)
                p = float(a.get('p', .5))
                if a.get('max_hue_delta'):
                    self.hue = (float(a['max_hue_delta']), p)
                if a.get('saturation_delta_range'):
                    self.saturation = (_range(a['saturation_delta_range'], name, 'saturation_delta_range'), p)
            elif name == 'ToFloat':
                _args(entry, (), name)
                to_float = True
            elif name == 'RandomAdjustBrightness':
                a = _args(entry, ('max_brightness_delta', 'p'), name)
                if not to_float:
                    raise ValueError(f'DeviceAugmentation: {name} needs ToFloat before it')
                self.brightness = (float(a['max_brightness_delta']), float(a.get('p', .5)))
            elif name == 'RandomAdjustContrast':
                a = _args(entry, ('contrast_delta_range', 'p'), name)
                if not to_float:
                    raise ValueError(f'DeviceAugmentation: {name} needs ToFloat before it')
                self.contrast = (_range(a['contrast_delta_range'], name, 'contrast_delta_range'), float(a.get('p', .5)))
            elif name == 'RandomExpand':
                a = _args(entry, ('aspect_ratio_range', 'area_range', 'p'), name)
                self.expand = (_range(a.get('aspect_ratio_range', (0.5, 2.0)), name, 'aspect_ratio_range'),
                               _range(a.get('area_range', (1.0, 16.0)), name, 'area_range'), float(a.get('p', .5)))
            elif name == 'RandomCrop':
                self.members = [_crop_member(entry, name)]
            elif name == 'OneOf':
                a = _args(entry, ('transforms',), name)
                for m in a.get('transforms', []):
                    if m['name'] == 'Identity':
                        self.members.append(dict(_IDENTITY))
                    elif m['name'] == 'RandomCrop':
                        self.members.append(_crop_member(m, 'OneOf[RandomCrop]'))
                    else:
                        raise ValueError(f"DeviceAugmentation: OneOf over {m['name']}: only Identity and RandomCrop members are supported")
                if not self.members:
                    raise ValueError('DeviceAugmentation: OneOf without members')
            elif name == 'RandomHorizontalFlip':
                self.hflip = float(_args(entry, ('p',), name).get('p', .5))
            elif name == 'RandomVerticalFlip':
                self.vflip = float(_args(entry, ('p',), name).get('p', .5))
        self.divide_255 = False
        mean, std = [0.0] * 3, [1.0] * 3
        names = [e['name'] for e in preprocessing]
        for name in names:
            if name not in ('ToFloatTensor', 'Normalize'):
                raise ValueError(f'DeviceAugmentation: {name} is not supported in preprocessing (ToFloatTensor, then Normalize)')
        if names not in (['ToFloatTensor'], ['ToFloatTensor', 'Normalize']):
            raise ValueError(f'DeviceAugmentation: preprocessing is {names}: expected ToFloatTensor, optionally followed by Normalize')
        for entry in preprocessing:
            if entry['name'] == 'ToFloatTensor':
                self.divide_255 = bool(_args(entry, ('normalize',), 'ToFloatTensor').get('normalize', False))
            else:
                a = _args(entry, ('mean', 'std'), 'Normalize')
                mean, std = self._triple(a.get('mean', 0.0), 'mean'), self._triple(a.get('std', 1.0), 'std')
        if any(s == 0 for s in std):
            raise ValueError(f'DeviceAugmentation: Normalize: std={std!r}')
        self.mean_std = np.array(list(mean) + list(std), np.float32)
        self.last_attempts = self.last_windows = None

    @staticmethod
    def _triple(value, what):
        vals = [float(v) for v in value] if isinstance(value, (list, tuple)) else [float(value)] * 3
        if len(vals) != 3:
            raise ValueError(f'DeviceAugmentation: Normalize: {what}={value!r} (a scalar or one value per RGB channel)')
        return vals

    # ---- host: the draws ---------------------------------------------------------------------------------------------------------------
    def draw(self, sizes, box_counts=None, rng=None):
        """``sizes``: [(H, W)] per image -> AugmentParams.  A handful of vectorised draws for the whole batch, no per-image loop.
        ``box_counts`` is accepted for symmetry with the reference's per-sample call and is not needed: whatever depends on the boxes (which
        candidate window is acceptable) is decided on the device."""
        rng = np.random.default_rng() if rng is None else rng
        sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
        B, T = len(sizes), self.attempts
        h, w = sizes[:, 0], sizes[:, 1]
        rec = np.zeros(B, PARAMS_DTYPE)
        rec['saturation'] = 1.0
        rec['contrast'] = 1.0
        flags = np.zeros(B, np.int32)
        if self.hue:                                        # transforms.py:141, :155
            on = rng.random(B) < self.hue[1]
            rec['hue_delta'] = np.where(on, rng.uniform(-self.hue[0], self.hue[0], B), 0.0)
            flags |= np.where(on, HUE_SATURATION, 0).astype(np.int32)
        if self.saturation:                                 # :142, :162
            on = rng.random(B) < self.saturation[1]
            rec['saturation'] = np.where(on, rng.uniform(*self.saturation[0], B), 1.0)
            flags |= np.where(on, HUE_SATURATION, 0).astype(np.int32)
        if self.brightness:                                 # :114
            on = rng.random(B) < self.brightness[1]
            rec['brightness'] = np.where(on, rng.uniform(-self.brightness[0], self.brightness[0], B) * 255., 0.0)
            flags |= np.where(on, BRIGHTNESS, 0).astype(np.int32)
        if self.contrast:                                   # :128
            on = rng.random(B) < self.contrast[1]
            rec['contrast'] = np.where(on, rng.uniform(*self.contrast[0], B), 1.0)
            flags |= np.where(on, CONTRAST, 0).astype(np.int32)
        cw, ch = w.copy(), h.copy()                         # the image after the expand
        if self.expand:                                     # functional/img.py:85-113: the first draw whose canvas is at least the image
            (alo, ahi), (slo, shi), p = self.expand
            on = rng.random(B) < p
            ar = rng.uniform(alo, ahi, (B, T))
            area = rng.uniform(slo, shi, (B, T)) * (h * w)[:, None]
            nw, nh = np.sqrt(area * ar).astype(np.int64), np.sqrt(area / ar).astype(np.int64)
            ok = (nw >= w[:, None]) & (nh >= h[:, None])
            first = ok.argmax(axis=1)
            on &= ok.any(axis=1)
            nw, nh = nw[np.arange(B), first], nh[np.arange(B), first]
            ex = rng.integers(0, np.where(on, nw - w, 0) + 1)
            ey = rng.integers(0, np.where(on, nh - h, 0) + 1)
            for key, val in (('expand_w', nw), ('expand_h', nh), ('expand_x', ex), ('expand_y', ey)):
                rec[key] = np.where(on, val, 0)
            cw, ch = np.where(on, nw, w), np.where(on, nh, h)
            flags |= np.where(on, EXPAND, 0).astype(np.int32)
        cand = np.zeros((B, T, 4), np.int32)
        if self.members:                                    # transforms.py:21, common.py:55, functional/img.py:55-83
            tab = self.members
            choice = rng.integers(0, len(tab), B)
            col = lambda key: np.array([m[key] for m in tab])[choice]   # noqa: E731
            on = col('crop') & (rng.random(B) < col('p'))
            aspect, area_r = np.array([m['aspect'] for m in tab])[choice], np.array([m['area'] for m in tab])[choice]
            ar = rng.uniform(aspect[:, :1], aspect[:, 1:], (B, T))
            area = rng.uniform(area_r[:, :1], area_r[:, 1:], (B, T)) * (ch * cw)[:, None]
            nw, nh = np.sqrt(area * ar).astype(np.int64), np.sqrt(area / ar).astype(np.int64)
            ok = (nw <= cw[:, None]) & (nh <= ch[:, None]) & (nw >= 1) & (nh >= 1) & on[:, None]
            x = rng.integers(0, np.where(ok, cw[:, None] - nw, 0) + 1)
            y = rng.integers(0, np.where(ok, ch[:, None] - nh, 0) + 1)
            cand = np.where(ok[:, :, None], np.stack([x, y, nw, nh], axis=2), 0).astype(np.int32)
            rec['min_iou'] = np.where(on, col('min_iou'), 0.0)
            rec['min_objects_kept'] = np.where(on, col('min_kept'), 0)
            flags |= np.where(on, CROP, 0).astype(np.int32) | np.where(on & col('keep_iou'), KEEP_IOU, 0).astype(np.int32)
        if self.hflip is not None:
            flags |= np.where(rng.random(B) < self.hflip, HFLIP, 0).astype(np.int32)
        if self.vflip is not None:
            flags |= np.where(rng.random(B) < self.vflip, VFLIP, 0).astype(np.int32)
        rec['flags'] = flags
        return AugmentParams(rec, np.ascontiguousarray(cand), [(int(a), int(b)) for a, b in sizes])

    # ---- device ------------------------------------------------------------------------------------------------------------------------
    def augment_padded(self, images, targets, params=None, rng=None):
        """``images``: list of ``uint8`` [H_i, W_i, 3] RGB tensors or arrays (host, or all on one device); ``targets``: list of [G_i, K]
        box rows (x1, y1, x2, y2, class, score, ...) in pixels of their image, K >= 4 and the same for the whole batch.
        -> ``(imgs [B, 3, out_h, out_w] fp32, rows [capacity, K], offsets int32 [B + 1])``, all on the device; no synchronisation.  The rows
        of image i are ``rows[offsets[i]:offsets[i + 1]]``; rows past ``offsets[-1]`` are padding; ``PackedGroundTruth(rows, offsets)`` is
        valid when K == 6.  ``self.last_attempts`` / ``self.last_windows`` keep the device tensors of the chosen attempt per image
        (-1: none acceptable, -2: no crop asked for) and of the composed window."""
        import torch
        from ... import _lib
        from ...detection.target_assigner import pack_ground_truth
        B = len(images)
        if B == 0 or len(targets) != B:
            raise ValueError(f'DeviceAugmentation: {B} images and {len(targets)} targets')
        images = [torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im for im in images]
        for im in images:
            if im.dtype != torch.uint8 or im.dim() != 3 or im.size(2) != 3 or im.size(0) < 1 or im.size(1) < 1:
                raise ValueError(f'DeviceAugmentation: images are uint8 [H, W, 3]; got {im.dtype} {tuple(im.shape)}')
        sizes = [(int(im.size(0)), int(im.size(1))) for im in images]
        if params is None:
            params = self.draw(sizes, rng=rng)
        if len(params) != B or list(params.sizes) != sizes:
            raise ValueError('DeviceAugmentation: params were drawn for other image sizes')
        on_device = [im.is_cuda for im in images]
        if any(on_device) and not all(on_device):
            raise ValueError('DeviceAugmentation: images partly on the host and partly on a device')
        device = images[0].device if on_device[0] else torch.device('cuda', torch.cuda.current_device())
        lib = _lib.lib()

        nbytes = np.array([3 * h * w for h, w in sizes], np.int64)
        desc = np.zeros(B, IMAGE_DTYPE)
        desc['offset'] = np.concatenate([[0], np.cumsum(nbytes)[:-1]])
        desc['height'], desc['width'] = [s[0] for s in sizes], [s[1] for s in sizes]
        cand = np.ascontiguousarray(params.candidates, np.int32)
        T = int(cand.shape[1])
        head = [desc.view(np.uint8), np.ascontiguousarray(params.records).view(np.uint8), cand.reshape(-1).view(np.uint8)]
        head_bytes = sum(a.size for a in head)              # (every part a multiple of 16 bytes)
        pixel_bytes = int(nbytes.sum())
        # one pinned staging buffer, one H2D copy: descriptors | records | candidates | pixels
        stage = torch.empty((head_bytes + (0 if on_device[0] else pixel_bytes),), dtype=torch.uint8)
        if torch.cuda.is_available():
            stage = stage.pin_memory()
        view = stage.numpy()
        pos = 0
        for a in head:
            view[pos:pos + a.size] = a
            pos += a.size
        if on_device[0]:
            pixels = torch.cat([im.contiguous().reshape(-1) for im in images])
        else:
            for im, n in zip(images, nbytes):
                view[pos:pos + n] = im.contiguous().reshape(-1).numpy()
                pos += int(n)
        dev = stage.to(device, non_blocking=True)
        if not on_device[0]:
            pixels = dev[head_bytes:]
        base = dev.data_ptr()
        p_desc, p_rec, p_cand = base, base + B * IMAGE_DTYPE.itemsize, base + B * (IMAGE_DTYPE.itemsize + PARAMS_DTYPE.itemsize)

        targets = [torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t for t in targets]
        widths = {int(t.shape[1]) for t in targets if t.dim() == 2}
        if len(widths) > 1:
            raise ValueError(f'DeviceAugmentation: ground-truth rows of different widths in one batch: {sorted(widths)}')
        K = widths.pop() if widths else 6
        if K < 4:
            raise ValueError(f'DeviceAugmentation: ground-truth rows of {K} columns')
        rows, offs, total = pack_ground_truth(list(targets), device, row=K)
        rows_out = torch.empty((max(total, 1), K), dtype=torch.float32, device=device)
        offs_out = torch.empty((B + 1,), dtype=torch.int32, device=device)
        attempt = torch.empty((B,), dtype=torch.int32, device=device)
        windows = torch.empty((B, 4), dtype=torch.int32, device=device)
        imgs = torch.empty((B, 3, self.out_h, self.out_w), dtype=torch.float32, device=device)
        stream = _lib.current_stream()
        with torch.cuda.device(device):
            ws = _lib.scratch(lib.ssdk_augment_boxes_workspace_bytes(B), device, 'augment_boxes')
            _lib.check(lib.ssdk_augment_boxes(C.c_void_p(p_desc), C.c_void_p(p_rec), C.c_void_p(p_cand), T, _lib.ptr(rows) if total else None, K,
                                              _lib.ptr(offs), B, total, self.out_w, self.out_h, _lib.ptr(rows_out), _lib.ptr(offs_out),
                                              _lib.ptr(attempt), _lib.ptr(windows), _lib.ptr(ws), ws.numel(), stream), 'ssdk_augment_boxes')
            ws = _lib.scratch(lib.ssdk_augment_images_workspace_bytes(B), device, 'augment_images')
            _lib.check(lib.ssdk_augment_images(C.c_void_p(pixels.data_ptr()), pixel_bytes, C.c_void_p(p_desc), C.c_void_p(p_rec), _lib.ptr(windows), B,
                                               self.out_w, self.out_h, int(self.divide_255), self.mean_std.ctypes.data_as(C.c_void_p),
                                               _lib.ptr(imgs), _lib.ptr(ws), ws.numel(), stream), 'ssdk_augment_images')
        self.last_attempts, self.last_windows = attempt, windows
        imgs._ssdk_keepalive = (dev, pixels, rows, offs)    # until the stream has consumed them
        return imgs, rows_out, offs_out

    def __call__(self, images, targets, rng=None):
        """-> ``(imgs, [rows of image i])``: the shape ``BatchContainer`` and ``step_fn`` take.  One D2H copy, of the offsets."""
        imgs, rows, offs = self.augment_padded(images, targets, rng=rng)
        o = offs.cpu().tolist()
        return imgs, [rows[o[i]:o[i + 1]] for i in range(len(o) - 1)]
