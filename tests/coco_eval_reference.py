"""The COCO bbox evaluation rules (COCOeval.evaluateImg / accumulate / summarize) restated in numpy: literal loops, fp64 throughout,
nothing shared with the device code.  The yardstick of tests/test_coco_eval.py (hand-worked values) and tests/test_coco_eval_gpu.py."""
import numpy as np

STAT_NAMES = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')


def default_tables():
    return (np.linspace(.5, .95, 10), np.linspace(0, 1, 101), np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64),
            np.array([1, 10, 100], np.int32))


def box_area(b):
    b = np.asarray(b, np.float64)
    return (b[2] - b[0]) * (b[3] - b[1])


def iou(d, g, crowd):
    d, g = np.asarray(d, np.float64), np.asarray(g, np.float64)
    iw = min(d[2], g[2]) - max(d[0], g[0])
    ih = min(d[3], g[3]) - max(d[1], g[1])
    inter = max(0.0, iw) * max(0.0, ih)
    den = box_area(d) if crowd else box_area(d) + box_area(g) - inter
    return 0.0 if den == 0.0 else inter / den


def evaluate(pred, gts, num_classes, gt_areas=None, image_area_scale=None, iou_thrs=None, rec_thrs=None, area_rngs=None, max_dets=None):
    """-> dict: precision [T, R, K, A, M], recall [T, K, A, M], stats {name: float}, rank int32 [N] (-1: foreign class), flags uint8 [N, T * A]
    (bit 0 matched, bit 1 ignored), order int64 [N] (class, score desc, image, row; foreign classes last), npig int32 [K, A]."""
    d_iou, d_rec, d_area, d_max = default_tables()
    iou_thrs = np.asarray(d_iou if iou_thrs is None else iou_thrs, np.float64)
    rec_thrs = np.asarray(d_rec if rec_thrs is None else rec_thrs, np.float64)
    area_rngs = np.asarray(d_area if area_rngs is None else area_rngs, np.float64).reshape(-1, 2)
    max_dets = np.asarray(d_max if max_dets is None else max_dets, np.int64)
    pred = np.asarray(pred, np.float32).reshape(-1, 7)
    T, R, A, M, K, N = len(iou_thrs), len(rec_thrs), len(area_rngs), len(max_dets), num_classes, pred.shape[0]
    num_images = len(gts)
    img = pred[:, 0].astype(np.int64)
    cls = pred[:, 5].astype(np.int64)
    score = pred[:, 6]
    foreign = (cls < 0) | (cls >= K)

    def scale_of(i):
        return 1.0 if image_area_scale is None or not 0 <= i < num_images else float(image_area_scale[i])

    # ground truth per image: class, crowd flag, the area it is binned by
    g_cls, g_crowd, g_area = [], [], []
    for i, g in enumerate(gts):
        g = np.asarray(g, np.float32)
        g_cls.append(g[:, 4].astype(np.int64))
        g_crowd.append(g[:, 6] != 0 if g.shape[1] > 6 else np.zeros(g.shape[0], bool))
        own = np.array([box_area(b[:4]) for b in g], np.float64) if gt_areas is None else np.asarray(gt_areas[i], np.float64)
        g_area.append(own.reshape(-1) * scale_of(i))

    npig = np.zeros((K, A), np.int32)
    for i in range(num_images):
        for j in range(len(g_cls[i])):
            k = g_cls[i][j]
            if 0 <= k < K and not g_crowd[i][j]:
                for a in range(A):
                    if not (g_area[i][j] < area_rngs[a, 0] or g_area[i][j] > area_rngs[a, 1]):
                        npig[k, a] += 1

    rank = np.full(N, -1, np.int32)
    flags = np.zeros((N, T * A), np.uint8)
    for i in sorted(set(img.tolist())):
        for k in sorted(set(cls[(img == i) & ~foreign].tolist())):
            rows = np.nonzero((img == i) & (cls == k))[0]
            rows = rows[np.argsort(-score[rows], kind='mergesort')]
            rank[rows] = np.arange(len(rows))
            rows = rows[:max_dets[-1]]
            gi = np.nonzero(g_cls[i] == k)[0] if 0 <= i < num_images else np.zeros(0, np.int64)
            ious = [[iou(pred[r, 1:5], gts[i][j][:4], g_crowd[i][j]) for j in gi] for r in rows]   # (the same for every t and a)
            for a in range(A):
                lo, hi = area_rngs[a]
                g_ign = np.array([bool(g_crowd[i][j]) or g_area[i][j] < lo or g_area[i][j] > hi for j in gi], bool)
                order = np.argsort(g_ign, kind='mergesort')          # the counted gts first, each part in row order
                for t in range(T):
                    taken = np.zeros(len(gi), bool)
                    for ri, r in enumerate(rows):
                        best = min(iou_thrs[t], 1 - 1e-10)
                        m = -1
                        for o in order:
                            j = gi[o]
                            if taken[o] and not g_crowd[i][j]:
                                continue
                            if m > -1 and not g_ign[m] and g_ign[o]:
                                break
                            v = ious[ri][o]
                            if v < best:
                                continue
                            best, m = v, o
                        if m > -1:
                            taken[m] = True
                            ign = g_ign[m]
                        else:
                            ar = box_area(pred[r, 1:5]) * scale_of(i)
                            ign = ar < lo or ar > hi
                        flags[r, t * A + a] = (1 if m > -1 else 0) | (2 if ign else 0)

    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    order_all = []
    for k in range(K):
        rows_k = np.nonzero(cls == k)[0]
        rows_k = rows_k[np.argsort(img[rows_k], kind='mergesort')]           # concatenated image by image ...
        rows_k = rows_k[np.argsort(-score[rows_k], kind='mergesort')]        # ... then merge-sorted by score
        order_all.append(rows_k)
        for a in range(A):
            if npig[k, a] == 0:
                continue
            for m in range(M):
                kept = rows_k[rank[rows_k] < max_dets[m]]
                nd = len(kept)
                for t in range(T):
                    f = flags[kept, t * A + a]
                    tp = np.cumsum(f == 1, dtype=np.float64)
                    fp = np.cumsum(f == 0, dtype=np.float64)
                    rc = tp / npig[k, a]
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(R)
                    inds = np.searchsorted(rc, rec_thrs, side='left')
                    for ri, pi in enumerate(inds):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    frows = np.nonzero(foreign)[0]
    order_all.append(frows[np.argsort(img[frows], kind='mergesort')])
    order = np.concatenate(order_all).astype(np.int64) if N else np.zeros(0, np.int64)
    return dict(precision=precision, recall=recall, stats=summarize(precision, recall, iou_thrs), rank=rank, flags=flags, order=order, npig=npig)


def summarize(precision, recall, iou_thrs):
    T, R, K, A, M = precision.shape

    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    def pick(want):
        hit = np.nonzero(np.abs(np.asarray(iou_thrs) - want) < 1e-9)[0]
        return int(hit[0]) if hit.size else None

    def ap(a, t=None, named=False):
        if a >= A or (named and t is None):
            return -1.0
        return mean(precision[:, :, :, a, M - 1] if t is None else precision[t, :, :, a, M - 1])

    def ar(a, m):
        return mean(recall[:, :, a, m]) if a < A and m < M else -1.0

    return {'AP': ap(0), 'AP50': ap(0, pick(0.5), True), 'AP75': ap(0, pick(0.75), True), 'APs': ap(1), 'APm': ap(2), 'APl': ap(3),
            'AR1': ar(0, 0), 'AR10': ar(0, 1), 'AR100': ar(0, 2), 'ARs': ar(1, M - 1), 'ARm': ar(2, M - 1), 'ARl': ar(3, M - 1)}
