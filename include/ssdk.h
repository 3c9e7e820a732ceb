/*
 * ssdk.h -- C ABI of libssdk, the MI355X (gfx950) implementation of the single-shot-detection hot path.
 *
 * One entry point per reference function on the path; the comment on each declaration cites the
 * reference interface it replaces (paths relative to the reference repository root).  Rules of the boundary:
 *   - every pointer marked DEV is device memory owned by the caller (torch); the library never allocates or
 *     frees device memory on the hot path and keeps no pointer past the call; workspaces are caller-provided,
 *     sized by the matching *_workspace_bytes() query;
 *   - every launch goes to the hipStream_t passed as `stream` (void*; NULL = the null stream); no call
 *     synchronises the device;
 *   - return value: 0 ok, <0 invalid argument (SSDK_E_*), >0 a hipError_t; no exception crosses the boundary;
 *     ssdk_last_error_string() gives the thread's last message;
 *   - fp32 everywhere unless stated; layouts are the reference's: scores [B, A*C] anchor-major/class-minor,
 *     locs [B, A*4], anchors/priors [A,4] = (cx, cy, w, h) in pixels, target [B, A, 6] =
 *     (x1, y1, x2, y2, class, score), ground-truth rows (x1, y1, x2, y2, class, score[, difficult]).
 */
#ifndef SSDK_H_
#define SSDK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSDK_VERSION 133

#define SSDK_OK 0
#define SSDK_E_INVALID (-1)   /* bad argument / shape */
#define SSDK_E_WORKSPACE (-2) /* workspace missing or too small */
#define SSDK_E_UNSUPPORTED (-3)
#define SSDK_E_STREAMK_TIMEOUT (-4) /* a stream-K head GEMM gave up on a parked partial tile (see ssdk_heads_fwd_timeouts) */

/* detection/matcher.py:4-5 */
#define SSDK_NOT_MATCHED (-2)
#define SSDK_IGNORE (-1)
/* force stage of ssdk_encode_ground_truth_ex */
#define SSDK_FORCE_MATCH_PER_PREDICTION 0 /* matcher.py:52-54: every box's best anchor, the highest box index wins a shared one */
#define SSDK_FORCE_MATCH_BIPARTITE 1      /* matcher.py:7-31: greedy bipartite matching, every box an anchor of its own */

/* classification loss kinds (bf/modules/losses.py) */
#define SSDK_CLS_CROSS_ENTROPY 0 /* torch.nn.CrossEntropyLoss(reduction='sum', ignore_index=-1), losses.py:4 */
#define SSDK_CLS_SIGMOID_FOCAL 1 /* SigmoidFocalLoss, losses.py:34-54 */
#define SSDK_CLS_SOFTMAX_FOCAL 2 /* SoftmaxFocalLoss, losses.py:56-78 */
#define SSDK_CLS_CE_SOFT 3       /* CrossEntropyWithSoftTargetsLoss, losses.py:80-93 (target of multibox_loss.py:68-71) */
#define SSDK_CLS_BCE_SOFT 4      /* BinaryCrossEntropyWithSoftTargetsLoss, losses.py:95-106 (target of multibox_loss.py:64-67) */
/* IoU-aware sigmoid kinds (not in the reference).  For one logit x with target y in [0, 1]: s = 1 / (1 + exp(-x)),
 * bce(x, y) = max(x, 0) - x y + log1p(exp(-|x|)).  The target row is the multiclass layout of multibox_loss.py:64-67 (the column of
 * class k is k - 1): a positive row (class not 0 / -1) has y = w * q in its class column and 0 elsewhere, every other sampled row
 * (a sampled ignore row included) is all zeros.  w = target column 5 (the mixup weight), q = the quality: 1 with
 * quality_from_iou == 0; otherwise the plain IoU (inter / union, clamped to [0, 1], 0 where the union is not positive or the quotient
 * not finite) of the prediction's decoded corners (box_coder.py:55-57 + to_corners) against the row's RAW target corners.  q is a
 * constant of the step: no gradient reaches locs through it. */
#define SSDK_CLS_QUALITY_FOCAL 5 /* Quality Focal Loss (arXiv:2006.04388), beta = focal_gamma >= 1:
                                    value |y - s|^beta bce(x, y),
                                    gradient beta |y - s|^(beta - 1) sgn(s - y) s (1 - s) bce(x, y) + |y - s|^beta (s - y), sgn(0) = 0 */
#define SSDK_CLS_VARIFOCAL 6     /* Varifocal Loss (arXiv:2008.13367), alpha = focal_alpha in [0, 1], gamma = focal_gamma >= 0:
                                    y > 0:  value y bce(x, y), gradient y (s - y);
                                    y == 0: value alpha s^gamma bce(x, 0), gradient alpha s^gamma (gamma (1 - s) bce(x, 0) + s) */
/* localisation loss kinds */
#define SSDK_LOC_SMOOTH_L1 0 /* torch.nn.SmoothL1Loss(reduction='sum') on box_coder-encoded targets, multibox_loss.py:81-86 */
#define SSDK_LOC_GIOU 1      /* GeneralizedIoULoss, losses.py:109-114, on decoded corners (multibox_loss.py:77-79) */
/* torch.nn.modules.loss re-exported by losses.py:4, reduction='sum', on the encoded targets like SSDK_LOC_SMOOTH_L1 (d = loc - target) */
#define SSDK_LOC_L1 2        /* torch.nn.L1Loss: |d|, gradient sign(d) with sign(0) = 0 (torch.nn.functional.l1_loss) */
#define SSDK_LOC_MSE 3       /* torch.nn.MSELoss: d^2, gradient 2d (torch.nn.functional.mse_loss) */
#define SSDK_LOC_HUBER 4     /* torch.nn.HuberLoss(delta = smooth_l1_beta): |d| < delta ? d^2 / 2 : delta (|d| - delta / 2),
                                gradient d clamped to [-delta, delta] (torch.nn.functional.huber_loss) */
/* IoU-based kinds on decoded corners, like SSDK_LOC_GIOU: P = the prediction's decoded corner box, T = the row's RAW target corners, and
 * the target is left alone.  (5, 6 and 7 are no kinds: refused.)  iou = inter / uni exactly as SSDK_LOC_GIOU computes it, no epsilon;
 * eps = 1e-7 only in the denominators these terms add.  cw = max(P.x2, T.x2) - min(P.x1, T.x1), ch likewise, c2 = cw^2 + ch^2 + eps;
 * rho2 = the squared distance of the two centres; w, h of P and wg, hg of T are plain differences.  Gradients: max / min to the selected
 * argument, half each at an exact tie, clamp(0) passes where its argument is >= 0 (torch autograd's rules, SSDK_LOC_GIOU's). */
#define SSDK_LOC_IOU 8       /* IoULoss: 1 - iou */
#define SSDK_LOC_DIOU 9      /* DistanceIoULoss (arXiv:1911.08287): 1 - iou + rho2 / c2 */
#define SSDK_LOC_CIOU 10     /* CompleteIoULoss (same paper): DIoU + alpha v, v = 4 / pi^2 (atan(wg / hg) - atan(w / h))^2,
                                alpha = v / (1 - iou + v + eps), a constant of the step: the gradient is alpha dv */
#define SSDK_LOC_EIOU 11     /* EfficientIoULoss (arXiv:2101.08158, without the focal factor):
                                DIoU + (w - wg)^2 / (cw^2 + eps) + (h - hg)^2 / (ch^2 + eps) */

int ssdk_version(void);

/*
 * bf/utils/box_utils.py:16-194 as a callable surface (every array DEV fp32; boxes 16-byte aligned rows of 4; no workspace unless said).
 *   ssdk_box_to_corners    :16-23   [cx,cy,w,h] -> [c - wh/2, c + wh/2]                                  box, out [n,4] (out may be box)
 *   ssdk_box_to_centroids  :25-36   inplace_form = 0: [(max+min)/2, max-min] (:36); != 0: wh = max-min, c = min + wh/2 (:33-34) -- the two
 *                                   forms round the centre differently, both as the reference does
 *   ssdk_box_area          :38-46   clamp(x2-x1, 0) * clamp(y2-y1, 0)                                     out [n]
 *   ssdk_box_intersection  :49-80   cat([max of the min corners, min of the max corners]); cartesian != 0: out [na,nb,4], else na == nb and
 *                                   out [na,4]; zero_incorrect != 0: rows with max < min in any coordinate become 0
 *   ssdk_box_iou           :83-101 (generalized = 0) / :104-143 (generalized != 0): cartesian != 0: out [na,nb], else out [na].  No +1, no
 *                                   epsilon: two degenerate boxes give NaN like the reference.  The [G,A] matrix ssdk_match_per_prediction takes.
 *   ssdk_nms               :145-194 ONE problem (n <= 65536; the batched fused path is ssdk_postprocess): max_per_class in 1..n-1 first keeps
 *                                   the max_per_class best scores (:186-188 topk(sorted=False): the reference defines the SET; here it is kept
 *                                   in descending score order, ties by ascending index); then soft == 0: hard NMS per torchvision.ops.nms's
 *                                   documented contract (:193; PARITY UNPINNED: torchvision is not vendored), soft != 0: _soft_nms (:145-163,
 *                                   incl. its loop condition mask.nonzero().sum()).  picked DEV int64 [>= min(n, cap)]: positions, in pick
 *                                   order, in the array the NMS ran on (the input, or the top-k subset when a cap applied); picked_boxes
 *                                   DEV [.,4] / picked_scores DEV [.] (NULL: not wanted): boxes[picked] / scores[picked]; count DEV int32.
 */
int ssdk_box_to_corners(const float* box, float* out, long long n, void* stream);
int ssdk_box_to_centroids(const float* box, float* out, long long n, int inplace_form, void* stream);
int ssdk_box_area(const float* box, float* out, long long n, void* stream);
int ssdk_box_intersection(const float* a, int na, const float* b, int nb, int cartesian, int zero_incorrect, float* out, void* stream);
int ssdk_box_iou(const float* a, int na, const float* b, int nb, int cartesian, int generalized, float* out, void* stream);
/* The IoU-based box terms row by row (csrc/iou_loss.h: the arithmetic of the fused loss kernels, the same bits).  kind = SSDK_LOC_GIOU,
 * _IOU, _DIOU, _CIOU or _EIOU (anything else: SSDK_E_INVALID); pred, target DEV [n,4] corner boxes, 16-byte aligned.
 *   _fwd: out DEV [n] = the kind's value of row i.
 *   _bwd: dpred DEV [n,4] (16-byte aligned) = grad_rows[i] * d value_i / d pred_i, grad_rows DEV [n].  No gradient towards target. */
int ssdk_box_iou_loss_fwd(int kind, const float* pred, const float* target, long long n, float* out, void* stream);
int ssdk_box_iou_loss_bwd(int kind, const float* pred, const float* target, const float* grad_rows, long long n, float* dpred, void* stream);
size_t ssdk_nms_workspace_bytes(int n);
int ssdk_nms(const float* boxes, const float* scores, int n, float overlap_threshold, float score_threshold, int max_per_class, int soft,
             float sigma, long long* picked, float* picked_boxes, float* picked_scores, int* count, void* workspace, size_t workspace_bytes,
             void* stream);

/*
 * DETERMINISTIC MODE (process-wide; default off, or SSDK_DETERMINISTIC=1 in the environment).  The reference runs every GPU job with
 * torch.backends.cudnn.deterministic = True / benchmark = False (bf/training/env.py:74-76).  Off, several kernels add fp32 partial
 * results with atomics in the order the hardware happens to retire them: split-K convolutions (forward too), the scatter form of the
 * data gradients, the K-split weight gradients, the bias-gradient column sums.  On, every fp32 sum is taken in an order fixed by the
 * launch: convolutions are not split over K with atomics (stream-K's parked partial tiles are already added in range order), the data
 * gradient of a strided convolution is a row matrix of contributions plus a per-pixel sum in a fixed order, weight gradients write one
 * partial tile per K split and a second kernel adds the partials in split order, bias gradients likewise.  (The heads' backward is the
 * same in both modes since round 5: rows in pixel order, plain stores, ordered sums -- no atomics either way.)  Same inputs ->
 * the same bits, run to run and eager vs HIP-graph replay; the cost is reported by bench.py (per_config[*].deterministic_ms_per_step).
 * (The BatchNorm sums stay fp64 atomics over per-workgroup fp32 partials: such sums are exact -- hence order-independent -- unless the
 * partials span more than ~2^18 in magnitude.)  The workspace sizes of ssdk_heads_bwd / ssdk_conv2d_bwd depend on the mode: size and
 * call under the same setting.  Returns the previous setting.
 */
int ssdk_set_deterministic(int enabled);
int ssdk_get_deterministic(void);
const char* ssdk_last_error_string(void);

/* ---- anchors ------------------------------------------------------------------------------------------------ */

/*
 * Host helper: per-level box sizes of detection/anchor_generators/ssd.py:55-104,125-136 (SsdAnchorGenerator with
 * num_branches = 1, flip = True).  `ratios` are the level's aspect_ratios before flipping; min_scale/max_scale are
 * the fp32 values scales[i], scales[i+1] of ssd.py:33.  Writes nb x (w, h) to hws (host, capacity hws_cap pairs)
 * and returns nb (>0) or an error (<0).
 */
int ssdk_anchor_sizes_ssd(const double* ratios, int nratio, float min_scale, float max_scale, int img_w, int img_h,
                          float* hws, int hws_cap);

/* Host helper: detection/anchor_generators/retina_net.py:18-26,40-43 box sizes (scale-major, ratio-minor). */
int ssdk_anchor_sizes_retina(const double* ratios, int nratio, int level, double scale, int scales_per_level,
                             float* hws, int hws_cap);

/* Host helper: torch.linspace(start, end, steps) fp32 as used by ssd.py:33 for the scale table. */
int ssdk_linspace_f32(float start, float end, int steps, float* out);

/*
 * Device: one level of _generate_anchors (ssd.py:106-151 / retina_net.py:28-54): out DEV [H, W, nb, 4] with
 * centres linspace((0.5)*step, (0.5 + n - 1)*step, n), step = img / n, and the given (w, h) table (host, nb pairs).
 */
int ssdk_anchors_level(float* out, int layer_h, int layer_w, int nb, const float* hws_host, int img_w, int img_h,
                       void* stream);
/* The same with the generator's `step` and `offset` given (ssd.py:111-118,138-139: step_w = step or img_w / layer_w; centres
 * linspace(offset * step, (offset + n - 1) * step, n)); ssdk_anchors_level is step = img / n, offset = (.5, .5). */
int ssdk_anchors_level_ex(float* out, int layer_h, int layer_w, int nb, const float* hws_host, double step_w, double step_h,
                          double offset_x, double offset_y, void* stream);

/* ---- target assignment (T1 + T2 + T3) ------------------------------------------------------------------------- */

size_t ssdk_encode_ground_truth_workspace_bytes(int batch, int total_gt);

/*
 * detection/target_assigner.py:22-63 TargetAssigner.encode_ground_truth, with bf/utils/box_utils.py:83-101 (iou)
 * and detection/matcher.py:33-56 (match_per_prediction, force_match_for_each_target=True) fused.
 *   gt_rows    DEV [total_gt, gt_stride] rows of all images back to back, gt_stride >= 6.  total_gt may be a fixed CAPACITY larger than
 *              gt_offsets[batch] (static buffers of a captured HIP graph): rows past gt_offsets[batch] are padding and ignored
 *   gt_offsets DEV int32 [batch + 1], image i owns rows gt_offsets[i] .. gt_offsets[i+1]
 *   anchors    DEV [A, 4] centroid form
 *   target     DEV [batch, A, 6] (written in full)
 *   box_idx    DEV int32 [batch, A] or NULL: the matcher's box_idx (-2 not matched, -1 ignore, >= 0 GT index)
 */
int ssdk_encode_ground_truth(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                             const float* anchors, int num_anchors, float matched_threshold,
                             float unmatched_threshold, float* target, int32_t* box_idx, void* workspace,
                             size_t workspace_bytes, void* stream);

size_t ssdk_match_per_prediction_workspace_bytes(int num_boxes);
/*
 * detection/matcher.py:33-56 match_per_prediction on a given weight matrix: weights DEV [num_boxes, num_anchors] (any values; NaN
 * ranks above everything, as in torch.max / argmax); box_idx DEV int64 [num_anchors] = argmax over the boxes (first maximum),
 * SSDK_NOT_MATCHED below unmatched_threshold, SSDK_IGNORE in [unmatched, matched); force_match_for_each_target != 0: every box's
 * best anchor (first maximum) is given to it, the highest box index winning an anchor several boxes claim (:52-54).
 */
int ssdk_match_per_prediction(const float* weights, int num_boxes, int num_anchors, float matched_threshold,
                              float unmatched_threshold, int force_match_for_each_target, int64_t* box_idx, void* workspace,
                              size_t workspace_bytes, void* stream);

size_t ssdk_match_bipartite_workspace_bytes(int num_boxes, int num_anchors);
/*
 * detection/matcher.py:7-31 match_bipartite on a given weight matrix: weights DEV [num_boxes, num_anchors].  num_boxes times: the
 * argmax of the whole matrix (first flat index on ties: the lowest row, then the lowest column) gives that row that column, then the
 * column and the row are zeroed.  anchor_idx DEV int64 [num_boxes] (the reference's box_idx is arange(num_boxes)); num_matched DEV
 * int32 [1]: the rounds whose maximum was above 0.
 *   EXHAUSTION: once the maximum is 0 (two boxes whose only positive entry is the same column, or num_boxes > num_anchors) every later
 *   round of the reference lands on flat index 0: it sets anchor_idx[0] = 0 and leaves the other left-over boxes' entries
 *   uninitialised.  Reproduced: anchor_idx[0] == 0 whenever a box was left over; the left-over boxes' entries are -1 here.
 *   inplace != 0: `weights` is the working matrix and is left as the reference leaves it (all zeros when every box got an anchor; after
 *   exhaustion the same zeroed rows and columns, row 0 and column 0 included).  inplace == 0: `weights` is only read (a copy in the
 *   workspace is matched).
 * NaN entries rank below everything (the reference asserts weights.max(dim=1) > 0 first, which a NaN row fails; that assert, with its
 * sync, is the Python wrapper's).  One workgroup; ends for any input.
 */
int ssdk_match_bipartite(float* weights, int num_boxes, int num_anchors, int inplace, int64_t* anchor_idx, int32_t* num_matched,
                         void* workspace, size_t workspace_bytes, void* stream);

size_t ssdk_encode_ground_truth_ex_workspace_bytes(int batch, int total_gt, int force_match);
/*
 * ssdk_encode_ground_truth with the force stage chosen by `force_match` (the other arguments as there):
 *   SSDK_FORCE_MATCH_PER_PREDICTION  ssdk_encode_ground_truth itself.
 *   SSDK_FORCE_MATCH_BIPARTITE       box_idx = match_per_prediction(iou, ..., force_match_for_each_target=False) (matcher.py:45-50), then
 *                                    box_idx[anchor_idx] = arange(G) with anchor_idx from match_bipartite(iou) (matcher.py:7-31), per
 *                                    image: one more launch (one workgroup per image) between the two of the default form; still
 *                                    nothing [G, A]-shaped.  Unlike ssdk_match_bipartite, the stage STOPS at the first maximum that is
 *                                    not above 0 (NaN included): the boxes left over get no forced anchor and box 0 keeps its own.
 *                                    Any number of boxes per image; num_anchors <= 262144 (SSDK_E_UNSUPPORTED above).
 */
int ssdk_encode_ground_truth_ex(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                                const float* anchors, int num_anchors, float matched_threshold, float unmatched_threshold,
                                int force_match, float* target, int32_t* box_idx, void* workspace, size_t workspace_bytes,
                                void* stream);

#define SSDK_ATSS_MAX_LEVELS 16
#define SSDK_ATSS_MAX_TOPK 32
size_t ssdk_encode_ground_truth_atss_workspace_bytes(int batch, int total_gt, int n_levels);
/*
 * Target assignment by Adaptive Training Sample Selection (arXiv:1912.02424, Algorithm 1; the reference has no such assigner).  Inputs and
 * outputs as for ssdk_encode_ground_truth, without thresholds:
 *   level_sizes HOST int32 [n_levels], positive, summing to num_anchors: pyramid level l owns the next level_sizes[l] anchors.  Read during
 *               the call (the kernels get the table by value), so the call may sit in a captured HIP graph.
 *   topk        candidates per (box, level), 1..SSDK_ATSS_MAX_TOPK; n_levels 1..SSDK_ATSS_MAX_LEVELS.
 * For every box g = (x1, y1, x2, y2, ...) of an image, all box arithmetic in fp32, one operation at a time:
 *   1. gcx = (x1 + x2) * 0.5f, gcy = (y1 + y2) * 0.5f; d2(a) = (cx_a - gcx)^2 + (cy_a - gcy)^2.
 *   2. Candidates: per level the min(topk, level size) anchors of smallest d2, ties to the lower anchor index, a NaN distance last.
 *   3. t_g = (float)(mean + std) of the n candidates' IoUs (the IoU of ssdk_encode_ground_truth), accumulated in fp64: mean = sum v / n,
 *      std = sqrt(sum (v - mean)^2 / (n - 1)), 0 when n == 1.
 *   4. A candidate a qualifies when iou(a, g) >= t_g and x1 < cx_a < x2 and y1 < cy_a < y2 (NaN never qualifies).
 *   5. An anchor that qualifies for several boxes takes the largest IoU, then the lowest box index.
 * box_idx[a] is that box or SSDK_NOT_MATCHED: no ignore band and NO force stage -- a box none of whose candidates qualifies has no positive
 * anchor.  Target rows: the box's six columns for a matched anchor, (0, 0, 0, 0, 0, 1) for every other.  Two launches, no host
 * synchronisation, the same bits run to run.
 */
int ssdk_encode_ground_truth_atss(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                                  const float* anchors, int num_anchors, const int32_t* level_sizes, int n_levels, int topk,
                                  float* target, int32_t* box_idx, void* workspace, size_t workspace_bytes, void* stream);

#define SSDK_TAL_MAX_TOPK 32
size_t ssdk_encode_ground_truth_tal_workspace_bytes(int batch, int total_gt, int topk);
/*
 * Target assignment by Task Alignment Learning (TOOD, arXiv:2108.07755 section 3.2; ABI 128; the reference has no such assigner).  An
 * anchor is positive for a box when its OWN prediction agrees with the box, and the classifier's target is that agreement.  gt_rows,
 * gt_stride, gt_offsets, batch, total_gt, anchors, target, box_idx as for ssdk_encode_ground_truth; beside them
 *   scores      DEV [batch, A, num_columns] class LOGITS in the sigmoid layout (class k is column k - 1), num_columns >= 1
 *   locs        DEV [batch, A, 4] encoded boxes (16-byte aligned, as the anchors)
 *   xy_scale, wh_scale   the box coder's
 *   topk        candidates per box, 1..SSDK_TAL_MAX_TOPK; alpha, beta: finite, >= 0 (TOOD: 1 and 6)
 * The predictions are only read: constants of the step.  For every box g = (x1, y1, x2, y2, class, score) of an image and every anchor
 * a = (cx, cy, w, h), all arithmetic in fp32, one operation at a time, nothing contracted:
 *   1. P_a = corners of (cx + w * tx / xy_scale, cy + h * ty / xy_scale, w * expf(tw / wh_scale), h * expf(th / wh_scale)): the decoded
 *      prediction of ssdk_multibox_loss_*'s GIoU term and of the soft-target losses' quality.
 *   2. u(a, g) = the plain IoU of P_a with (x1, y1, x2, y2), exactly the quality q of the soft-target losses: inter / union, clamped to
 *      [0, 1], 0 where the union is not positive or the quotient is not finite.
 *   3. s(a, g) = 1 / (1 + __expf(-scores[a, k - 1])) with k = (int)class; 0 when class is not within 1..num_columns (NaN included).
 *   4. a is INSIDE g when x1 < cx < x2 and y1 < cy < y2: the anchor's own centre, as rule 4 of ssdk_encode_ground_truth_atss; NaN is
 *      never inside.
 *   5. m(a, g) = s^alpha * u^beta.  x^e is 1 for e == 0 (also 0^0), x for 1, x * x for 2; u^6 is (u * u)^3 = u2 * u2 * u2; every other
 *      exponent is one __powf(x, e).  A NaN m counts as below every number in rules 6 and 8.
 *   6. The candidates of g are its min(topk, #inside) inside anchors of largest m, ties to the lower anchor index.  A box without an
 *      inside anchor has no candidate.
 *   7. An anchor that is a candidate of several boxes goes to the one with the largest u, then the lowest box index.
 *   8. Over the anchors g kept after rule 7: m_max = max m, u_max = max u, t(a) = m(a, g) / (m_max + 1e-9f) * u_max.
 * box_idx[a] = g for a kept anchor, its target row the box's columns 0..4 and score * t(a) in column 5; every other anchor:
 * SSDK_NOT_MATCHED and (0, 0, 0, 0, 0, 1).  No ignore band and no force stage.  Three launches, nothing [G, A]-shaped, no atomics, no
 * host synchronisation, the same bits run to run; the call may sit in a captured HIP graph.
 */
int ssdk_encode_ground_truth_tal(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                                 const float* anchors, int num_anchors, const float* scores, int num_columns, const float* locs,
                                 float xy_scale, float wh_scale, int topk, float alpha, float beta, float* target, int32_t* box_idx,
                                 void* workspace, size_t workspace_bytes, void* stream);

#define SSDK_SIMOTA_MAX_TOPK 32
size_t ssdk_encode_ground_truth_simota_workspace_bytes(int batch, int total_gt, int num_anchors, int n_levels);
/*
 * Target assignment by SimOTA (YOLOX, arXiv:2107.08430 section 2.4: OTA, arXiv:2103.14259, with the Sinkhorn iteration replaced by a dynamic
 * top-k; ABI 132; the reference has no such assigner).  The number of positives of a box comes from the prediction itself.  gt_rows,
 * gt_stride, gt_offsets, batch, total_gt, anchors, scores, num_columns, locs, xy_scale, wh_scale, target, box_idx as for
 * ssdk_encode_ground_truth_tal; level_sizes as for ssdk_encode_ground_truth_atss; beside them
 *   level_strides   HOST float [n_levels * 2]: (sx, sy) per level, image pixels per cell of that level's map, finite and > 0.  Read during
 *                   the call and handed to the kernels by value, so the call may sit in a captured HIP graph.  n_levels 1..SSDK_ATSS_MAX_LEVELS.
 *   center_radius   finite, > 0 (YOLOX: 2.5); candidate_topk (q) 1..SSDK_SIMOTA_MAX_TOPK (YOLOX: 10); iou_weight finite, >= 0 (YOLOX: 3)
 *   dynamic_k       DEV int32 [total_gt] or NULL: rule 5's k_g (0 in the padding rows past gt_offsets[batch])
 * For every box g = (x1, y1, x2, y2, class, score) of an image and every anchor a = (cx, cy, w, h) of level l, all arithmetic in fp32, one
 * operation at a time, nothing contracted:
 *   1. P_a and u(a, g) are rules 1 and 2 of ssdk_encode_ground_truth_tal, by the same device functions.
 *   2. Regions.  in_box: x1 < cx < x2 and y1 < cy < y2.  in_centre: with gcx = (x1 + x2) * 0.5f, gcy = (y1 + y2) * 0.5f,
 *      rx = center_radius * sx_l, ry = center_radius * sy_l:  gcx - rx < cx < gcx + rx and gcy - ry < cy < gcy + ry.  NaN is in neither.
 *      region = in_box || in_centre; penalised = !(in_box && in_centre).
 *   3. Class term.  YOLOX's binary cross-entropy of the sigmoid row against the box's one-hot row, summed over the columns, is
 *      S_a - x[a, k - 1] with S_a = sum_c softplus(x[a, c]), softplus(x) = fmaxf(x, 0) + __logf(1 + __expf(-|x|)), summed in fp32 in one
 *      fixed order and computed once per call: eight partial sums, partial l over the column quads 4j..4j+3 with j = l, l + 8, ... in
 *      ascending column order, then p[l] += p[l ^ 4], p[l] += p[l ^ 2], p[l] += p[l ^ 1].  k = (int)class.  A class outside
 *      1..num_columns (NaN included) has the all-zero row: cls = S_a.  (There is no objectness branch: the probability is the class
 *      sigmoid alone.)
 *   4. cost(a, g) = cls + iou_weight * (-__logf(u + 1e-8f)).  A NaN cost ranks above every number.
 *   5. n_g = the number of region anchors of g, q' = min(q, n_g); k_g = min(max((int)S, 1), q') with S the fp64 sum of the q' largest u
 *      over the region anchors, largest first; k_g = 0 when n_g = 0.
 *   6. The candidates of g are its k_g region anchors that are smallest by (penalised, cost, anchor index).  (The lexicographic order is
 *      YOLOX's cost + 1e5 * penalised wherever the unpenalised cost is below 1e5, without the rounding of adding 1e5 in fp32.)
 *   7. An anchor that is a candidate of several boxes goes to the smallest (penalised, cost), then the lowest box index.
 *   8. box_idx[a] = g and the target row is the box's six columns (column 5 is the box's score, as ATSS; QualityFocalLoss(use_iou=True)
 *      forms YOLOX's IoU-aware class target from it); every other anchor: SSDK_NOT_MATCHED and (0, 0, 0, 0, 0, 1).  No ignore band and no
 *      force stage.
 * One stated deviation from YOLOX / mmdet: a box ranks only anchors of its OWN region (YOLOX ranks the union of all boxes' regions, which
 * differs only for a box with fewer than k_g region anchors: it would then take 1e5-penalised anchors from other boxes' regions).
 * Three launches, nothing [G, A]- or [G, A, C]-shaped, no atomics, no host synchronisation, the same bits run to run.
 */
int ssdk_encode_ground_truth_simota(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                                    const float* anchors, int num_anchors, const int32_t* level_sizes, const float* level_strides, int n_levels,
                                    const float* scores, int num_columns, const float* locs, float xy_scale, float wh_scale,
                                    float center_radius, int candidate_topk, float iou_weight, float* target, int32_t* box_idx,
                                    int32_t* dynamic_k, void* workspace, size_t workspace_bytes, void* stream);

/* ---- sampler + loss (S1 + L1 + L2 + L3) ----------------------------------------------------------------------- */

size_t ssdk_multibox_loss_workspace_bytes(int batch, int num_anchors, int num_classes);

/*
 * detection/sampler.py:12-25 hard_negative_mining.  scores DEV [batch, A, C]; target_classes DEV fp32, the class
 * of anchor r at target_classes[r * class_stride] (class_stride = 6 and pointer = target + 4 reads the class column
 * of a [batch, A, 6] target in place; 1 = a dense [batch, A] array); sampled DEV uint8 [batch, A] (1 = positive or
 * selected hard negative).  Leaves the per-anchor log-sum-exp of the scores in the workspace for
 * ssdk_multibox_loss_fwd to reuse (lse_valid).
 */
int ssdk_hard_negative_mining(const float* scores, const float* target_classes, int class_stride, int batch,
                              int num_anchors, int num_classes, double negative_per_positive_ratio,
                              int64_t min_negative_per_image, uint8_t* sampled, void* workspace, size_t workspace_bytes,
                              void* stream);

/* detection/sampler.py:9-10 naive_sampler: positives only. */
int ssdk_naive_sampler(const float* target_classes, int class_stride, int batch, int num_anchors, uint8_t* sampled,
                       void* stream);
/* Its twin for losses that train the classifier on every anchor: sampled = (class != -1). */
int ssdk_valid_sampler(const float* target_classes, int class_stride, int batch, int num_anchors, uint8_t* sampled,
                       void* stream);

/*
 * Loss configuration of detection/losses/multibox_loss.py:11-33 (what the constructed loss objects carry).
 *   focal_alpha < 0 means None (SoftmaxFocalLoss only).  reduce_mean == 1: the focal losses divide by the number of
 *   sampled rows -- the reference's constructor drops reduction='sum' for classes whose __init__ takes **kwargs
 *   (bf/utils/misc_utils.py:22-29).  reduce_mean == 2: out3 holds the plain sums, NOT divided by
 *   max(1, #positives) -- a loss module of bf/modules/losses.py:34-106 on its own (forward(prediction, target) outside
 *   MultiboxLoss).  soft_epsilon: label smoothing of the soft-target losses.
 *   smooth_l1_beta: beta of SSDK_LOC_SMOOTH_L1 (>= 0; 0 is torch.nn.functional.smooth_l1_loss's L1 case, = SSDK_LOC_L1) and delta of
 *   SSDK_LOC_HUBER (> 0); unused by the other kinds.
 *   ce_label_smoothing, class_weight: torch.nn.CrossEntropyLoss(label_smoothing=, weight=) -- SSDK_CLS_CROSS_ENTROPY only (0 / NULL for
 *   every other kind).  Per sampled row i with label y (ignore_index -1 rows excluded), over the C classes with p = softmax(x_i):
 *   (1 - ce_label_smoothing) * w_y * (-log p_y) + ce_label_smoothing / C * sum_c w_c * (-log p_c), the reduction='sum' form of
 *   torch.nn.functional.cross_entropy.  ce_label_smoothing in [0, 1]; class_weight DEV float[C] or NULL (every w_c = 1), read by the
 *   forward and the backward (keep it alive and at the same address across both -- and across the replays of a captured graph).
 *   Both fields are appended: a positional initialisation of the older fields leaves them 0 / NULL, i.e. plain cross-entropy.
 *   quality_from_iou (appended likewise, 0 when left out): SSDK_CLS_QUALITY_FOCAL / _VARIFOCAL only -- non-zero computes the quality q
 *   from the predicted box (above), 0 takes q = 1 (the target value is given).  For these two kinds focal_gamma is beta (>= 1) resp.
 *   gamma (>= 0), focal_alpha is Varifocal's alpha in [0, 1], and reduce_mean means what it means for the focal kinds.
 */
typedef struct ssdk_loss_params {
    int cls_kind;  /* SSDK_CLS_* */
    int loc_kind;  /* SSDK_LOC_* */
    float focal_gamma;
    float focal_alpha;
    int reduce_mean;
    float soft_epsilon;
    float classification_weight;
    float localization_weight;
    float xy_scale, wh_scale, eps; /* BoxCoder */
    float smooth_l1_beta;     /* SmoothL1Loss beta, HuberLoss delta */
    float ce_label_smoothing; /* CrossEntropyLoss label_smoothing */
    const float* class_weight; /* CrossEntropyLoss weight, DEV [C] or NULL */
    int quality_from_iou;      /* SSDK_CLS_QUALITY_FOCAL / _VARIFOCAL: q = IoU(decoded prediction, raw target) instead of 1 */
} ssdk_loss_params;

/*
 * detection/losses/multibox_loss.py:35-94 MultiboxLoss.forward for a given sampled mask.
 *   classification: sum over the sampled rows of the loss selected by cls_kind (ignore_index = -1 for the hard-label
 *   kinds), localisation: loc_kind over the positives.
 *   target DEV [batch, A, 6]: with SSDK_LOC_SMOOTH_L1 it is MUTATED like the reference -- columns 0..3 become the
 *          encoded regression targets (to_centroids + encode_box in place, multibox_loss.py:81-82 / box_coder.py:22-30),
 *          every anchor (the same for SSDK_LOC_L1 / _MSE / _HUBER); with SSDK_LOC_GIOU, _IOU, _DIOU, _CIOU and _EIOU it is left alone
 *          (multibox_loss.py:77-79).
 *   out3   DEV float[3] = (loss, class_loss, loc_loss), each already divided by max(1, #positives).
 *   lse_valid != 0: the workspace already holds this batch's per-anchor log-sum-exp (left there by
 *          ssdk_hard_negative_mining on the same scores), so the scores are not read again for sampled negatives.
 *   sampled DEV uint8 [batch, A], or NULL = "every row whose class is not -1 is sampled" (what ssdk_valid_sampler writes, without
 *          the mask).  NULL is accepted for SSDK_CLS_SIGMOID_FOCAL, _QUALITY_FOCAL and _VARIFOCAL only (SSDK_E_INVALID otherwise); it
 *          runs the dense, element-parallel kernels, which _QUALITY_FOCAL and _VARIFOCAL use with a mask as well.
 * The workspace keeps what ssdk_multibox_loss_bwd needs (divider, scale, per-anchor log-sum-exp -- for SSDK_CLS_QUALITY_FOCAL /
 * _VARIFOCAL the per-anchor quality q instead, so that the backward sees the forward's q whatever the box kind did to the target);
 * pass the same one.
 */
int ssdk_multibox_loss_fwd(const ssdk_loss_params* params, const float* scores, const float* locs, const float* anchors,
                           float* target, const uint8_t* sampled, int batch, int num_anchors, int num_classes, int lse_valid,
                           float* out3, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Backward of ssdk_multibox_loss_fwd.  grad_out DEV float[2] = (dL/dclass_loss, dL/dloc_loss).
 * target is the target as the forward call left it.  dscores DEV [batch, A, C] and dlocs DEV [batch, A, 4] are
 * written in full (zeros off the sampled / positive rows).  sampled: the forward call's (NULL included).
 */
int ssdk_multibox_loss_bwd(const ssdk_loss_params* params, const float* scores, const float* locs, const float* anchors,
                           const float* target, const uint8_t* sampled, const float* grad_out, int batch, int num_anchors,
                           int num_classes, float* dscores, float* dlocs, void* workspace, size_t workspace_bytes,
                           void* stream);
/* ... which also writes row_mask DEV uint8 [batch][num_anchors] (NULL: not wanted): 1 where the anchor's dscores / dlocs rows can be
 * non-zero (it contributes a classification term, or it is a positive and contributes a box term), 0 where both rows were written as
 * zeros -- the guarantee ssdk_heads_bwd_ex takes.  grad_single != 0: grad_out is ONE device scalar, the upstream gradient of
 * loss = class_loss + loc_loss (out3[0] of the forward), applied to both terms; 0: grad_out[2] = (d class_loss, d loc_loss). */
int ssdk_multibox_loss_bwd_ex(const ssdk_loss_params* params, const float* scores, const float* locs, const float* anchors,
                              const float* target, const uint8_t* sampled, const float* grad_out, int grad_single, int batch, int num_anchors,
                              int num_classes, float* dscores, float* dlocs, uint8_t* row_mask, void* workspace, size_t workspace_bytes,
                              void* stream);

/* detection/box_coder.py:13-34 encode_box (inplace != 0: :22-30, eps after the divide; else :32-34). boxes [n_batch, A, 4]. */
int ssdk_encode_box(const float* boxes, const float* priors, float* out, int batch, int num_anchors, float xy_scale,
                    float wh_scale, float eps, int inplace_semantics, void* stream);
/* detection/box_coder.py:37-57 decode_box -> centroid boxes (inplace_semantics != 0: op order of :45-53, else :55-57). */
int ssdk_decode_box(const float* locs, const float* priors, float* out, int batch, int num_anchors, float xy_scale,
                    float wh_scale, int inplace_semantics, void* stream);

/* ---- postprocess (P1 + P2) ----------------------------------------------------------------------------------- */

size_t ssdk_postprocess_workspace_bytes(int batch, int num_anchors, int num_classes, int softmax, int max_per_class,
                                        int max_total);
/* ... for a call with this soft_nms: soft-NMS without max_per_class (or above 256) keeps a decaying score per candidate and up to
 * min(max_per_class, num_anchors) rows per class, which the size above (= soft_nms 0) does not hold. */
size_t ssdk_postprocess_workspace_bytes_ex(int batch, int num_anchors, int num_classes, int softmax, int max_per_class,
                                           int max_total, int soft_nms);

/*
 * detection/postprocessor.py:24-78 Postprocessor.postprocess with bf/utils/box_utils.py:166-194 (nms wrapper:
 * per-class top max_per_class, then hard NMS per torchvision.ops.nms's contract, or -- soft_nms != 0 -- the gaussian
 * soft-NMS of box_utils.py:145-163 with sigma = soft_sigma) fused.
 *   scores DEV [batch, A, C] logits; locs DEV [batch, A, 4]; priors DEV [A, 4]
 *   softmax != 0: F.softmax and drop column 0 (classes 1..C-1); else sigmoid (classes 1..C)
 *   max_per_class: 1..256, or <= 0 for None (every candidate of a class enters NMS, box_utils.py:186), or > 256 -- the last two take
 *   the greedy kernels (hard: post_nms_any_kernel, a class then yields at most max_total rows, more can never reach the final
 *   top-max_total; soft: post_softnms_any_kernel, workspace from ssdk_postprocess_workspace_bytes_ex) and at most 131 072 anchors;
 *   max_total <= 0 means None
 *   out    DEV [batch, out_cap, 6] rows (x1, y1, x2, y2, class, score); counts DEV int32 [batch];
 *          out_cap >= (max_total > 0 ? max_total : ncls * max_per_class)   (max_per_class None: ncls * num_anchors)
 *   nms_candidates DEV int64 [batch] or NULL: number of boxes that entered NMS per image
 */
int ssdk_postprocess(const float* scores, const float* locs, const float* priors, int batch, int num_anchors,
                     int num_classes, int softmax, float score_threshold, int max_per_class, float nms_threshold,
                     int soft_nms, float soft_sigma, int max_total, float xy_scale, float wh_scale, float* out, int out_cap,
                     int32_t* counts,
                     int64_t* nms_candidates, void* workspace, size_t workspace_bytes, void* stream);
/* TEST HOOK, host only (no device; ABI 129): the dispatch ssdk_postprocess would take for a call of this shape and these options, decided by
 * the functions the real entry point launches by and under the environment of the call (SSDK_POST_SAMPLE / _NO_SAMPLE, SSDK_POST_WGS,
 * SSDK_POST_NO_FOLD, SSDK_NMS_ONE_PASS, SSDK_POST_OLD).  sample: 1 / 0 = the plan with / without the sample pass where the shape allows
 * one (the real call chooses by a hint the previous call left), < 0 = what the next call of this process would choose.  Refuses what
 * ssdk_postprocess refuses on shape.  out[16]:
 *   [0] pipeline: 0 = post_select2_kernel + post_nms_wave_kernel (+ post_finish_kernel or post_merge2_kernel), 1 = greedy
 *       (max_per_class None or > 256: post_select_kernel + post_nms_any_kernel / post_softnms_any_kernel + post_merge_kernel),
 *       2 = general (post_select_kernel + post_nms_kernel + post_merge_kernel)
 *   [1] softmax  [4] 64-row tiles per image  [13] tie_up: the last mantissa bit of nms_threshold (pipeline 0 compares
 *       inter with the midpoint of the threshold and the next float times the union; a tie goes up when the bit is set)
 *   pipeline 0 only (0 otherwise): [2] pad, [3] JMAX of post_select2_kernel<SOFTMAX, PAD, JMAX>; [5] ns: sample tiles (0: no sample pass,
 *   no post_tau_kernel); [6] Gs, [7] Ts, [8] Gm, [9] Tm: workgroups per image and tiles per workgroup of the sample / main pass;
 *   [10] nseg; [11] list_cap: keys per (image, class) list; [12] khead: head size of the two-pass NMS (0: one pass,
 *   post_nms_wave_kernel<.., 0>); [14] 1: head + post_finish_kernel, 0 with khead > 0: head, post_img_tau_kernel, tail and merge as
 *   launches of their own; [15] reserved (0). */
int ssdk_debug_postprocess_plan(int batch, int num_anchors, int num_classes, int softmax, int max_per_class, float nms_threshold,
                                int soft_nms, int max_total, int sample, long long* out);

/* ---- multi-scale heads (H1) ----------------------------------------------------------------------------------- */

/*
 * One pyramid level of detection/detector.py:50-63: score = Conv2d(Cin, n_score, 3, padding=1, bias) and
 * loc = Conv2d(Cin, n_loc, 3, padding=1, bias) (detection/detector_builder.py:111-137), each followed by
 * permute(0,2,3,1).contiguous().view(B,-1), written straight into the concatenated outputs of detector.py:65-66.
 *   x        DEV [batch, H, W, Cin]  NHWC (= torch channels_last memory of the [B,Cin,H,W] source map)
 *   w_score  DEV [n_score, 3, 3, Cin] (= channels_last memory of the [n_score,Cin,3,3] parameter); b_score [n_score] or NULL
 *   w_loc    DEV [n_loc, 3, 3, Cin]; b_loc [n_loc] or NULL (n_loc may be 0)
 *   scores_offset / locs_offset: this level's first element inside one image's row of scores / locs
 *            (= C resp. 4 times the anchors of the preceding levels); element (image b, pixel p = y*W+x, channel n) lives at
 *            scores[b*scores_batch_stride + scores_offset + p*n_score + n], locs alike.
 *   backward outputs (ssdk_heads_bwd only; NULL = skip): dx DEV [batch,H,W,Cin]; dw_score/dw_loc like the weights
 *            (both or neither); db_score/db_loc.  All are overwritten, not accumulated.
 */
/* A level that is a SINGLE head (n_loc == 0: the score tower's or the loc tower's convolution of a SharedConvPredictor level, which run as
 * two calls because they read different maps) cannot tell the library how many anchor types a pixel has; its caller may pass that count
 * in locs_offset, which means nothing else for such a level (0 = unknown).  With it the sparse backward of ssdk_heads_bwd takes the
 * ordered anchor-row form (rows of n_score / types columns) in both modes; without it the level falls back to round 4's forms, dense in
 * deterministic mode. */
typedef struct ssdk_head_level {
    const float* x;
    int h, w, cin;
    const float* w_score;
    const float* b_score;
    int n_score;
    const float* w_loc;
    const float* b_loc;
    int n_loc;
    long long scores_offset;
    long long locs_offset;
    float* dx;
    float* dw_score;
    float* db_score;
    float* dw_loc;
    float* db_loc;
} ssdk_head_level;

/*
 * All levels of detector.py:50-66 in one grouped launch (n_levels <= 8): scores DEV [batch, scores_batch_stride],
 * locs DEV [batch, locs_batch_stride].  fp32 in, fp32 accumulate on the matrix cores (v_mfma_f32_32x32x2_f32).
 */
/* workspace DEV (optional, NULL = none): ssdk_heads_fwd_workspace_bytes() bytes, ZERO-FILLED ONCE by the caller before its first use and then
 * left to the library between calls (it holds parked partial tiles and their ready flags, told apart from call to call by a launch
 * counter).  With it, a launch of a few rounds of whole tiles runs in stream-K form: the K slices of the whole launch are cut into equal
 * ranges, one per resident workgroup, and a tile that straddles two ranges is summed through the workspace -- same results up to fp32
 * summation order of that one K split.  The last 256-byte-rounded part of the workspace is its flag region: 512 ready flags (back to 0
 * once their partial tile was consumed), the timeout counter, and the launch counter of the last stream-K launch that ran on it
 * (a launch that took another form leaves the region as it was).  That word is DIAGNOSTIC only -- tests and fault analysis read it; the
 * library never does, and no caller may build on it. */
/* The stream-K fix-up wait is bounded (a workgroup that never runs must not hang the GPU), and a wait that runs out is LOUD: the owner fills
 * its output tile with NaN instead of storing an incomplete sum, counts the event in the workspace, and sets a sticky word in pinned host
 * memory that makes this and every later ssdk_heads_fwd of the process return SSDK_E_STREAMK_TIMEOUT.  ssdk_heads_fwd_timeouts reads the
 * workspace's counter back (it SYNCHRONISES `stream`: a test / end-of-run check, not a hot-path call); *timeouts_host == 0 is the only
 * healthy value.  (Reference: none -- torch.nn.Conv2d has no such failure mode; detection/detector.py:50-63.) */
size_t ssdk_heads_fwd_workspace_bytes(void);
int ssdk_heads_fwd_timeouts(const void* workspace, size_t workspace_bytes, void* stream, unsigned* timeouts_host);
/* The sticky host word alone, without synchronising anything: 1 once any stream-K launch of this process has given up on a parked
 * partial tile.  For callers that replay captured HIP graphs (a replay does not pass through ssdk_heads_fwd's own check): test it before
 * every replay.  The kernel is loud on its own as well: from the first loss on, every launch on that workspace -- replayed or not --
 * stores NaN in every tile. */
int ssdk_streamk_poisoned(void);
/* TEST HOOK (fault injection, process-wide, synchronises the device): the stream-K workgroup with range index `drop_workgroup` never
 * raises its flag (-1: none), and an owner gives up after `spin_limit` polls (0: the default 2^22).  Used by
 * tests/streamk_fault_worker.py in a child process; never by the product path. */
int ssdk_debug_streamk_fault(int drop_workgroup, unsigned spin_limit);   /* refused (-3) unless SSDK_ENABLE_FAULT_INJECTION=1 is in the environment */
/* Recovery after SSDK_E_STREAMK_TIMEOUT (e.g. a trainer that goes back to a checkpoint inside the process): synchronises `stream`, clears
 * the flags and the timeout counter of this ssdk_heads_fwd / ssdk_conv2d_fwd_ws workspace and the process-wide sticky word, so that
 * ssdk_heads_fwd runs again and captured graphs replay healthy launches.  The outputs of the step that timed out are lost (NaN). */
int ssdk_streamk_reset(void* workspace, size_t workspace_bytes, void* stream);
/* TEST HOOK: byte offsets, inside the workspace of ssdk_heads_bwd / ssdk_heads_bwd_ex, of the intermediates the ordered anchor-row backward
 * keeps for level `level` (fp32 mode): out[0..7] = ga (rows [type][B*H*W][Jpad]), T (rows [row][9*Cin]), aidx (int [type][B*H*W]: T row or -1),
 * apix (int [type][B*H*W]: pixel of row r), acounts (int[16]: rows per type), plan (int[34]: first T row per type, then first 128-row
 * tile per type), mode (int: 2 = anchor rows, 0 = dense), T capacity in rows.  -3 when these levels do not take that pipeline. */
int ssdk_debug_heads_bwd_layout(const ssdk_head_level* levels, int n_levels, int batch, int level, unsigned long long* out);
int ssdk_heads_fwd(const ssdk_head_level* levels, int n_levels, int batch, float* scores, long long scores_batch_stride,
                   float* locs, long long locs_batch_stride, void* workspace, size_t workspace_bytes, void* stream);
/* The same with a cap on the persistent workgroups of the stream-K form (0 = the library's choice: 512 = every 64 KB LDS slot of the
 * chip; otherwise rounded down to a multiple of 8, at least 256): a caller that runs the levels taken from the backbone
 * (detection/detector.py:36-38) on one stream and the pyramid tail (detector.py:39-43) with its levels' heads on another leaves the
 * tail's kernels room beside this launch.  Several calls may fill disjoint level slices of the same scores / locs rows concurrently
 * on different streams, each with its own workspace. */
int ssdk_heads_fwd_ex(const ssdk_head_level* levels, int n_levels, int batch, float* scores, long long scores_batch_stride,
                      float* locs, long long locs_batch_stride, int max_workgroups, void* workspace, size_t workspace_bytes, void* stream);

/*
 * FAST MODE of ssdk_heads_fwd (opt-in, never the default): the role of apex AMP O1 in the reference (bf/training/env.py:87-95 runs these
 * convolutions in half precision; detection/postprocessor.py:39-40 casts back to fp32).  Every fp32 operand is split into bf16 pieces and
 * the product is the sum of its `terms` = 3 largest cross terms (a_hi b_hi + a_hi b_mid + a_mid b_hi) on v_mfma_f32_32x32x16_bf16 with
 * fp32 accumulation: a product is wrong by ~2^-16 relative instead of exact, logits by ~1e-5 of their scale.  Same arguments, layouts
 * and outputs as ssdk_heads_fwd; Cin % 32 == 0 on every level; workspace = ssdk_heads_fwd_fast_workspace_bytes() bytes (the split
 * weights of this call; nothing is kept between calls).  The backward pass stays ssdk_heads_bwd (fp32).
 */
size_t ssdk_heads_fwd_fast_workspace_bytes(const ssdk_head_level* levels, int n_levels);
int ssdk_heads_fwd_fast(const ssdk_head_level* levels, int n_levels, int batch, float* scores, long long scores_batch_stride, float* locs,
                        long long locs_batch_stride, int terms, void* workspace, size_t workspace_bytes, void* stream);

size_t ssdk_heads_bwd_workspace_bytes(const ssdk_head_level* levels, int n_levels, int batch);

/* FAST MODE of the backward pass (opt-in, like ssdk_heads_fwd_fast / ssdk_conv2d_fwd_fast; the reference's AMP covers forward AND
 * backward: bf/training/env.py:87-95, bf/training/callbacks.py:34-40): the DATA gradients that are dense stride-1 convolutions -- the
 * heads' dense form (every level of a focal-loss step), the 3 x 3 / 1 x 1 stride-1 layers of towers, necks and tails -- run as the forward
 * convolution of dy with the mirrored kernel on the split-bf16 GEMM (three cross terms on v_mfma_f32_32x32x16_bf16, fp32 accumulate);
 * the weights' two bf16 planes are split per call from the re-laid-out fp32 weights -- and the WEIGHT gradients (dense, pixel-row and
 * anchor-row forms alike) run on the split-bf16 form of the K-split GEMM, both operands split in registers after the LDS reads.
 * Everything else of ssdk_heads_bwd / ssdk_conv2d_bwd (the sparse and strided data gradients, bias gradients, the pack) is unchanged
 * fp32, as are the arguments; the
 * workspaces are larger (the planes): size them with the _fast_ functions.  A level / layer the kernel cannot take (channels not a
 * multiple of 32, operands beyond 2 GiB) silently stays on the fp32 kernel. */
size_t ssdk_heads_bwd_fast_workspace_bytes(const ssdk_head_level* levels, int n_levels, int batch);
int ssdk_heads_bwd_fast(const ssdk_head_level* levels, int n_levels, int batch, const float* dscores, long long scores_batch_stride,
                        const float* dlocs, long long locs_batch_stride, int terms, void* workspace, size_t workspace_bytes, void* stream);

/* ssdk_heads_bwd with what the producer of the gradient knows about its sparsity: row_mask DEV uint8 [batch][num_anchors] (NULL: nothing
 * known), 0 = the caller GUARANTEES that the score and loc gradient rows of that anchor (anchors numbered like the rows of scores / locs:
 * level after level, pixel-major, anchor type minor) are entirely zero -- ssdk_multibox_loss_bwd_ex writes exactly this mask for the
 * gradient it produces (hard-negative mining: ~4 % of the anchors).  The pack pass then reads only the pixels that have a marked anchor
 * instead of scanning all of dscores for non-zero rows (SSD-300 / 81 classes, batch 32: 88 MB).  fast_terms: 0 = fp32 (ssdk_heads_bwd),
 * 3 = the dense data gradients in fast mode (ssdk_heads_bwd_fast; size the workspace accordingly). */
int ssdk_heads_bwd_ex(const ssdk_head_level* levels, int n_levels, int batch, const float* dscores, long long scores_batch_stride,
                      const float* dlocs, long long locs_batch_stride, const unsigned char* row_mask, int num_anchors, int fast_terms,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Backward of ssdk_heads_fwd (what autograd derives for detector.py:50-66): dscores / dlocs are the gradients of the
 * concatenated outputs, addressed like scores / locs. */
int ssdk_heads_bwd(const ssdk_head_level* levels, int n_levels, int batch, const float* dscores,
                   long long scores_batch_stride, const float* dlocs, long long locs_batch_stride, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- pyramid tail (H2) and RetinaNet tower (H3): generic NHWC convolution + BatchNorm --------------------------- */

/*
 * torch.nn.Conv2d(cin, cout, ksize, stride, padding, bias) on NHWC buffers, as used by bf/modules/conv.py:4-36
 * (Conv2dBn of detection/detector_builder.py:57-109) and detection/modules/predictors.py:28-31,60-66.
 *   x [batch,hin,win,cin]; w [cout,ksize,ksize,cin] (channels_last memory of the OIHW parameter); bias [cout] or NULL;
 *   ksize 1 or 3, stride 1 or 2; relu != 0 fuses max(.,0) into the epilogue (the tower's conv -> ReLU);
 *   y [batch,hout,wout,cout].  Backward fields (ssdk_conv2d_bwd): dy like y (gradient w.r.t. the convolution output,
 *   i.e. with a fused ReLU already undone by ssdk_relu_bwd); dx like x, dw like w, db [cout]; NULL = skip.
 */
typedef struct ssdk_conv_desc {
    const float* x;
    int hin, win, cin;
    const float* w;
    const float* bias;
    int cout, ksize, stride, pad, relu;
    float* y;
    const float* dy;
    float* dx;
    float* dw;
    float* db;
    const float* w_t;   /* ssdk_conv2d_bwd: the weights as re-laid out by ssdk_conv2d_transpose_weights, or NULL (the call does it itself) */
    double* stats;      /* ssdk_conv2d_fwd: NULL, or a BatchNorm `sums` buffer [2 * cout + 2] (fp64) into which the per-channel sums of the
                           output and of its squares are ADDED (the values stored, i.e. after bias and ReLU), [2 * cout] = rows: the
                           statistics half of the BatchNorm that follows (bf/modules/conv.py:33-35), taken in the GEMM epilogue when the
                           convolution is not split over K, else by a pass over the output; cout % 4 == 0 */
    int dx_is_zero;     /* ssdk_conv2d_bwd: non-zero = dx already holds zeros (ssdk_batchnorm_bwd_chained_ex zero-filled it on this stream): when the
                           data gradient takes the atomic scatter form (ssdk_conv2d_dx_form == 1) the library skips its own zero-fill of dx and
                           adds into the buffer as it is; every other form overwrites dx and ignores the flag */
} ssdk_conv_desc;

/* n <= 8 convolutions (e.g. the five pyramid levels of one shared tower layer) in one grouped launch. */
int ssdk_conv2d_fwd(const ssdk_conv_desc* descs, int n, int batch, void* stream);
/* The same with the stream-K workspace of ssdk_heads_fwd (ssdk_heads_fwd_workspace_bytes() bytes, zero-filled once by the caller, shared with
 * ssdk_heads_fwd on the same stream; NULL = none): a launch of one or two rounds of whole tiles -- the large layers of a pyramid tail
 * (detection/detector_builder.py:73-82 at 18 x 18 / 9 x 9) -- then runs in stream-K form instead of splitting K with atomics into a
 * zero-filled output.  Same results up to fp32 summation order; a fix-up wait that runs out is loud (ssdk_heads_fwd_timeouts). */
int ssdk_conv2d_fwd_ws(const ssdk_conv_desc* descs, int n, int batch, void* workspace, size_t workspace_bytes, void* stream);

/* The same split-bf16 GEMM for a group of convolutions (ssdk_conv2d_fwd's descriptors: RetinaNet's towers, detection/modules/predictors.py:60-76,
 * and any tail / neck convolution with Cin % 32 == 0).  Bias, ReLU and outputs as ssdk_conv2d_fwd; descriptors that share a weight tensor
 * (a tower layer over five pyramid levels) share its split planes; ssdk_conv_desc::stats is honoured by a statistics pass after the launch. */
size_t ssdk_conv2d_fwd_fast_workspace_bytes(const ssdk_conv_desc* descs, int n);
int ssdk_conv2d_fwd_fast(const ssdk_conv_desc* descs, int n, int batch, int terms, void* workspace, size_t workspace_bytes, void* stream);
size_t ssdk_conv2d_bwd_workspace_bytes(const ssdk_conv_desc* descs, int n, int batch);
/* accumulate != 0: dw / db are added to what the buffers hold; else they are overwritten (descriptors that name the
 * same dw / db -- weights shared across levels -- are summed into it). */
int ssdk_conv2d_bwd(const ssdk_conv_desc* descs, int n, int batch, int accumulate, void* workspace, size_t workspace_bytes,
                    void* stream);
/* ... with the stream-K state of ssdk_heads_fwd / ssdk_conv2d_fwd_ws (ssdk_heads_fwd_workspace_bytes() bytes, zeroed once, kept between
 * calls): with SSDK_CONV_STREAMK_BWD=1 in the environment a stride-1 data-gradient launch of a few rounds of tiles whose last round is
 * partly filled (the RetinaNet towers) runs in stream-K form like the forward launch of the same layers (off by default: measured no
 * faster).  Same results up to fp32 summation order inside a tile cut in two. */
int ssdk_conv2d_bwd_sk(const ssdk_conv_desc* descs, int n, int batch, int accumulate, void* workspace, size_t workspace_bytes,
                       void* sk_workspace, size_t sk_workspace_bytes, void* stream);
/* ... with the stride-1 data gradients in fast mode (see ssdk_heads_bwd_fast above). */
size_t ssdk_conv2d_bwd_fast_workspace_bytes(const ssdk_conv_desc* descs, int n, int batch);
int ssdk_conv2d_bwd_fast(const ssdk_conv_desc* descs, int n, int batch, int accumulate, int terms, void* workspace, size_t workspace_bytes,
                         void* stream);
/* The weights of n <= 24 convolutions in the layout ssdk_conv2d_bwd's backward-data GEMM reads (stride 1: [cin][tap][cout], else
 * [tap][cin][cout]), outs[i] = cin * ksize^2 * cout floats, 16-byte aligned, ONE launch: called once per training step for all the
 * layers of a chain, the results passed as ssdk_conv_desc::w_t (the reference has no counterpart: cuDNN re-lays weights out inside
 * every backward call, bf/modules/conv.py:30-36 through torch.nn.Conv2d). */
int ssdk_conv2d_transpose_weights(const ssdk_conv_desc* descs, int n, float* const* outs, void* stream);
/* TEST HOOK, host only (no device, no pointer is dereferenced: the descriptors' pointers are looked at for NULL and 16-byte alignment):
 * the GEMM launches that ssdk_conv2d_fwd_ws (direction 0) or the data-gradient part of ssdk_conv2d_bwd / _bwd_sk (direction 1; descriptors
 * without dx make none) would make for these descriptors, decided by the code, the environment and the deterministic flag the real call
 * uses.  have_workspace: a stream-K workspace would be passed.  One entry per launch (direction 1: stride-1, strided scatter, strided
 * ordered -- at most 3): kernel = the instantiation ("dma generic one-tile", "staged<4> mirror", "streamk", "... + strided_dx" when the
 * sum pass follows); per problem, in the order of the launch's descriptors (desc[i] = index in descs): column blocks, K splits, half-width
 * last tile, first workgroup and workgroup count in the grouped grid. */
typedef struct ssdk_conv_plan_launch {
    char kernel[48];
    int grid, count;
    int desc[8], n_blocks[8], k_splits[8], half_last[8], block_begin[8], blocks[8];
} ssdk_conv_plan_launch;
int ssdk_debug_conv2d_plan(const ssdk_conv_desc* descs, int n, int batch, int direction, int have_workspace, ssdk_conv_plan_launch* out,
                           int max_launches, int* n_launches);
/* Host only: the form the data gradient of `desc` takes in ssdk_conv2d_bwd under the process' deterministic flag and environment, the
 * plan's own decision: 0 = stride-1 GEMM (dx overwritten, or zero-filled by the library when it splits K), 1 = strided atomic scatter (dx
 * zero-filled, then added into), 2 = strided ordered rows + sum pass (dx overwritten).  Only stride is read. */
int ssdk_conv2d_dx_form(const ssdk_conv_desc* desc);
/* TEST HOOK, host only: out[0] = zero-fill launches (zero_many_kernel) this process has made in the convolution entry points, out[1] = the
 * floats they covered. */
int ssdk_debug_zero_fill_counts(unsigned long long* out);
/* dx = y > 0 ? dy : 0 (n floats, n % 4 == 0). */
int ssdk_relu_bwd(const float* y, const float* dy, long long n, float* dx, void* stream);

size_t ssdk_batchnorm_workspace_bytes(int channels); /* = the [2 * channels + 2] doubles of a `sums` buffer (below), 256-byte rounded */
/* Every entry point of the BatchNorm family moves float4s: channels % 4 == 0 and 16-byte aligned x / y / dy / dx, SSDK_E_UNSUPPORTED
 * otherwise.  The composed entry points (_fwd, _bwd, _fwd_chained, _bwd_chained) check all of it before their first launch: a call that
 * is refused has written nothing. */
/*
 * torch.nn.BatchNorm2d forward on [rows = batch*H*W][channels] (NHWC), optional fused ReLU after it (conv.py:33-35).
 * training != 0: batch statistics (biased variance), running_mean / running_var updated with `momentum` (unbiased
 * variance) when non-NULL; else running statistics.  save_mean / save_rstd [channels] are kept for the backward.
 * num_batches_tracked DEV int64 [1] or NULL: the module's counter, incremented by one in training mode
 * (torch.nn.modules.batchnorm._BatchNorm.forward does `self.num_batches_tracked.add_(1)` -- a launch of its own per layer).
 */
int ssdk_batchnorm_fwd(const float* x, long long rows, int channels, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                       int training, int relu, float* y, float* save_mean, float* save_rstd, void* workspace,
                       size_t workspace_bytes, void* stream);
/* y is the forward output (needed only when relu bit 0 is set, for the mask).  Backward entry points read `relu` as two bits: bit 0 = the
 * norm's own fused ReLU; bit 1 = the norm's INPUT x is the output of a ReLU (conv -> ReLU -> BatchNorm, detection/modules/predictors.py:60-76)
 * whose gradient is taken in the same pass: dx = 0 where x <= 0, and the producer skips its own ReLU-gradient pass. */
int ssdk_batchnorm_bwd(const float* x, const float* y, const float* dy, long long rows, int channels, const float* gamma,
                       const float* save_mean, const float* save_rstd, int relu, int training, float* dx, float* dgamma,
                       float* dbeta, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Synchronised BatchNorm (the reference converts every BatchNorm with apex `convert_syncbn_model`, detection/init.py:85, in
 * --distributed mode): ssdk_batchnorm_fwd / _bwd cut in two, with the caller's all-reduce(sum) over the ranks in between.
*   sums DEV double [2 * channels + 2]: forward  = (sum x, sum x^2, rows, 0); backward = (sum dy', sum dy' * xhat, rows, 0), dy' = dy masked
 *   by the fused ReLU (the last double is padding: buffers are zero-filled in 16-byte units).  One all-reduce(sum) of the whole buffer -- or of several layers' buffers laid back to back, e.g. the five
 *   per-level norms of one RetinaNet tower layer -- makes them the statistics of the global batch.
 *   ssdk_batchnorm_apply: training-mode forward from such sums (count_in_sums != 0: the row count is sums[2 * channels], else `rows`);
 *     running statistics, num_batches_tracked, save_mean / save_rstd as ssdk_batchnorm_fwd.
 *   ssdk_batchnorm_bwd_apply: dx from `sums` (global; total_rows = sums + 2 * channels or NULL for `rows`), dgamma / dbeta from
 *     `sums_local` (this rank's own sums, NULL = sums): parameter gradients stay per-rank sums, the gradient exchange averages them
 *     like every other parameter's (torch.nn.SyncBatchNorm does the same).
 * With one rank the two halves are exactly ssdk_batchnorm_fwd / ssdk_batchnorm_bwd (which are implemented as their composition).
 */
int ssdk_batchnorm_stats(const float* x, long long rows, int channels, double* sums, void* stream);
int ssdk_batchnorm_apply(const float* x, long long rows, int channels, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, int64_t* num_batches_tracked, float momentum, float eps, int relu, float* y,
                         float* save_mean, float* save_rstd, const double* sums, int count_in_sums, void* stream);
int ssdk_batchnorm_bwd_stats(const float* x, const float* y, const float* dy, long long rows, int channels, const float* save_mean,
                             const float* save_rstd, int relu, double* sums, void* stream);
int ssdk_batchnorm_bwd_apply(const float* x, const float* y, const float* dy, long long rows, int channels, const float* gamma,
                             const float* save_mean, const float* save_rstd, int relu, int training, const double* sums,
                             const double* sums_local, const double* total_rows, float* dx, float* dgamma, float* dbeta, void* stream);

/*
 * Chained form for a layer that keeps two `sums` buffers of its own (forward, backward), so that no zero-fill launch runs in front of
 * the statistics: `sums` must hold zeros on entry; `zero_after` (NULL = none; a buffer of the same size that nothing else touches during
 * the call) is zero-filled by the apply launch -- the forward call zeroes the layer's backward buffer, the backward call its forward
 * buffer.  Training mode, statistics of this process's rows; otherwise exactly ssdk_batchnorm_fwd / ssdk_batchnorm_bwd.
 */
int ssdk_batchnorm_fwd_chained(const float* x, long long rows, int channels, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, int64_t* num_batches_tracked, float momentum, float eps, int relu, float* y,
                               float* save_mean, float* save_rstd, double* sums, double* zero_after, void* stream);
int ssdk_batchnorm_bwd_chained(const float* x, const float* y, const float* dy, long long rows, int channels, const float* gamma,
                               const float* save_mean, const float* save_rstd, int relu, float* dx, float* dgamma, float* dbeta,
                               double* sums, double* zero_after, void* stream);
/* TEST HOOK, host only (no device): the grid of the statistics launches behind ssdk_batchnorm_stats / _stats_accumulate / _bwd_stats and the
 * composed entry points for a [rows][channels] map, decided by the code and the environment (SSDK_BN_ROWS, SSDK_BN_WGS, SSDK_BN_SLAB) the real
 * call uses.  out[4] = rows per workgroup, row blocks, slab width in float4 columns (a power of two <= 64), slabs.  The launch has
 * row blocks x slabs workgroups, slabs innermost: workgroup g takes rows [g / slabs * rows_per_workgroup, ...) and the float4 columns
 * [s * slab, (s + 1) * slab), s = g % slabs, then s + slabs, ... while they exist (slabs == 1: whole rows).  Exactly `row blocks` workgroups
 * add to any one address of `sums`. */
int ssdk_debug_batchnorm_plan(long long rows, int channels, long long* out);
/* ssdk_batchnorm_bwd_chained whose apply launch also zero-fills zero_also[0 .. zero_also_floats) -- any float count, 4-byte aligned start, a
 * buffer nothing else touches during the call; the stores are spread over the launch's workgroups.  NULL or 0: exactly
 * ssdk_batchnorm_bwd_chained.  Meant for the dx of the producing strided convolution (ssdk_conv_desc::dx_is_zero). */
int ssdk_batchnorm_bwd_chained_ex(const float* x, const float* y, const float* dy, long long rows, int channels, const float* gamma,
                                  const float* save_mean, const float* save_rstd, int relu, float* dx, float* dgamma, float* dbeta,
                                  double* sums, double* zero_after, float* zero_also, long long zero_also_floats, void* stream);
/* The statistics half alone, ADDING into `sums` (no zero-fill; sums[2 * channels] = rows), and the apply half of the chained form for sums
 * that are already complete -- accumulated by the producing convolution's epilogue (ssdk_conv_desc::stats): conv -> BatchNorm then costs one
 * launch for the norm instead of two, and the statistics pass over the activation is gone (bf/modules/conv.py:30-36). */
int ssdk_batchnorm_stats_accumulate(const float* x, long long rows, int channels, double* sums, void* stream);
int ssdk_batchnorm_apply_chained(const float* x, long long rows, int channels, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, int64_t* num_batches_tracked, float momentum, float eps, int relu, float* y,
                                 float* save_mean, float* save_rstd, const double* sums, double* zero_after, void* stream);

/* ---- FPN top-down step (next-row f1) -------------------------------------------------------------------------------- */

/* bf/modules/features.py:106-107: out = fine + F.interpolate(coarse, size=(hf, wf), mode='nearest'); NHWC, channels % 4 == 0.
 * fine == NULL: plain nearest upsampling (features.py:371, M2Det base features). */
int ssdk_upsample_nearest_add_fwd(const float* fine, const float* coarse, int batch, int hf, int wf, int hc, int wc,
                                  int channels, float* out, void* stream);
/* gradient w.r.t. coarse: each coarse pixel sums dout over the fine pixels it was copied to (the gradient w.r.t. fine is dout). */
int ssdk_upsample_nearest_add_bwd(const float* dout, int batch, int hf, int wf, int hc, int wc, int channels,
                                  float* dcoarse, void* stream);
/* bf/modules/features.py:107-108, :264-265 with interpolation_mode='bilinear': out = fine + F.interpolate(coarse, size=(hf, wf),
 * mode='bilinear') (align_corners=False, no antialiasing); fine == NULL: plain bilinear resizing (features.py:371-373, M2Det base
 * features).  Per axis src = max(in / out * (dst + 0.5) - 0.5, 0), i0 = min((int)src, in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0,
 * l0 = 1 - l1; out = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).  Any pair of sizes (up, equal = identity, down, 1). */
int ssdk_upsample_bilinear_add_fwd(const float* fine, const float* coarse, int batch, int hf, int wf, int hc, int wc,
                                   int channels, float* out, void* stream);
/* gradient w.r.t. coarse (torch's upsample_bilinear2d_backward; the gradient w.r.t. fine is dout): each coarse pixel gathers weight * dout
 * over the fine pixels that read it, with the forward's own weights, rows and columns in ascending order -- no atomics, no zero-fill,
 * every element of dcoarse written: deterministic in both modes. */
int ssdk_upsample_bilinear_add_bwd(const float* dout, int batch, int hf, int wf, int hc, int wc, int channels,
                                   float* dcoarse, void* stream);

/* ---- M2Det scale-wise feature aggregation (next-row f1), bf/modules/features.py:273-300 ----------------------------- */

/* F.adaptive_avg_pool2d(x, 1): x [batch, hw, channels] (NHWC) -> out [batch, channels]; and its backward. */
int ssdk_global_avgpool_fwd(const float* x, int batch, int hw, int channels, float* out, void* stream);
int ssdk_global_avgpool_bwd(const float* dout, int batch, int hw, int channels, float* dx, void* stream);
/* out = x * sigmoid(z), z [batch, channels] broadcast over the pixels (features.py:296-298); backward gives dx and dz. */
int ssdk_sigmoid_gate_fwd(const float* x, const float* z, int batch, int hw, int channels, float* out, void* stream);
int ssdk_sigmoid_gate_bwd(const float* x, const float* z, const float* dout, int batch, int hw, int channels, float* dx,
                          float* dz, void* stream);

/* The same gate over PIECES (round 4): the maps the reference concatenates in front of the gate (features.py:385, torch.cat of the eight
 * TUM outputs of a scale, each [batch, hw, piece_channels]) are read where they are -- the concatenated map is never built.
 * `pieces`: n_pieces (<= 8) device pointers, 16-byte aligned, all of the same shape; columns k * piece_channels .. of pooled / z / out / dout /
 * dpool belong to piece k.
 *   pool_fwd:         pooled [batch, n * pc] = mean over the pixels                                  (features.py:288)
 *   gate_fwd:         out [batch, hw, n * pc] = piece * sigmoid(z)                                   (:296-298)
 *   gate_bwd_reduce:  dz [batch, n * pc] = sigmoid'(z) * sum_hw dout * piece                         (first half of the backward: feeds fc2 / fc1)
 *   gate_bwd_apply:   dpieces[k] [batch, hw, pc] = dout[.., k * pc ..] * sigmoid(z) + dpool / hw     (second half: the gate's and the pool's
 *                     gradient of a piece in one pass, each piece's gradient a contiguous map) */
int ssdk_sfam_pool_fwd(const float* const* pieces, int n_pieces, int batch, int hw, int piece_channels, float* pooled, void* stream);
int ssdk_sfam_gate_fwd(const float* const* pieces, int n_pieces, int batch, int hw, int piece_channels, const float* z, float* out,
                       void* stream);
int ssdk_sfam_gate_bwd_reduce(const float* const* pieces, int n_pieces, int batch, int hw, int piece_channels, const float* z,
                              const float* dout, float* dz, void* stream);
int ssdk_sfam_gate_bwd_apply(float* const* dpieces, int n_pieces, int batch, int hw, int piece_channels, const float* z, const float* dout,
                             const float* dpool, void* stream);

/* ---- depthwise convolution (bf/modules/conv.py:39-85 DepthwiseConv2dBn: depthwise k x k, groups = channels, then a 1x1 pointwise
 * convolution; `use_depthwise` configs such as samples/ssd_mb2_voc.py).  NHWC activations, weights [channels][k*k] (= the memory of
 * torch's [C,1,k,k] parameter), optional bias.  HBM-bound stencil; the pointwise half is ssdk_conv2d_*.
 *   fwd: y[b,yo,xo,c] = bias[c] + sum_tap w[c][tap] * x[b, yo*stride - pad + ky, xo*stride - pad + kx, c]
 *   bwd: dx (may be NULL), dw [channels][k*k] and db (may be NULL) are OVERWRITTEN (accumulate == 0) or added to. */
int ssdk_depthwise_conv2d_fwd(const float* x, const float* w, const float* bias, int batch, int hin, int win, int channels, int ksize,
                              int stride, int pad, float* y, void* stream);
int ssdk_depthwise_conv2d_bwd(const float* x, const float* w, const float* dy, int batch, int hin, int win, int channels, int ksize,
                              int stride, int pad, float* dx, float* dw, float* db, int accumulate, void* stream);

/* The forward of a depthwise Conv2dBn block -- depthwise k x k convolution -> BatchNorm2d -> ReLU (bf/modules/conv.py:30-36 with
 * groups = channels), the `pyramid_output` blocks that FeaturePyramid(use_depthwise=True) builds (bf/modules/features.py:79-98: stride 1 /
 * padding 1 on the tapped levels, stride 2 / padding 1 on the extra ones).  Arguments as ssdk_depthwise_conv2d_fwd's and checked by its
 * rules (channels % 4 == 0, ksize <= 5, 16-byte aligned maps and bias); y and sums / the running statistics must not be NULL.  A refusal
 * is SSDK_E_INVALID before any launch: nothing is written and ssdk_last_error_string() names the entry.  The backward is
 * ssdk_depthwise_conv2d_bwd behind the norm's.
 *   stats_fwd (training): y is ssdk_depthwise_conv2d_fwd's bit for bit, and the SAME launch adds the BatchNorm statistics of y to `sums`
 *        [2 * channels + 2] doubles -- sum y into sums[0 .. C), sum y^2 into sums[C .. 2C), accumulated in fp64 from the first add -- and stores
 *        sums[2C] = batch * hout * wout.  Like ssdk_batchnorm_stats_accumulate it ADDS to what is there (no zero-fill); the norm is then
 *        ssdk_batchnorm_apply_chained alone.  One fp64 atomic per channel, sum and workgroup; at most ~256 workgroups add to one address.
 *   norm_fwd (evaluation): ONE launch with the evaluation-mode norm (+ ReLU when relu != 0) in the stencil's epilogue; y is bit for bit
 *        ssdk_depthwise_conv2d_fwd followed by ssdk_batchnorm_fwd(training = 0).  gamma / beta may be NULL (1 / 0); 16-byte aligned. */
int ssdk_depthwise_conv2d_stats_fwd(const float* x, const float* w, const float* bias, int batch, int hin, int win, int channels, int ksize,
                                    int stride, int pad, float* y, double* sums, void* stream);
int ssdk_depthwise_conv2d_norm_fwd(const float* x, const float* w, const float* bias, int batch, int hin, int win, int channels, int ksize,
                                   int stride, int pad, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, int relu, float* y, void* stream);

/* The same stencil over 1 <= n_levels <= 8 maps that share batch, channels (% 4), weight [channels][k*k] and bias but have their own
 * hs[l] x ws[l]: the RetinaNet-lite tower of SharedConvPredictor(use_depthwise=True) (detection/modules/predictors.py:33-35,67-68), whose
 * DepthwiseConv2dBn (bf/modules/conv.py:72-76) is shared by the pyramid levels.  xs / ys / dys / dxs are HOST arrays of n_levels device
 * pointers (16-byte aligned NHWC fp32 maps); they are packed into the kernel argument, so there is no device-side table, no allocation
 * and no synchronisation (safe inside a captured graph).  Every level is checked by the rules of ssdk_depthwise_conv2d_* before any
 * launch; a refusal (< 0) names the function and the level.
 *   fwd: one launch; every level's y equals ssdk_depthwise_conv2d_fwd's bit for bit (the same tap order and fmaf chain).
 *   bwd: dx (one launch over the levels with a non-NULL dxs entry; dxs itself may be NULL) equals ssdk_depthwise_conv2d_bwd's bit for
 *        bit.  dw [channels][k*k] and db (either may be NULL) are OVERWRITTEN by two launches without atomics or zero-fill: the
 *        concatenated output pixels of all levels (level after level, each in b, y, x order; P of them) are cut into
 *        chunks = ceil(P / ppb) runs of ppb = ceil(P / clamp(P / 256, 1, 512)) pixels, a workgroup stores one partial per
 *        (chunk, tap, channel) -- row k*k is the bias column -- into `workspace`, and the second launch adds the chunks in ascending
 *        order.  The split depends on the shapes only, never on ssdk_set_deterministic: both modes give the same bits.
 *   workspace: ssdk_..._group_workspace_bytes() = chunks * (k*k + 1) * channels * 4 bytes (16-byte aligned; < 0 on bad arguments);
 *        a smaller workspace_bytes is refused.  Not needed (may be NULL) when dw and db are both NULL. */
long long ssdk_depthwise_conv2d_group_workspace_bytes(const int* hs, const int* ws, int n_levels, int batch, int channels, int ksize,
                                                      int stride, int pad);
int ssdk_depthwise_conv2d_group_fwd(const float* const* xs, const int* hs, const int* ws, int n_levels, const float* w, const float* bias,
                                    int batch, int channels, int ksize, int stride, int pad, float* const* ys, void* stream);
int ssdk_depthwise_conv2d_group_bwd(const float* const* xs, const int* hs, const int* ws, int n_levels, const float* w,
                                    const float* const* dys, int batch, int channels, int ksize, int stride, int pad,
                                    float* const* dxs /* NULL, or NULL entries: no data gradient */, float* dw, float* db /* may be NULL */,
                                    void* workspace, long long workspace_bytes, void* stream);

/* ---- depthwise feature pyramid (Tiny-DSOD D-FPN, bf/modules/features.py:123-212) ------------------------------------------------
 * NHWC fp32, channels % 4 == 0, 16-byte aligned maps.  Arguments are checked on the host before any launch (negative status).
 *
 * features.py:188-195  down[0](F.pad(f, [0, pad_right, 0, pad_bottom])) starts with nn.MaxPool2d(2): the 2 x 2 / stride 2 max-pool of the
 * map padded with pad_bottom (0 or 1) zero rows and pad_right zero columns; y [batch, (h + pad_bottom) / 2, (w + pad_right) / 2, channels].
 * The pad is a real 0.0 that takes part in the max.  torch's CPU rule: window order (0,0), (0,1), (1,0), (1,1), the first maximum wins a
 * tie, NaN wins.  A map without a single window (h + pad_bottom < 2 or w + pad_right < 2) is refused.
 * bwd: dx [batch, h, w, channels] is OVERWRITTEN -- dy at each window's maximum (recomputed from x), 0 elsewhere and where the maximum is
 * in the pad (F.pad drops that gradient).  Gather form: no atomics, deterministic. */
int ssdk_maxpool2x2_fwd(const float* x, int batch, int h, int w, int channels, int pad_bottom, int pad_right, float* y, void* stream);
int ssdk_maxpool2x2_bwd(const float* x, const float* dy, int batch, int h, int w, int channels, int pad_bottom, int pad_right, float* dx,
                        void* stream);
/* features.py:198  torch.cat(pieces, dim=1): n_pieces (1..8, host array of device pointers) maps of `rows` pixels with piece_channels[k]
 * (host array, each % 4 == 0) channels -> out [rows, sum of the channels]; bwd: the split, each dpieces[k] written as its own map. */
int ssdk_concat_channels_fwd(const float* const* pieces, const int* piece_channels, int n_pieces, long long rows, float* out, void* stream);
int ssdk_concat_channels_bwd(const float* dout, const int* piece_channels, int n_pieces, long long rows, float* const* dpieces, void* stream);
/* features.py:203-205  up_conv[i](F.interpolate(coarse, size=(hf, wf), mode='nearest')), the convolution half of Conv2dBn(C, C, 3,
 * padding=1, groups=C): a 3 x 3 depthwise convolution, pad 1, stride 1, of the nearest-upsampled map, reading `coarse` [batch, hc, wc,
 * channels] through torch's index map (that of ssdk_upsample_nearest_add) -- the upsampled map is never built.  w [channels][9], optional
 * bias; y [batch, hf, wf, channels].
 * bwd: dcoarse (may be NULL) is the gather over the fine pixels of each coarse pixel (no atomics); dw [channels][9] and db (may be NULL)
 * are OVERWRITTEN, reduced as ssdk_depthwise_conv2d_bwd's (in a fixed order in deterministic mode). */
int ssdk_depthwise_upsample_conv2d_fwd(const float* coarse, const float* w, const float* bias, int batch, int hc, int wc, int hf, int wf,
                                       int channels, float* y, void* stream);
int ssdk_depthwise_upsample_conv2d_bwd(const float* coarse, const float* w, const float* dy, int batch, int hc, int wc, int hf, int wf,
                                       int channels, float* dcoarse, float* dw, float* db, void* stream);

/* ---- device-resident input side ---------------------------------------------------------------------
 * bf/core/batch_container.py:25-45  BatchContainer.mixup_ with the random draws (lam ~ Beta(alpha, alpha), index = randperm(B),
 * roll = rand(B) < p) made by the caller exactly as the reference makes them on the host.
 *   images: out[i] = roll[i] ? lam * in[i] + (1 - lam) * in[index[i]] : in[i]   (out-of-place; fp32, two roundings like the
 *   reference's separate multiply and add; lam and 1 - lam are rounded to fp32 first, as torch does for a python scalar).
 *   ground truth (packed rows [total, gt_stride] + int32 offsets [B + 1], as for ssdk_encode_ground_truth): image i keeps its
 *   rows with score (column 5) * lam followed by the rows of image index[i] with score * (1 - lam) when roll[i], unchanged
 *   otherwise (:33-43).  rows_out must hold 2 * total rows; offsets_out [B + 1] is written on the device. */
int ssdk_mixup_images(const float* in, float* out, int batch, long long per_image, const int* index, const unsigned char* roll,
                      double lam, void* stream);
int ssdk_mixup_ground_truth(const float* rows_in, int gt_stride, const int* offsets_in, int batch, const int* index,
                            const unsigned char* roll, double lam, float* rows_out, int* offsets_out, void* stream);

/* ---- device-side SSD augmentation (ABI 133) ------------------------------------------------------------
 * bf/preprocessing/transforms.py in its one supported order: RandomAdjustHueSaturation, ToFloat, RandomAdjustBrightness,
 * RandomAdjustContrast, RandomExpand, RandomCrop, RandomHorizontalFlip / RandomVerticalFlip, Resize, ToFloatTensor, Normalize, every
 * step optional but the resize.  The random draws are the caller's: one ssdk_augment_params per image plus a table of candidate crop
 * windows.  The source images lie in ONE ragged uint8 buffer, interleaved RGB rows (HWC), each found by its ssdk_augment_image.
 *
 * Geometry.  The expand puts the image at (expand_x, expand_y) of a canvas expand_w x expand_h filled with the image's scalar mean;
 * the crop takes a window of that canvas; the flips mirror the window; the resize maps it onto out_w x out_h, bilinear with half-pixel
 * centres, src = (dst + 0.5) * (win / out) - 0.5, taps clamped to the WINDOW, no antialiasing.  The composition is one window in source
 * coordinates (windows[b] = x, y, w, h; x and y may be negative, the window may reach past the source on every side): a tap inside the
 * source reads its three bytes and applies the colour steps, a tap outside is the fill.
 *
 * Colour, on a source pixel (r, g, b), fp32:
 *   SSDK_AUG_HUE_SATURATION  float HSV: v = max, c = max - min, s = c / v (0 at v = 0), h in sextants; h += hue_delta * 6 (that is
 *                            hue_delta * 360 degrees, modulo 360), s = clip(s * saturation, 0, 1); back to RGB
 *                            channel(n) = v - v s max(0, min(k, 4 - k, 1)), k = (n + h) mod 6, n = 5, 3, 1 for r, g, b.
 *                            (The reference goes through cv2's 8-bit HSV; this is not bit-compatible with it, by design.)
 *   SSDK_AUG_BRIGHTNESS      x = clip(x + brightness, 0, 255)            (brightness = u * 255, already multiplied)
 *   SSDK_AUG_CONTRAST        x = clip(mean_c + contrast * (x - mean_c), 0, 255), mean_c the per-channel mean of the image after the steps above
 *   fill                     the mean over all channels of the image after the contrast step
 * Both means are fp64 sums over a fixed partition in a fixed order (no floating-point atomics: the same bits run to run), the quotient
 * taken in fp64 and rounded to float once. */
#define SSDK_AUG_HUE_SATURATION 1
#define SSDK_AUG_BRIGHTNESS 2
#define SSDK_AUG_CONTRAST 4
#define SSDK_AUG_EXPAND 8
#define SSDK_AUG_CROP 16      /* try the candidates; without it the window is the whole canvas and attempt_out is -2 */
#define SSDK_AUG_HFLIP 32
#define SSDK_AUG_VFLIP 64
#define SSDK_AUG_KEEP_IOU 128 /* keep_criterion 'iou'; without it 'center_point' */

typedef struct ssdk_augment_image {
    long long offset; /* of the image's first byte in the source buffer */
    int height, width;
} ssdk_augment_image;

typedef struct ssdk_augment_params {
    int flags; /* SSDK_AUG_* */
    float hue_delta, saturation, brightness, contrast;
    int expand_w, expand_h, expand_x, expand_y; /* canvas size and the image's origin in it (SSDK_AUG_EXPAND) */
    float min_iou;
    int min_objects_kept;
    int reserved;
} ssdk_augment_params;

/*
 * Stage 1: window choice and boxes (functional/box.py, functional/img.py:55-83, detection_dataset.py:31-32), float32 op for op.
 *   images, params   DEV [batch]
 *   candidates       DEV int32 [batch, attempts, 4]: (xmin, ymin, w, h) in the canvas; w <= 0 marks a candidate the host found larger than
 *                    the image (img.py:69-70).  A candidate that does not lie inside the canvas is skipped as well.
 *   rows_in          DEV fp32 [total_rows, gt_stride] + offsets_in DEV int32 [batch + 1], as for ssdk_encode_ground_truth; gt_stride >= 4
 *   rows_out         DEV fp32 [total_rows, gt_stride]: the surviving rows back to back, image after image, in input order; columns 4 and up
 *                    unchanged; rows past offsets_out[batch] are not written.  offsets_out DEV int32 [batch + 1].
 *   attempt_out      DEV int32 [batch]: index of the accepted candidate, -1 if none was (the image stays uncropped), -2 without SSDK_AUG_CROP
 *   windows_out      DEV int32 [batch, 4]: the window in source coordinates, for ssdk_augment_images
 * With region = [xmin, ymin, xmin + w - 1, ymin + h - 1]: a box's new corners are its zero_incorrect intersection with the region; iou is
 * that of the box with its own clipped version; the candidate is accepted when max(iou) > min_iou (strictly; a NaN iou rejects every
 * candidate) and at least min_objects_kept boxes stay -- those whose centre lies strictly inside the region, or whose own iou > min_iou with
 * SSDK_AUG_KEEP_IOU.  An image without boxes accepts its first valid candidate.  Accepted boxes are shifted by the window's origin and
 * clipped to [0, w - 1] x [0, h - 1]; a flip is (width - 1 - x) with the corners swapped; the resize multiplies by float(out_w / width)
 * and clips to [0, out_w - 1]; boxes with x1 == x2 or y1 == y2 are then dropped.
 * Two launches, no allocation, no synchronisation.
 */
size_t ssdk_augment_boxes_workspace_bytes(int batch);
int ssdk_augment_boxes(const ssdk_augment_image* images, const ssdk_augment_params* params, const int* candidates, int attempts,
                       const float* rows_in, int gt_stride, const int* offsets_in, int batch, int total_rows, int out_w, int out_h,
                       float* rows_out, int* offsets_out, int* attempt_out, int* windows_out, void* workspace, size_t workspace_bytes,
                       void* stream);
/*
 * Stages 2 and 3: the two statistics passes and the gather, given the windows.
 *   src [src_bytes]  DEV uint8: the ragged image buffer.  An image whose descriptor does not fit into it is read nowhere and is all fill.
 *   windows          DEV int32 [batch, 4] (ssdk_augment_boxes' windows_out, or the caller's own)
 *   divide_255       ToFloatTensor(normalize=True);  mean_std HOST float [6]: Normalize's mean[3] then std[3] (std != 0), read during the call
 *   out              DEV fp32 [batch, 3, out_h, out_w] = ((v / 255) - mean) / std
 * Three launches (both statistics passes leave at once for images that do not need them), no allocation, no synchronisation.
 */
size_t ssdk_augment_images_workspace_bytes(int batch);
int ssdk_augment_images(const unsigned char* src, long long src_bytes, const ssdk_augment_image* images, const ssdk_augment_params* params,
                        const int* windows, int batch, int out_w, int out_h, int divide_255, const float* mean_std, float* out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- evaluation metric -----------------------------------------------------------------------------
 * detection/metrics/mean_average_precision.py:10-116  mean_average_precision(predictions, gts, class_labels, iou_threshold, voc)
 *   predictions [n_pred, 7] device: image id, corner box, class id, score (the rows bf/eval.py:58-66 builds from the
 *   postprocessor's output).  Ground truth as for ssdk_encode_ground_truth: rows [total_gt, gt_stride] + offsets
 *   int32[num_images + 1]; class at column 4; difficult flag at column 6 when gt_stride > 6 (reference :22).
 *   Class ids are integers in [0, num_classes).  ap_out[num_classes]: AP of every class with at least one counted ground
 *   truth, NaN for the others; map_out[1] (double): their mean (:111).  voc != 0: 11-point interpolation (:99-103).
 *   Score ties (the reference's argsort is unstable): lower prediction row first.  The reference's 0/0 -> NaN precision
 *   for a class whose best prediction hits a difficult box is reproduced. */
size_t ssdk_mean_average_precision_workspace_bytes(long long n_pred, long long total_gt, int num_classes);
int ssdk_mean_average_precision(const float* predictions, long long n_pred, const float* gt_rows, int gt_stride,
                                const int* gt_offsets, int num_images, long long total_gt, int num_classes,
                                float iou_threshold, int voc, float* ap_out, double* map_out, void* workspace,
                                size_t workspace_bytes, void* stream);
/* The same call with the integer quantities behind the mean (ABI 126; each may be NULL; same workspace size):
 *   order_out   DEV uint32 [n_pred]: prediction rows in (class ascending, score descending, row ascending) order -- the order of the
 *               per-class cumulative counts; rows of a foreign class (c < 0 or c >= num_classes) come last, in row order.  -0.0 and
 *               +0.0 are one score (the reference's comparison): they tie and fall back to row order.
 *   outcome_out DEV uint8 [n_pred], indexed by prediction row: 0 = neither counter moves (a hit on a difficult box, or a foreign
 *               class), 1 = true positive, 2 = false positive.
 * ssdk_mean_average_precision forwards here with two NULLs. */
int ssdk_mean_average_precision_ex(const float* predictions, long long n_pred, const float* gt_rows, int gt_stride,
                                   const int* gt_offsets, int num_images, long long total_gt, int num_classes,
                                   float iou_threshold, int voc, float* ap_out, double* map_out, uint32_t* order_out,
                                   uint8_t* outcome_out, void* workspace, size_t workspace_bytes, void* stream);

/* The stable LSD radix sort both orders above are made with, on its own: (uint64 key, uint32 value) pairs, ascending on key bits
 * [0, end_bit) -- higher bits are ignored -- equal keys keep their input order.  All four arrays DEV [n].  keys / vals are NOT
 * modified: they are staged in the workspace first, so keys_out == keys (and vals_out == vals) is allowed.
 * SSDK_E_INVALID for n < 0, n >= 2^31, end_bit outside 1..64 or a null array with n > 0; SSDK_E_WORKSPACE for a missing or too small
 * workspace (ssdk_sort_pairs_u64_workspace_bytes(n); 0 for an n that is refused).  A refused call launches nothing and writes nothing. */
size_t ssdk_sort_pairs_u64_workspace_bytes(long long n);
int ssdk_sort_pairs_u64(const uint64_t* keys, const uint32_t* vals, long long n, int end_bit, uint64_t* keys_out, uint32_t* vals_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- COCO-style bbox evaluation: AP@[.50:.95], area bins, AR (ABI 131; not in the reference) --------------------------
 * The published COCO rules (COCOeval.evaluateImg / accumulate / summarize), for boxes, on the device.
 * Inputs.  predictions and ground truth as for ssdk_mean_average_precision; a non-zero column 6 (gt_stride > 6) marks a CROWD region
 * (COCO's iscrowd, which is also its ignore).  gt_area DEV fp64 [total_gt] or NULL: the annotation's area (NULL: the box area).
 * image_area_scale DEV fp64 [num_images] or NULL: multiplies every area of that image, gt (gt_area included) and detection, for the
 * area-range test only (normalised boxes; NULL: 1).  Tables: iou_thrs DEV fp64 [T], rec_thrs DEV fp64 [R], area_rngs DEV fp64 [A][2]
 * (lo, hi), max_dets HOST int32 [M], positive and strictly ascending (it sizes the walk, so the host must know it).
 * Limits: T, A, M, R >= 1, T * A <= 64, M <= 4, R <= 1024, T * R * K * A * M < 2^31; anything else is refused with SSDK_E_INVALID, nothing launched.
 * Arithmetic (evaluateImg / maskUtils.iou): fp64 from the fp32 coordinates, every operation rounded on its own.  area = (x2 - x1) * (y2 - y1);
 * inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1)); iou = inter / (area_d + area_g - inter), inter / area_d for a crowd gt,
 * 0 for a zero denominator.
 * Groups (evaluateImg): the detections of an (image, class) are ranked by (score descending, row ascending; -0.0 == +0.0); the first
 * max_dets[M - 1] take part.  Per (threshold t, area range a): a gt is ignored when it is crowd or its area is < lo or > hi; gts are
 * visited with the counted ones first, each part in row order; a detection in rank order takes the gt of the largest IoU >=
 * min(t, 1 - 1e-10) (the last of equals), skipping gts already matched unless crowd, and never trading a counted match for an ignored
 * gt; it inherits its gt's ignore flag; unmatched, it is ignored when its own area lies outside [lo, hi].
 * Accumulation (accumulate): per (class k, a, max_dets m, t) the detections of rank < max_dets[m] in (score descending, image ascending,
 * row ascending) order; tp = matched & ~ignored, fp = ~matched & ~ignored, cumulative; npig = class-k gts not ignored under a.  npig == 0:
 * precision and recall are -1.  Otherwise rc = tp / npig, pr = tp / (fp + tp + 2^-52), recall = rc[last] (0 without detections), pr
 * becomes its reverse running maximum, precision[t, r] = pr at the first position with rc >= rec_thrs[r], 0 when there is none.
 * Outputs, all DEV fp64: precision [T, R, K, A, M], recall [T, K, A, M] (pycocotools' index order) and stats[12] (summarize) = AP, AP50,
 * AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl: the mean of the entries > -1 of a slice, -1 without any.  All-area statistics
 * take range 0, the s / m / l ones ranges 1 / 2 / 3; every AP and ARs / ARm / ARl take max_dets[M - 1], AR1 / AR10 / AR100 take max_dets[0] /
 * [1] / [2]; a statistic whose index does not exist is -1; AP50 / AP75 take the threshold within 1e-9 of 0.5 / 0.75, -1 when absent.
 * A detection of a class outside [0, num_classes) takes part in nothing; one of an image outside [0, num_images) has no ground truth.
 * Every result is a function of the inputs alone: two runs give the same bits. */
size_t ssdk_coco_eval_workspace_bytes(long long n_pred, long long total_gt, int num_classes, int num_iou_thrs, int num_area_rngs);
int ssdk_coco_eval(const float* predictions, long long n_pred, const float* gt_rows, int gt_stride, const int* gt_offsets, int num_images,
                   long long total_gt, int num_classes, const double* gt_area, const double* image_area_scale, const double* iou_thrs,
                   int num_iou_thrs, const double* rec_thrs, int num_rec_thrs, const double* area_rngs, int num_area_rngs, const int* max_dets,
                   int num_max_dets, double* precision, double* recall, double* stats, void* workspace, size_t workspace_bytes, void* stream);
/* The same call with the integer quantities behind the curves (each may be NULL; same workspace size):
 *   rank_out  DEV int32 [n_pred] by prediction row: the position within its (image, class) group (evaluateImg's score order), -1 for a
 *             foreign class.
 *   flags_out DEV uint8 [n_pred, T * A] by prediction row, pair (t, a) at t * A + a: bit 0 = matched, bit 1 = ignored; 0 for a foreign class
 *             and for rank >= max_dets[M - 1].
 *   order_out DEV uint32 [n_pred]: prediction rows in (class ascending, score descending, image ascending, row ascending) order --
 *             accumulate's order; foreign classes last, in (image, row) order.  Image ids order as signed integers.
 *   npig_out  DEV int32 [K, A]. */
int ssdk_coco_eval_ex(const float* predictions, long long n_pred, const float* gt_rows, int gt_stride, const int* gt_offsets, int num_images,
                      long long total_gt, int num_classes, const double* gt_area, const double* image_area_scale, const double* iou_thrs,
                      int num_iou_thrs, const double* rec_thrs, int num_rec_thrs, const double* area_rngs, int num_area_rngs, const int* max_dets,
                      int num_max_dets, double* precision, double* recall, double* stats, int32_t* rank_out, uint8_t* flags_out,
                      uint32_t* order_out, int32_t* npig_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- integral box head + Distribution Focal Loss (Generalized Focal Loss, arXiv:2006.04388; ABI 127; not in the reference) ----------
 *
 * Shapes.  bins = reg_max + 1, 2 <= bins <= 64.  The loc logits are z [B, A, 4, bins] (a row of 4 * bins floats per anchor); side
 * k = 0..3 is the encoded coordinate tx, ty, tw, th of box_coder.py:22-30 (xy_scale, wh_scale, eps; the in-place form).
 * Value grid.  v_k[i] = -L_k + i * (2 L_k / reg_max), L_k = xy_limit for k = 0, 1 and wh_limit for k = 2, 3.
 * Integral.  p = softmax(z[b, a, k, :]) with the row maximum subtracted first; loc[b, a, k] = sum_i p_i v_k[i].  locs [B, A*4] is an
 * ordinary encoded loc tensor: ssdk_multibox_loss_fwd, ssdk_decode_box and ssdk_postprocess take it as it is.
 * DFL.  On positive rows only (class != 0 && class != -1, as the box terms).  t_k = the row's encoded target, from its RAW corners and
 * its anchor, op for op as ssdk_multibox_loss_fwd encodes it; y = fminf(fmaxf((t_k + L_k) / step_k, 0), reg_max);
 * yl = min(floor(y), reg_max - 1), yr = yl + 1; the side's term is lse(z) - ((yr - y) z[yl] + (y - yl) z[yr]); the row's term is the
 * mean of its four sides, not weighted by target column 5 (like the box terms); the batch value is
 * distribution_weight * sum / max(1, #positives).  The clamp is DFL's alone: the box term on the expectation sees the true target.
 * Gradients.  dz_i = g_dfl * distribution_weight / (4 max(1, #positives)) * (p_i - (yr - y)[i == yl] - (y - yl)[i == yr])
 *                  + dloc_k * p_i * (v_k[i] - loc_k); rows that are not positive receive zeros.
 * No atomics, nothing zero-filled beforehand, every sum in an order fixed by the launch: results repeat bit for bit (run to run, eager
 * against a replayed HIP graph); ssdk_set_deterministic changes nothing here.
 * Refused with SSDK_E_INVALID, nothing launched or written: bins outside [2, 64], a limit or scale that is not positive, NULL logits /
 * locs / dlogits, a target without anchors (or without out), a DFL gradient without the class column; SSDK_E_WORKSPACE for a target
 * (class column) without a large enough workspace.  New fields are only ever appended to the struct. */
typedef struct ssdk_integral_params {
    int bins;
    float xy_limit, wh_limit;
    float xy_scale, wh_scale, eps;
    float distribution_weight; /* 0: integral regression alone -- the positives are still counted, the term and y are skipped */
} ssdk_integral_params;
size_t ssdk_integral_workspace_bytes(int batch, int num_anchors);
/* One pass over the logits (+ the one-workgroup sum of the per-workgroup partials when there is a target).
 *   logits DEV [B, A, 4, bins], 16-byte aligned; anchors DEV [A, 4] or NULL; target DEV [B, A, 6] or NULL (postprocess, evaluation: the
 *   integral alone; out and the workspace are then neither needed nor touched).
 *   locs DEV [B, A, 4]; out DEV [2] = (DFL value, #positives as float); workspace: caller-owned, kept until the backward has run --
 *   it holds each positive row's four y and the divider.
 * With a target, call it BEFORE ssdk_multibox_loss_fwd, which overwrites the raw corners under the SmoothL1 family; the backward reads
 * y from the workspace (both directions see the same target) and never reads target columns 0..3. */
int ssdk_integral_fwd(const ssdk_integral_params* params, const float* logits, const float* anchors, const float* target, int batch,
                      int num_anchors, float* locs, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* One launch.  dlocs DEV [B, A, 4] or NULL (zeros; no fill launch needed); target_classes DEV: the class column, element r at
 * target_classes[r * class_stride] (6 for a [B, A, 6] target), or NULL: every row counts as positive and there is no DFL term (the
 * backward of the integral alone; no workspace); grad_dfl DEV [1]: the upstream gradient of the DFL value, or NULL (0).
 * dlogits DEV [B, A, 4, bins], 16-byte aligned, written densely: a tile of rows without a positive is stored as zeros without reading
 * its logits; a positive row's logits are read once. */
int ssdk_integral_bwd(const ssdk_integral_params* params, const float* logits, const float* dlocs, const float* target_classes,
                      int class_stride, const float* grad_dfl, int batch, int num_anchors, float* dlogits, void* workspace,
                      size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_H_ */
