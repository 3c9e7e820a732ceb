// iou_loss.h -- the IoU-based box terms on corner boxes, per box: value and d value / dP of predicted corners P against target corners T.
// Included by loss.hip (the fused loss kernels) and boxes.hip (the row-wise entry points ssdk_box_iou_loss_fwd / _bwd); both translation
// units are built -ffp-contract=off, so one definition gives both the same bits.
//
//   SSDK_LOC_GIOU   1 - generalized_iou                                   giou_loss / giou_loss_grad (the reference's, as they were in loss.hip)
//   SSDK_LOC_IOU    1 - iou
//   SSDK_LOC_DIOU   1 - iou + rho2 / c2                                   arXiv:1911.08287
//   SSDK_LOC_CIOU   DIoU + alpha v                                        same paper; alpha is a constant of the step
//   SSDK_LOC_EIOU   DIoU + (w - wg)^2 / (cw^2 + eps) + (h - hg)^2 / (ch^2 + eps)   arXiv:2101.08158, without the focal factor
//
// area, inter, uni and iou = inter / uni are computed op for op as giou_loss computes them (area4, tmaxf, tminf, clamp0, no epsilon).
// cw, ch: the enclosing box's width and height (plain differences), c2 = cw^2 + ch^2 + eps; rho2: the squared distance of the centres;
// w, h of P and wg, hg of T: plain differences, not clamped; v = 4 / pi^2 (atan(wg / hg) - atan(w / h))^2, alpha = v / (1 - iou + v + eps).
// eps = 1e-7 (torchvision's) appears only where these terms add a denominator.
//
// Gradient rules (what torch autograd does for torch.max / torch.min / clamp(min=0)): max / min send the gradient to the selected
// argument, an exact tie splits it in half, clamp(0) passes it where its argument is >= 0.  A degenerate target (zero area, hg == 0) is
// outside the contract; a decoded prediction always has w, h > 0.
#pragma once

#include "common.h"

namespace ssdk {

// 1 - generalized_iou (box_utils.py:104-143, cartesian=False) of predicted corners P against target corners T
__device__ __forceinline__ float giou_loss(float4 P, float4 T) {
    const float inter = area4(tmaxf(P.x, T.x), tmaxf(P.y, T.y), tminf(P.z, T.z), tminf(P.w, T.w));
    const float uni = area4(P.x, P.y, P.z, P.w) + area4(T.x, T.y, T.z, T.w) - inter;
    const float enc = area4(tminf(P.x, T.x), tminf(P.y, T.y), tmaxf(P.z, T.z), tmaxf(P.w, T.w));
    return 1.0f - (inter / uni - (enc - uni) / enc);
}

// d(giou_loss)/dP: loss = 2 - inter/uni - uni/enc; max/min route the gradient to the selected argument (ties: half),
// clamp(0) passes it where its argument is >= 0 (what autograd does for box_utils.py:104-143)
__device__ __forceinline__ float4 giou_loss_grad(float4 P, float4 T) {
    const float pw = P.z - P.x, ph = P.w - P.y, cw = clamp0(pw), ch = clamp0(ph);
    const float area_p = cw * ch, area_t = area4(T.x, T.y, T.z, T.w);
    const float ix1 = tmaxf(P.x, T.x), iy1 = tmaxf(P.y, T.y), ix2 = tminf(P.z, T.z), iy2 = tminf(P.w, T.w);
    const float iw = clamp0(ix2 - ix1), ih = clamp0(iy2 - iy1), inter = iw * ih;
    const float uni = area_p + area_t - inter;
    const float ex1 = tminf(P.x, T.x), ey1 = tminf(P.y, T.y), ex2 = tmaxf(P.z, T.z), ey2 = tmaxf(P.w, T.w);
    const float ew = clamp0(ex2 - ex1), eh = clamp0(ey2 - ey1), enc = ew * eh;
    const float d_uni = inter / (uni * uni) - 1.0f / enc, d_enc = uni / (enc * enc);
    const float c_inter = -1.0f / uni - d_uni, c_area = d_uni;
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    auto sel = [](float a, float b, bool greater) { return greater ? (a > b ? 1.0f : (a == b ? 0.5f : 0.0f)) : (a < b ? 1.0f : (a == b ? 0.5f : 0.0f)); };
    if (pw >= 0.0f) { d.z += c_area * ch; d.x -= c_area * ch; }
    if (ph >= 0.0f) { d.w += c_area * cw; d.y -= c_area * cw; }
    if (ix2 - ix1 >= 0.0f) { const float g = c_inter * ih; d.z += g * sel(P.z, T.z, false); d.x -= g * sel(P.x, T.x, true); }
    if (iy2 - iy1 >= 0.0f) { const float g = c_inter * iw; d.w += g * sel(P.w, T.w, false); d.y -= g * sel(P.y, T.y, true); }
    if (ex2 - ex1 >= 0.0f) { const float g = d_enc * eh; d.z += g * sel(P.z, T.z, true); d.x -= g * sel(P.x, T.x, false); }
    if (ey2 - ey1 >= 0.0f) { const float g = d_enc * ew; d.w += g * sel(P.w, T.w, true); d.y -= g * sel(P.y, T.y, false); }
    return d;
}

constexpr float kIouEps = 1e-7f;               // torchvision's eps: only in the denominators the new terms add
constexpr float kFourOverPiSq = 0.40528473f;   // 4 / pi^2

// the kinds that compare decoded corners with the RAW target and leave the target alone
constexpr bool iou_kind(int k) { return k == SSDK_LOC_GIOU || (k >= SSDK_LOC_IOU && k <= SSDK_LOC_EIOU); }

// d max(a, b) / da (greater) or d min(a, b) / da: 1 where a is selected, 1/2 at an exact tie
__device__ __forceinline__ float sel_max(float a, float b) { return a > b ? 1.0f : (a == b ? 0.5f : 0.0f); }
__device__ __forceinline__ float sel_min(float a, float b) { return a < b ? 1.0f : (a == b ? 0.5f : 0.0f); }

template <int K>
__device__ __forceinline__ float iou_family_loss(float4 P, float4 T) {
    static_assert(K >= SSDK_LOC_IOU && K <= SSDK_LOC_EIOU, "iou_family_loss: SSDK_LOC_IOU, _DIOU, _CIOU or _EIOU");
    const float inter = area4(tmaxf(P.x, T.x), tmaxf(P.y, T.y), tminf(P.z, T.z), tminf(P.w, T.w));
    const float uni = area4(P.x, P.y, P.z, P.w) + area4(T.x, T.y, T.z, T.w) - inter;
    const float iou = inter / uni;
    if constexpr (K == SSDK_LOC_IOU) {
        return 1.0f - iou;
    } else {
        const float cw = tmaxf(P.z, T.z) - tminf(P.x, T.x), ch = tmaxf(P.w, T.w) - tminf(P.y, T.y);
        const float c2 = cw * cw + ch * ch + kIouEps;
        const float dx = (P.x + P.z - T.x - T.z) / 2.0f, dy = (P.y + P.w - T.y - T.w) / 2.0f;
        const float diou = 1.0f - iou + (dx * dx + dy * dy) / c2;
        const float w = P.z - P.x, h = P.w - P.y, wg = T.z - T.x, hg = T.w - T.y;
        if constexpr (K == SSDK_LOC_DIOU) {
            return diou;
        } else if constexpr (K == SSDK_LOC_CIOU) {
            const float a = atanf(wg / hg) - atanf(w / h);
            const float v = kFourOverPiSq * (a * a);
            const float alpha = v / (1.0f - iou + v + kIouEps);
            return diou + alpha * v;
        } else {
            const float dw = w - wg, dh = h - hg;
            return diou + dw * dw / (cw * cw + kIouEps) + dh * dh / (ch * ch + kIouEps);
        }
    }
}

// d(iou_family_loss<K>)/dP
template <int K>
__device__ __forceinline__ float4 iou_family_grad(float4 P, float4 T) {
    static_assert(K >= SSDK_LOC_IOU && K <= SSDK_LOC_EIOU, "iou_family_grad: SSDK_LOC_IOU, _DIOU, _CIOU or _EIOU");
    const float w = P.z - P.x, h = P.w - P.y, pw = clamp0(w), ph = clamp0(h);
    const float area_p = pw * ph, area_t = area4(T.x, T.y, T.z, T.w);
    const float ix1 = tmaxf(P.x, T.x), iy1 = tmaxf(P.y, T.y), ix2 = tminf(P.z, T.z), iy2 = tminf(P.w, T.w);
    const float iw = clamp0(ix2 - ix1), ih = clamp0(iy2 - iy1), inter = iw * ih;
    const float uni = area_p + area_t - inter;
    // 1 - inter / uni, uni = area_p + area_t - inter
    const float c_area = inter / (uni * uni), c_inter = -1.0f / uni - c_area;
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (w >= 0.0f) { d.z += c_area * ph; d.x -= c_area * ph; }
    if (h >= 0.0f) { d.w += c_area * pw; d.y -= c_area * pw; }
    if (ix2 - ix1 >= 0.0f) { const float g = c_inter * ih; d.z += g * sel_min(P.z, T.z); d.x -= g * sel_max(P.x, T.x); }
    if (iy2 - iy1 >= 0.0f) { const float g = c_inter * iw; d.w += g * sel_min(P.w, T.w); d.y -= g * sel_max(P.y, T.y); }
    if constexpr (K != SSDK_LOC_IOU) {
        const float cw = tmaxf(P.z, T.z) - tminf(P.x, T.x), ch = tmaxf(P.w, T.w) - tminf(P.y, T.y);
        const float c2 = cw * cw + ch * ch + kIouEps;
        const float dx = (P.x + P.z - T.x - T.z) / 2.0f, dy = (P.y + P.w - T.y - T.w) / 2.0f;
        const float rho2 = dx * dx + dy * dy;
        // rho2 / c2: d rho2 / dP = (dx, dy, dx, dy); d c2 = 2 cw d cw + 2 ch d ch
        float kx = -rho2 / (c2 * c2) * (2.0f * cw), ky = -rho2 / (c2 * c2) * (2.0f * ch);   // coefficients of d cw, d ch
        d.x += dx / c2; d.z += dx / c2; d.y += dy / c2; d.w += dy / c2;
        if constexpr (K == SSDK_LOC_CIOU) {
            const float wg = T.z - T.x, hg = T.w - T.y;
            const float a = atanf(wg / hg) - atanf(w / h);
            const float v = kFourOverPiSq * (a * a);
            const float alpha = v / (1.0f - inter / uni + v + kIouEps);
            // alpha dv: d atan(w / h) = (h dw - w dh) / (w^2 + h^2)
            const float k = alpha * (2.0f * kFourOverPiSq) * a / (w * w + h * h);
            const float gw = -k * h, gh = k * w;
            d.z += gw; d.x -= gw; d.w += gh; d.y -= gh;
        } else if constexpr (K == SSDK_LOC_EIOU) {
            const float dw = w - (T.z - T.x), dh = h - (T.w - T.y);
            const float cw2 = cw * cw + kIouEps, ch2 = ch * ch + kIouEps;
            const float gw = 2.0f * dw / cw2, gh = 2.0f * dh / ch2;
            d.z += gw; d.x -= gw; d.w += gh; d.y -= gh;
            kx -= dw * dw / (cw2 * cw2) * (2.0f * cw);
            ky -= dh * dh / (ch2 * ch2) * (2.0f * ch);
        }
        d.z += kx * sel_max(P.z, T.z); d.x -= kx * sel_min(P.x, T.x);
        d.w += ky * sel_max(P.w, T.w); d.y -= ky * sel_min(P.y, T.y);
    }
    return d;
}

// the box term of an IoU kind (iou_kind(K)): GIoU by the two functions above, the rest by the family's
template <int K>
__device__ __forceinline__ float corner_loss(float4 P, float4 T) {
    if constexpr (K == SSDK_LOC_GIOU) return giou_loss(P, T);
    else return iou_family_loss<K>(P, T);
}
template <int K>
__device__ __forceinline__ float4 corner_loss_grad(float4 P, float4 T) {
    if constexpr (K == SSDK_LOC_GIOU) return giou_loss_grad(P, T);
    else return iou_family_grad<K>(P, T);
}

}  // namespace ssdk
