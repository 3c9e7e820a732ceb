// augment.hip -- device-side SSD augmentation (include/ssdk.h, ABI 133): bf/preprocessing/transforms.py + functional/{img,box}.py
// as ONE gather per output pixel.  Expand, crop, flips and resize each map an axis-aligned window onto another, so they compose into one
// window in source coordinates; the colour steps are pointwise and are applied to the source bytes as they are read.
//
//   ssdk_augment_boxes    augment_choose_kernel (one wavefront per image: the first acceptable crop candidate, the window, the box count)
//                         augment_write_kernel  (one wavefront per image: offsets, surviving rows back to back in input order)
//   ssdk_augment_images   augment_stats_kernel<1> (per-channel mean after hue/saturation + brightness; contrast images only)
//                         augment_stats_kernel<2> (scalar mean after the contrast step; expanding images only)
//                         augment_gather_kernel   (bilinear gather, colour, normalise, planar fp32 store)
//
// Box arithmetic is float32, one rounding per operation (this TU is built -ffp-contract=off), in the order of functional/box.py.
#include "common.h"

namespace ssdk {

constexpr int kAugWaves = 4;         // images per workgroup of the two box kernels
constexpr int kAugParts = 128;       // workgroups per image of a statistics pass: a FIXED partition, so the sums are the same bits run to run
constexpr int kAugThreads = 256;
static_assert(kAugThreads == 4 * kWave, "the statistics are finished by four wavefronts: three channel means and the fill");

// np.clip: NaN stays NaN
__device__ __forceinline__ float clipf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct AugGeom {
    int flags;
    int img_w, img_h;       // source
    int can_w, can_h;       // canvas: the image after the expand
    int ex, ey;             // where the source sits in the canvas
};

__device__ __forceinline__ AugGeom aug_geom(const ssdk_augment_image& im, const ssdk_augment_params& p) {
    AugGeom g;
    g.flags = p.flags;
    g.img_w = im.width > 0 ? im.width : 0;
    g.img_h = im.height > 0 ? im.height : 0;
    const bool ex = (p.flags & SSDK_AUG_EXPAND) != 0;
    g.can_w = ex ? p.expand_w : g.img_w;
    g.can_h = ex ? p.expand_h : g.img_h;
    g.ex = ex ? p.expand_x : 0;
    g.ey = ex ? p.expand_y : 0;
    return g;
}

struct AugWindow { int x, y, w, h; bool crop; };   // in canvas coordinates; crop: a candidate was accepted

// functional/box.py:62-69: the box's zero_incorrect intersection with the region and the IoU of the box with it
__device__ __forceinline__ void crop_box(float4 t, float rx1, float ry1, float rx2, float ry2, float4& n, float& iou) {
    const float mnx = tmaxf(rx1, t.x), mny = tmaxf(ry1, t.y), mxx = tminf(rx2, t.z), mxy = tminf(ry2, t.w);
    const bool neg = (mxx < mnx) || (mxy < mny);
    n = neg ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(mnx, mny, mxx, mxy);
    iou = iou_corner(t, area4(t.x, t.y, t.z, t.w), n, area4(n.x, n.y, n.z, n.w));
}

__device__ __forceinline__ bool crop_keeps(float4 t, float rx1, float ry1, float rx2, float ry2, float iou, int flags, float min_iou) {
    if (flags & SSDK_AUG_KEEP_IOU) return iou > min_iou;
    const float cx = (t.x + t.z) / 2.0f, cy = (t.y + t.w) / 2.0f;   // box.py:73-74, strict on both sides
    return cx > rx1 && cy > ry1 && cx < rx2 && cy < ry2;
}

__device__ __forceinline__ float4 expand_box(float4 t, const AugGeom& g) {
    if (g.flags & SSDK_AUG_EXPAND) {   // (no add at all without the expand: x + 0 would turn -0 into +0)
        const float ex = (float)g.ex, ey = (float)g.ey;
        t = make_float4(t.x + ex, t.y + ey, t.z + ex, t.w + ey);
    }
    return t;
}

// raw row -> final corners; false: the box is dropped (by the crop's keep criterion or as degenerate after the resize)
__device__ __forceinline__ bool final_box(float4 t, const AugGeom& g, const AugWindow& w, float min_iou, int out_w, int out_h, float4& out) {
    t = expand_box(t, g);
    if (w.crop) {
        const float rx1 = (float)w.x, ry1 = (float)w.y, rx2 = (float)(w.x + w.w - 1), ry2 = (float)(w.y + w.h - 1);
        float4 n;
        float iou;
        crop_box(t, rx1, ry1, rx2, ry2, n, iou);
        if (!crop_keeps(t, rx1, ry1, rx2, ry2, iou, g.flags, min_iou)) return false;
        const float hx = (float)(w.w - 1), hy = (float)(w.h - 1);
        t = make_float4(clipf(n.x - rx1, 0.0f, hx), clipf(n.y - ry1, 0.0f, hy), clipf(n.z - rx1, 0.0f, hx), clipf(n.w - ry1, 0.0f, hy));
    }
    if (g.flags & SSDK_AUG_HFLIP) {
        const float m = (float)(w.w - 1);
        t = make_float4(m - t.z, t.y, m - t.x, t.w);
    }
    if (g.flags & SSDK_AUG_VFLIP) {
        const float m = (float)(w.h - 1);
        t = make_float4(t.x, m - t.w, t.z, m - t.y);
    }
    const float sx = (float)((double)out_w / (double)w.w), sy = (float)((double)out_h / (double)w.h);   // box.py:11-12: a float64 ratio, rounded once
    const float hx = (float)(out_w - 1), hy = (float)(out_h - 1);
    t = make_float4(clipf(t.x * sx, 0.0f, hx), clipf(t.y * sy, 0.0f, hy), clipf(t.z * sx, 0.0f, hx), clipf(t.w * sy, 0.0f, hy));
    out = t;
    return !(t.x == t.z || t.y == t.w);   // detection_dataset.py:31-32
}

__device__ __forceinline__ float4 load_box(const float* __restrict__ rows, int stride, int r) {
    const float* p = rows + (long long)r * stride;
    return make_float4(p[0], p[1], p[2], p[3]);
}

// rows [r0, r0 + n) of image b, or nothing where the offsets make no sense
__device__ __forceinline__ void image_rows(const int* __restrict__ off, int b, int total, int& r0, int& n) {
    r0 = off[b];
    n = off[b + 1] - r0;
    if (r0 < 0 || n < 0 || (long long)r0 + n > (long long)total) { r0 = 0; n = 0; }
}

__device__ __forceinline__ bool candidate_valid(int4 c, const AugGeom& g) {
    return c.z > 0 && c.w > 0 && c.x >= 0 && c.y >= 0 && c.z <= g.can_w && c.w <= g.can_h && c.x <= g.can_w - c.z && c.y <= g.can_h - c.w;
}

__device__ __forceinline__ AugWindow window_of(int chosen, const int* __restrict__ cand, int attempts, int b, const AugGeom& g) {
    AugWindow w;
    w.crop = chosen >= 0;
    if (w.crop) {
        const int* c = cand + ((long long)b * attempts + chosen) * 4;
        w.x = c[0]; w.y = c[1]; w.w = c[2]; w.h = c[3];
    } else {
        w.x = 0; w.y = 0; w.w = g.can_w; w.h = g.can_h;
    }
    if (w.w < 1) w.w = 1;   // (an image of no size: keeps the ratios finite; it has no pixel to read)
    if (w.h < 1) w.h = 1;
    return w;
}

// ---- stage 1a: the first acceptable candidate, the window for the gather, the number of boxes that survive -----------------------------
__global__ void __launch_bounds__(kAugWaves * kWave)
augment_choose_kernel(const ssdk_augment_image* __restrict__ images, const ssdk_augment_params* __restrict__ params, const int* __restrict__ cand,
                      int attempts, const float* __restrict__ rows_in, int stride, const int* __restrict__ off_in, int batch, int total, int out_w,
                      int out_h, int* __restrict__ attempt_out, int* __restrict__ windows, int* __restrict__ counts) {
    const int b = blockIdx.x * kAugWaves + (threadIdx.x >> 6), lane = lane_id();
    if (b >= batch) return;   // (wave-uniform; the kernel has no workgroup barrier)
    const ssdk_augment_params p = params[b];
    const AugGeom g = aug_geom(images[b], p);
    int r0, n;
    image_rows(off_in, b, total, r0, n);
    int chosen = -2;
    if (p.flags & SSDK_AUG_CROP) {
        chosen = -1;
        for (int a = 0; a < attempts; ++a) {
            const int* cp = cand + ((long long)b * attempts + a) * 4;
            const int4 c = make_int4(cp[0], cp[1], cp[2], cp[3]);
            if (!candidate_valid(c, g)) continue;                  // img.py:69-70
            if (n == 0) { chosen = a; break; }                     // box.py:63-64
            const float rx1 = (float)c.x, ry1 = (float)c.y, rx2 = (float)(c.x + c.z - 1), ry2 = (float)(c.y + c.w - 1);
            float mx = -INFINITY;
            int nan = 0, kept = 0;
            for (int i = lane; i < n; i += kWave) {
                const float4 t = expand_box(load_box(rows_in, stride, r0 + i), g);
                float4 nb;
                float iou;
                crop_box(t, rx1, ry1, rx2, ry2, nb, iou);
                if (iou != iou) nan = 1; else mx = fmaxf(mx, iou);
                kept += crop_keeps(t, rx1, ry1, rx2, ry2, iou, p.flags, p.min_iou) ? 1 : 0;
            }
            mx = wave_allreduce(mx, OpMaxF());
            nan = wave_allreduce(nan, OpAddI());
            kept = wave_allreduce(kept, OpAddI());
            // box.py:71, :80: numpy's max is NaN as soon as one IoU is, and NaN > min_iou is false
            if (nan == 0 && mx > p.min_iou && kept >= p.min_objects_kept) { chosen = a; break; }
        }
    }
    const AugWindow w = window_of(chosen, cand, attempts, b, g);
    int count = 0;
    for (int i = lane; i < n; i += kWave) {
        float4 o;
        count += final_box(load_box(rows_in, stride, r0 + i), g, w, p.min_iou, out_w, out_h, o) ? 1 : 0;
    }
    count = wave_allreduce(count, OpAddI());
    if (lane == 0) {
        attempt_out[b] = chosen;
        counts[b] = count;
        windows[b * 4 + 0] = w.x - g.ex;   // source coordinates: the canvas' origin lies at (-ex, -ey)
        windows[b * 4 + 1] = w.y - g.ey;
        windows[b * 4 + 2] = w.w;
        windows[b * 4 + 3] = w.h;
    }
}

// ---- stage 1b: offsets and rows ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kAugWaves * kWave)
augment_write_kernel(const ssdk_augment_image* __restrict__ images, const ssdk_augment_params* __restrict__ params, const int* __restrict__ cand,
                     int attempts, const float* __restrict__ rows_in, int stride, const int* __restrict__ off_in, int batch, int total, int out_w,
                     int out_h, const int* __restrict__ attempt_in, const int* __restrict__ counts, float* __restrict__ rows_out,
                     int* __restrict__ off_out) {
    const int b = blockIdx.x * kAugWaves + (threadIdx.x >> 6), lane = lane_id();
    if (b >= batch) return;
    int base = 0;
    for (int i = lane; i < b; i += kWave) base += counts[i];   // (integers: any order gives the same sum)
    base = wave_allreduce(base, OpAddI());
    if (lane == 0) {
        off_out[b] = base;
        if (b == batch - 1) off_out[batch] = base + counts[b];
    }
    const ssdk_augment_params p = params[b];
    const AugGeom g = aug_geom(images[b], p);
    int r0, n;
    image_rows(off_in, b, total, r0, n);
    const AugWindow w = window_of(attempt_in[b], cand, attempts, b, g);
    for (int i0 = 0; i0 < n; i0 += kWave) {
        const int i = i0 + lane;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const bool keep = i < n && final_box(load_box(rows_in, stride, r0 + i), g, w, p.min_iou, out_w, out_h, o);
        const unsigned long long mask = __ballot(keep);
        const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && pos < total) {
            const float* src = rows_in + (long long)(r0 + i) * stride;
            float* dst = rows_out + (long long)pos * stride;
            dst[0] = o.x; dst[1] = o.y; dst[2] = o.z; dst[3] = o.w;
            for (int c = 4; c < stride; ++c) dst[c] = src[c];   // class, score and whatever else the row carries
        }
        base += __popcll(mask);
    }
}

// ---- colour: steps 1-4 on one source pixel ---------------------------------------------------------------------------------------------
struct AugColour {
    int flags;
    float hue6, sat, bright, contrast;   // hue shift in sextants (delta * 6 = delta * 360 degrees / 60)
    float mean[3];
};

__device__ __forceinline__ float hsv_channel(float n, float h, float v, float vs) {
    float k = n + h;
    k = k - 6.0f * floorf(k / 6.0f);
    const float m = fmaxf(0.0f, fminf(fminf(k, 4.0f - k), 1.0f));
    return v - vs * m;
}

// steps 1-3: hue/saturation in float HSV, to float, brightness
__device__ __forceinline__ float3 colour_pre(float r, float g, float b, const AugColour& c) {
    if (c.flags & SSDK_AUG_HUE_SATURATION) {
        const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b)), ch = mx - mn;
        float h = 0.0f;
        if (ch > 0.0f) {
            if (mx == r) h = (g - b) / ch;
            else if (mx == g) h = 2.0f + (b - r) / ch;
            else h = 4.0f + (r - g) / ch;
        }
        float s = mx > 0.0f ? ch / mx : 0.0f;
        h = h + c.hue6;
        s = clipf(s * c.sat, 0.0f, 1.0f);
        const float vs = mx * s;
        r = hsv_channel(5.0f, h, mx, vs);
        g = hsv_channel(3.0f, h, mx, vs);
        b = hsv_channel(1.0f, h, mx, vs);
    }
    if (c.flags & SSDK_AUG_BRIGHTNESS) {
        r = clipf(r + c.bright, 0.0f, 255.0f);
        g = clipf(g + c.bright, 0.0f, 255.0f);
        b = clipf(b + c.bright, 0.0f, 255.0f);
    }
    return make_float3(r, g, b);
}
// step 4
__device__ __forceinline__ float3 colour_contrast(float3 v, const AugColour& c) {
    if (c.flags & SSDK_AUG_CONTRAST) {
        v.x = clipf(c.mean[0] + c.contrast * (v.x - c.mean[0]), 0.0f, 255.0f);
        v.y = clipf(c.mean[1] + c.contrast * (v.y - c.mean[1]), 0.0f, 255.0f);
        v.z = clipf(c.mean[2] + c.contrast * (v.z - c.mean[2]), 0.0f, 255.0f);
    }
    return v;
}

__device__ __forceinline__ AugColour colour_of(const ssdk_augment_params& p) {
    AugColour c;
    c.flags = p.flags;
    c.hue6 = p.hue_delta * 6.0f;
    c.sat = p.saturation;
    c.bright = p.brightness;
    c.contrast = p.contrast;
    c.mean[0] = c.mean[1] = c.mean[2] = 0.0f;
    return c;
}

// the image's bytes, or null where its descriptor does not fit the buffer (such an image reads nothing and is all fill)
__device__ __forceinline__ const unsigned char* image_bytes(const unsigned char* __restrict__ src, long long src_bytes, const ssdk_augment_image& im,
                                                            long long& npx) {
    npx = 0;
    if (im.width <= 0 || im.height <= 0 || im.offset < 0) return nullptr;
    const long long n = (long long)im.width * im.height;
    if (im.offset > src_bytes || n > (src_bytes - im.offset) / 3) return nullptr;
    npx = n;
    return src + im.offset;
}

// One channel's sum over the kAugParts workgroups of a pass, by ONE WAVEFRONT (every lane calls it): lane l adds the parts l, l + 64, ...
// in index order, then a butterfly over the lanes -- a fixed order, and every lane ends with the same bits.
__device__ __forceinline__ double parts_sum(const double* __restrict__ part, int b, int c) {
    double s = 0.0;
    for (int k = lane_id(); k < kAugParts; k += kWave) s += part[((long long)b * kAugParts + k) * 3 + c];
    return wave_allreduce(s, OpAddD());
}

// ---- stage 2: statistics.  PASS 1: per-channel sums after steps 1-3 (contrast images).  PASS 2: after step 4 (expanding images). --------
template <int PASS>
__global__ void __launch_bounds__(kAugThreads)
augment_stats_kernel(const unsigned char* __restrict__ src, long long src_bytes, const ssdk_augment_image* __restrict__ images,
                     const ssdk_augment_params* __restrict__ params, const double* __restrict__ part1, double* __restrict__ part_out) {
    __shared__ double red[kAugThreads / kWave];
    __shared__ float s_mean[3];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const ssdk_augment_params p = params[b];
    if (!(p.flags & (PASS == 1 ? SSDK_AUG_CONTRAST : SSDK_AUG_EXPAND))) return;   // (uniform over the workgroup)
    long long npx;
    const unsigned char* img = image_bytes(src, src_bytes, images[b], npx);
    AugColour col = colour_of(p);
    if (PASS == 2 && (p.flags & SSDK_AUG_CONTRAST)) {
        const int c = threadIdx.x >> 6;   // waves 0..2: one channel each
        if (c < 3) {
            const double sum = parts_sum(part1, b, c);
            if (lane_id() == 0) s_mean[c] = npx > 0 ? (float)(sum / (double)npx) : 0.0f;
        }
        __syncthreads();
        col.mean[0] = s_mean[0]; col.mean[1] = s_mean[1]; col.mean[2] = s_mean[2];
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 4
    for (long long i = (long long)chunk * kAugThreads + threadIdx.x; i < npx; i += (long long)kAugParts * kAugThreads) {
        const unsigned char* px = img + i * 3;
        float3 v = colour_pre((float)px[0], (float)px[1], (float)px[2], col);
        if (PASS == 2) v = colour_contrast(v, col);
        a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z;
    }
    a0 = block_sum(a0, red);
    a1 = block_sum(a1, red);
    a2 = block_sum(a2, red);
    if (threadIdx.x == 0) {
        double* o = part_out + ((long long)b * kAugParts + chunk) * 3;
        o[0] = a0; o[1] = a1; o[2] = a2;
    }
}

// ---- stage 3: the gather ---------------------------------------------------------------------------------------------------------------
struct AugNorm { int div255; float mean[3], std[3]; };

struct AugTap { int a, b; float w; };   // two taps in SOURCE coordinates and the weight of the second

// Resize's tap pair of output index d: src = (d + 0.5) * (win / out) - 0.5, clamped to the window, then flip, then window -> source
__device__ __forceinline__ AugTap make_tap(int d, double win_over_out, int win, int origin, bool flip) {
    const double s = ((double)d + 0.5) * win_over_out - 0.5;
    const double f = floor(s);
    AugTap t;
    t.w = (float)(s - f);
    int a = (int)f, b = a + 1;
    a = a < 0 ? 0 : (a > win - 1 ? win - 1 : a);
    b = b < 0 ? 0 : (b > win - 1 ? win - 1 : b);
    if (flip) { a = win - 1 - a; b = win - 1 - b; }
    t.a = a + origin;
    t.b = b + origin;
    return t;
}

__device__ __forceinline__ float3 read_tap(const unsigned char* __restrict__ img, int W, int H, int x, int y, const AugColour& col, float fill) {
    if (img == nullptr || x < 0 || y < 0 || x >= W || y >= H) return make_float3(fill, fill, fill);
    const unsigned char* px = img + ((long long)y * W + x) * 3;
    return colour_contrast(colour_pre((float)px[0], (float)px[1], (float)px[2], col), col);
}

__device__ __forceinline__ float lerp2(float p00, float p01, float p10, float p11, float wx, float wy) {
    const float top = (1.0f - wx) * p00 + wx * p01, bot = (1.0f - wx) * p10 + wx * p11;
    return (1.0f - wy) * top + wy * bot;
}

__device__ __forceinline__ float normalise(float v, const AugNorm& nm, int c) {
    if (nm.div255) v = v / 255.0f;
    return (v - nm.mean[c]) / nm.std[c];
}

// one thread per 4 adjacent output pixels of a row, all three channels; tpr = threads per row; vec: rows are float4-aligned
__global__ void __launch_bounds__(kAugThreads)
augment_gather_kernel(const unsigned char* __restrict__ src, long long src_bytes, const ssdk_augment_image* __restrict__ images,
                      const ssdk_augment_params* __restrict__ params, const int* __restrict__ windows, const double* __restrict__ part1,
                      const double* __restrict__ part2, float* __restrict__ out, int out_w, int out_h, int tpr, int vec, AugNorm nm) {
    __shared__ float s_stat[4];
    const int b = blockIdx.y;
    const ssdk_augment_params p = params[b];
    const ssdk_augment_image im = images[b];
    long long npx;
    const unsigned char* img = image_bytes(src, src_bytes, im, npx);
    const int wave = threadIdx.x >> 6;   // waves 0..2: the channel means; wave 3: the fill
    if (wave < 3) {
        float m = 0.0f;
        if ((p.flags & SSDK_AUG_CONTRAST) && npx > 0) m = (float)(parts_sum(part1, b, wave) / (double)npx);
        if (lane_id() == 0) s_stat[wave] = m;
    } else {
        float fill = 0.0f;
        if ((p.flags & SSDK_AUG_EXPAND) && npx > 0) {   // img.mean(): every channel of every pixel
            const double s = (parts_sum(part2, b, 0) + parts_sum(part2, b, 1)) + parts_sum(part2, b, 2);
            fill = (float)(s / (3.0 * (double)npx));
        }
        if (lane_id() == 0) s_stat[3] = fill;
    }
    __syncthreads();
    const long long t = (long long)blockIdx.x * kAugThreads + threadIdx.x;
    if (t >= (long long)out_h * tpr) return;
    AugColour col = colour_of(p);
    col.mean[0] = s_stat[0]; col.mean[1] = s_stat[1]; col.mean[2] = s_stat[2];
    const float fill = s_stat[3];
    const int y = (int)(t / tpr), x0 = (int)(t % tpr) * 4;
    const int wx0 = windows[b * 4 + 0], wy0 = windows[b * 4 + 1];
    int ww = windows[b * 4 + 2], wh = windows[b * 4 + 3];
    if (ww < 1) ww = 1;
    if (wh < 1) wh = 1;
    const int W = im.width, H = im.height;
    const double scale_x = (double)ww / (double)out_w, scale_y = (double)wh / (double)out_h;
    const AugTap ty = make_tap(y, scale_y, wh, wy0, (p.flags & SSDK_AUG_VFLIP) != 0);
    float r[4], g[4], bl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        r[j] = g[j] = bl[j] = 0.0f;
        if (x >= out_w) continue;
        const AugTap tx = make_tap(x, scale_x, ww, wx0, (p.flags & SSDK_AUG_HFLIP) != 0);
        const float3 p00 = read_tap(img, W, H, tx.a, ty.a, col, fill), p01 = read_tap(img, W, H, tx.b, ty.a, col, fill);
        const float3 p10 = read_tap(img, W, H, tx.a, ty.b, col, fill), p11 = read_tap(img, W, H, tx.b, ty.b, col, fill);
        r[j] = normalise(lerp2(p00.x, p01.x, p10.x, p11.x, tx.w, ty.w), nm, 0);
        g[j] = normalise(lerp2(p00.y, p01.y, p10.y, p11.y, tx.w, ty.w), nm, 1);
        bl[j] = normalise(lerp2(p00.z, p01.z, p10.z, p11.z, tx.w, ty.w), nm, 2);
    }
    const size_t plane = (size_t)out_h * out_w;
    float* o = out + (size_t)b * 3 * plane + (size_t)y * out_w + x0;
    if (vec) {   // out_w % 4 == 0 and a 16-byte aligned base: x0 + 3 < out_w
        *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(o + plane) = make_float4(g[0], g[1], g[2], g[3]);
        *reinterpret_cast<float4*>(o + 2 * plane) = make_float4(bl[0], bl[1], bl[2], bl[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j < out_w) {
                o[j] = r[j];
                o[plane + j] = g[j];
                o[2 * plane + j] = bl[j];
            }
        }
    }
}

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_augment_boxes_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return align_up(sizeof(int) * (size_t)batch, 256);
}

extern "C" int ssdk_augment_boxes(const ssdk_augment_image* images, const ssdk_augment_params* params, const int* candidates, int attempts,
                                  const float* rows_in, int gt_stride, const int* offsets_in, int batch, int total_rows, int out_w, int out_h,
                                  float* rows_out, int* offsets_out, int* attempt_out, int* windows_out, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    SSDK_REQUIRE(images && params && offsets_in && offsets_out && attempt_out && windows_out && batch > 0 && batch <= (1 << 20) && gt_stride >= 4 &&
                     total_rows >= 0 && attempts >= 0 && out_w > 0 && out_h > 0 && (attempts == 0 || candidates) &&
                     (total_rows == 0 || (rows_in && rows_out && rows_in != rows_out)),
                 SSDK_E_INVALID, "ssdk_augment_boxes: batch=%d total_rows=%d gt_stride=%d attempts=%d out=%dx%d (out-of-place only)", batch,
                 total_rows, gt_stride, attempts, out_w, out_h);
    SSDK_REQUIRE(workspace && workspace_bytes >= ssdk_augment_boxes_workspace_bytes(batch), SSDK_E_WORKSPACE,
                 "ssdk_augment_boxes: workspace of %zu bytes, %zu needed", workspace_bytes, ssdk_augment_boxes_workspace_bytes(batch));
    hipStream_t s = (hipStream_t)stream;
    int* counts = static_cast<int*>(workspace);
    const dim3 grid((unsigned)cdiv(batch, kAugWaves)), block(kAugWaves * kWave);
    hipLaunchKernelGGL(augment_choose_kernel, grid, block, 0, s, images, params, candidates, attempts, rows_in, gt_stride, offsets_in, batch, total_rows,
                       out_w, out_h, attempt_out, windows_out, counts);
    SSDK_CHECK_LAUNCH("augment_choose_kernel");
    hipLaunchKernelGGL(augment_write_kernel, grid, block, 0, s, images, params, candidates, attempts, rows_in, gt_stride, offsets_in, batch, total_rows,
                       out_w, out_h, attempt_out, counts, rows_out, offsets_out);
    SSDK_CHECK_LAUNCH("augment_write_kernel");
    return SSDK_OK;
}

extern "C" size_t ssdk_augment_images_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return 2 * align_up(sizeof(double) * 3 * kAugParts * (size_t)batch, 256);
}

extern "C" int ssdk_augment_images(const unsigned char* src, long long src_bytes, const ssdk_augment_image* images,
                                   const ssdk_augment_params* params, const int* windows, int batch, int out_w, int out_h, int divide_255,
                                   const float* mean_std, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    SSDK_REQUIRE(src && src_bytes >= 0 && images && params && windows && out && mean_std && batch > 0 && batch <= 65535 && out_w > 0 && out_h > 0 &&
                     (long long)out_w * out_h <= (1LL << 30),
                 SSDK_E_INVALID, "ssdk_augment_images: batch=%d out=%dx%d src_bytes=%lld", batch, out_w, out_h, src_bytes);
    AugNorm nm;
    nm.div255 = divide_255 != 0;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean_std[c];
        nm.std[c] = mean_std[3 + c];
        SSDK_REQUIRE(nm.mean[c] == nm.mean[c] && nm.std[c] == nm.std[c] && nm.std[c] != 0.0f, SSDK_E_INVALID,
                     "ssdk_augment_images: mean[%d]=%g std[%d]=%g", c, (double)nm.mean[c], c, (double)nm.std[c]);
    }
    SSDK_REQUIRE(workspace && workspace_bytes >= ssdk_augment_images_workspace_bytes(batch), SSDK_E_WORKSPACE,
                 "ssdk_augment_images: workspace of %zu bytes, %zu needed", workspace_bytes, ssdk_augment_images_workspace_bytes(batch));
    hipStream_t s = (hipStream_t)stream;
    Carver ws(workspace);
    double* part1 = ws.take<double>(3 * kAugParts * (size_t)batch);
    double* part2 = ws.take<double>(3 * kAugParts * (size_t)batch);
    const dim3 sgrid(kAugParts, (unsigned)batch);
    hipLaunchKernelGGL(augment_stats_kernel<1>, sgrid, dim3(kAugThreads), 0, s, src, src_bytes, images, params, (const double*)nullptr, part1);
    SSDK_CHECK_LAUNCH("augment_stats_kernel<1>");
    hipLaunchKernelGGL(augment_stats_kernel<2>, sgrid, dim3(kAugThreads), 0, s, src, src_bytes, images, params, (const double*)part1, part2);
    SSDK_CHECK_LAUNCH("augment_stats_kernel<2>");
    const int tpr = cdiv(out_w, 4);
    const int vec = (out_w % 4 == 0) && (((uintptr_t)out & 15) == 0);
    const long long threads = (long long)out_h * tpr;
    const dim3 ggrid((unsigned)((threads + kAugThreads - 1) / kAugThreads), (unsigned)batch);
    hipLaunchKernelGGL(augment_gather_kernel, ggrid, dim3(kAugThreads), 0, s, src, src_bytes, images, params, windows, (const double*)part1,
                       (const double*)part2, out, out_w, out_h, tpr, vec, nm);
    SSDK_CHECK_LAUNCH("augment_gather_kernel");
    return SSDK_OK;
}
