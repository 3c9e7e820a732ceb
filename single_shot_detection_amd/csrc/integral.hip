// integral.hip -- the integral box head of Generalized Focal Loss (arXiv:2006.04388) and its Distribution Focal Loss (include/ssdk.h:
// ssdk_integral_fwd / ssdk_integral_bwd).  Not in the reference.
//
// The loc logits are z[B, A, 4, bins]: for each encoded box coordinate a discrete distribution over the value grid v_k[i].  The forward
// reads them once (loc = the expectation under softmax(z); on the positive rows also the DFL term, the positive count and the row's
// four target positions y, kept in the workspace for the backward); the backward writes dlogits once.  A (row, side) is `bins`
// contiguous floats, a row 4 * bins floats = `bins` 16-byte vectors, so a tile of rows is a contiguous, 16-byte aligned run:
//   integral_fwd_kernel   a tile of 64 rows (32 above 32 bins) streams into LDS with 16-byte coalesced loads, then one lane per
//                         (row, side) walks its `bins` floats in LDS -- the LDS row pitch is odd, so lanes never share a bank.
//                         Per-workgroup partial sums, summed in a fixed order by integral_finalize_kernel.
//   integral_bwd_kernel   the same tiles: a tile without a positive row is stored as zeros and reads no logits; otherwise only the
//                         positive rows' logits are loaded, their gradient replaces them in LDS, and the tile leaves in 16-byte stores.
// No atomics, no zero-fill, every sum in an order fixed by the launch.  Built -ffp-contract=off like loss.hip: the target encode is
// loss.hip's (loss_fwd_kernel), op for op.
#include <algorithm>
#include <math.h>

#include "common.h"

namespace ssdk {

constexpr int kIntThreads = 256;
constexpr int kIntMaxPartials = 2048;
constexpr int kIntMaxBins = 64;

struct IntegralState {  // in the workspace: written by integral_finalize_kernel, read by the backward
    float divider;      // max(1, #positives)
    float value;
    int npos;
    int pad;
};

struct IntegralWs {
    float* y;         // [B*A*4] target position in bin units of every positive (row, side); other rows are never written or read
    float* partials;  // [kIntMaxPartials]
    int* counts;      // [kIntMaxPartials]
    IntegralState* state;
};

static IntegralWs carve_integral_ws(void* ws, size_t n_rows, size_t* total) {
    Carver c(ws);
    IntegralWs w;
    w.y = c.take<float>(4 * n_rows);
    w.partials = c.take<float>(kIntMaxPartials);
    w.counts = c.take<int>(kIntMaxPartials);
    w.state = c.take<IntegralState>(1);
    if (total) *total = c.off;
    return w;
}

struct IntegralParams {
    int bins, pitch, tile_rows, vec_steps;  // pitch: LDS floats per (row, side), odd; vec_steps: 16-byte vectors per thread and tile
    float xy_limit, wh_limit, xy_scale, wh_scale, eps, weight;
};

// Where element 4 * threadIdx.x of a tile sits in LDS -- (row, side) slot and bin -- and how far kIntThreads vectors move it: the staging
// loops derive every element's place by additions (two integer divisions per thread and launch).
struct BinWalk {
    int rs0, i0, step_rs, step_i;
    __device__ __forceinline__ explicit BinWalk(int bins)
        : rs0(4 * (int)threadIdx.x / bins), i0(4 * (int)threadIdx.x % bins), step_rs(4 * kIntThreads / bins), step_i(4 * kIntThreads % bins) {}
};

// softmax statistics of one (row, side) in LDS: the row maximum m at bin im, s = sum exp(z - m), and d = E[v] - v[im], summed around the
// peak so that a sharp distribution keeps its relative accuracy (the peak's own term is exactly 0)
__device__ __forceinline__ void side_stats(const float* __restrict__ z, int bins, float step, float& m, int& im, float& s, float& d) {
    m = z[0];
    im = 0;
    for (int i = 1; i < bins; ++i) {
        const float x = z[i];
        if (x > m) { m = x; im = i; }
    }
    s = 0.0f;
    float sv = 0.0f;
    for (int i = 0; i < bins; ++i) {
        const float e = __expf(z[i] - m);
        s += e;
        sv += e * ((float)(i - im) * step);
    }
    d = sv / s;
}

// The row's encoded target coordinate of side k from its raw corners: box_utils.py:33-34 to_centroids(inplace), then box_coder.py:22-30
// encode_box(inplace) -- op for op loss.hip's loss_fwd_kernel.
__device__ __forceinline__ float encoded_side(float2 t01, float2 t23, float4 pr, int side, const IntegralParams& p) {
    t23.x -= t01.x; t23.y -= t01.y;
    t01.x += t23.x / 2.0f; t01.y += t23.y / 2.0f;
    t01.x -= pr.x; t01.y -= pr.y;
    t01.x /= pr.z; t01.y /= pr.w;
    t01.x *= p.xy_scale; t01.y *= p.xy_scale;
    t23.x /= pr.z; t23.y /= pr.w;
    t23.x += p.eps; t23.y += p.eps;
    t23.x = logf(t23.x); t23.y = logf(t23.y);
    t23.x *= p.wh_scale; t23.y *= p.wh_scale;
    return side == 0 ? t01.x : (side == 1 ? t01.y : (side == 2 ? t23.x : t23.y));
}

template <bool HAS_TARGET>
__global__ void __launch_bounds__(kIntThreads) integral_fwd_kernel(IntegralParams p, const float4* __restrict__ logits,
                                                                   const float4* __restrict__ anchors, const float* __restrict__ target,
                                                                   long long n_rows, int A, float* __restrict__ locs, float* __restrict__ ys,
                                                                   float* __restrict__ partials, int* __restrict__ counts) {
    extern __shared__ float4 s_tile4[];
    __shared__ float s_red[kIntThreads / kWave];
    __shared__ int s_redi[kIntThreads / kWave];
    float* s_tile = reinterpret_cast<float*>(s_tile4);
    const int tid = threadIdx.x, bins = p.bins, pitch = p.pitch, reg_max = bins - 1;
    const BinWalk walk(bins);
    const int side = tid & 3;
    const float L = side < 2 ? p.xy_limit : p.wh_limit;
    const float step = 2.0f * L / (float)reg_max;
    const long long last4 = n_rows * bins - 1;   // the last 16-byte vector of the logits
    float acc = 0.0f;
    int npos = 0;
    const long long n_tiles = (n_rows + p.tile_rows - 1) / p.tile_rows;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long r0 = tile * p.tile_rows;
        const int rows = (int)min((long long)p.tile_rows, n_rows - r0);
        // ---- stage: every load and store unconditional.  Vectors behind the tile's (or the tensor's) end land in LDS slots behind the
        // rows in use -- the allocation covers vec_steps * kIntThreads vectors -- and are never read.
        const long long g0 = r0 * bins;
        float4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < p.vec_steps) v[k] = logits[min(g0 + tid + k * kIntThreads, last4)];
        __syncthreads();   // (the previous tile's lanes have read their rows)
        if (pitch == bins) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < p.vec_steps) s_tile4[tid + k * kIntThreads] = v[k];
        } else {
            int rs = walk.rs0, i = walk.i0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < p.vec_steps) {
                    const float xs[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
                    int rs_ = rs, i_ = i;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        s_tile[rs_ * pitch + i_] = xs[j];
                        if (++i_ == bins) { i_ = 0; ++rs_; }
                    }
                    rs += walk.step_rs; i += walk.step_i;
                    if (i >= bins) { i -= bins; ++rs; }
                }
            }
        }
        __syncthreads();
        // ---- one lane per (row, side)
        if (tid < rows * 4) {
            const float* z = s_tile + tid * pitch;
            float m, s, d;
            int im;
            side_stats(z, bins, step, m, im, s, d);
            locs[r0 * 4 + tid] = (-L + (float)im * step) + d;
            if constexpr (HAS_TARGET) {
                const long long r = r0 + (tid >> 2);
                const float2* trow = reinterpret_cast<const float2*>(target + r * 6);  // 24-byte rows: 8-byte aligned
                const int cls = (int)trow[2].x;
                const bool pos = cls != 0 && cls != -1;
                npos += (pos && side == 0) ? 1 : 0;
                if (pos && p.weight != 0.0f) {
                    const float t = encoded_side(trow[0], trow[1], anchors[r % A], side, p);
                    const float y = fminf(fmaxf((t + L) / step, 0.0f), (float)reg_max);
                    const int yl = min((int)floorf(y), reg_max - 1);
                    const float wl = (float)(yl + 1) - y, wr = y - (float)yl;
                    ys[r0 * 4 + tid] = y;
                    acc += 0.25f * ((m + logf(s)) - (wl * z[yl] + wr * z[yl + 1]));
                }
            }
        }
    }
    if constexpr (HAS_TARGET) {
        const float a_ = block_sum(acc, s_red);
        const int n_ = block_sum(npos, s_redi);
        if (tid == 0) { partials[blockIdx.x] = a_; counts[blockIdx.x] = n_; }
    }
}

__global__ void __launch_bounds__(256) integral_finalize_kernel(const float* __restrict__ partials, const int* __restrict__ counts, int n_part,
                                                                float weight, IntegralState* __restrict__ state, float* __restrict__ out2) {
    __shared__ double s_red[4];
    __shared__ int s_redi[4];
    double a = 0.0;
    int n = 0;
    for (int k = threadIdx.x; k < n_part; k += blockDim.x) { a += (double)partials[k]; n += counts[k]; }
    a = block_sum(a, s_red);
    n = block_sum(n, s_redi);
    if (threadIdx.x == 0) {
        const float divider = (float)(n < 1 ? 1 : n);
        const float value = weight != 0.0f ? weight * (float)a / divider : 0.0f;
        state->divider = divider; state->value = value; state->npos = n; state->pad = 0;
        out2[0] = value; out2[1] = (float)n;
    }
}

__global__ void __launch_bounds__(kIntThreads) integral_bwd_kernel(IntegralParams p, const float4* __restrict__ logits, const float* __restrict__ dlocs,
                                                                   const float* __restrict__ target_cls, int cls_stride,
                                                                   const float* __restrict__ ys, const IntegralState* __restrict__ state,
                                                                   const float* __restrict__ grad_dfl, long long n_rows,
                                                                   float4* __restrict__ dlogits) {
    extern __shared__ float4 s_tile4[];
    __shared__ unsigned char s_pos[64];
    float* s_tile = reinterpret_cast<float*>(s_tile4);
    const int tid = threadIdx.x, bins = p.bins, pitch = p.pitch, reg_max = bins - 1;
    const BinWalk walk(bins);
    const int side = tid & 3;
    const float L = side < 2 ? p.xy_limit : p.wh_limit;
    const float step = 2.0f * L / (float)reg_max;
    // dfl = weight * sum(row means) / divider: each side's term carries weight / (4 divider) of the upstream scalar
    const float g_dfl = (grad_dfl && state && p.weight != 0.0f) ? grad_dfl[0] * p.weight / (4.0f * state->divider) : 0.0f;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const long long n_tiles = (n_rows + p.tile_rows - 1) / p.tile_rows;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long r0 = tile * p.tile_rows;
        const int rows = (int)min((long long)p.tile_rows, n_rows - r0);
        const int n4 = rows * bins;
        const long long g0 = r0 * bins;
        bool pos = false;
        if (tid < rows * 4) {
            pos = true;
            if (target_cls) {
                const int cls = (int)target_cls[(r0 + (tid >> 2)) * cls_stride];
                pos = cls != 0 && cls != -1;
            }
            if (side == 0) s_pos[tid >> 2] = pos ? 1 : 0;
        }
        if (!__syncthreads_or(pos)) {   // no positive row: zeros, and no logits read
            for (int v = tid; v < n4; v += kIntThreads) dlogits[g0 + v] = zero4;
            continue;   // (s_pos is rewritten only behind the next tile's barrier, which every thread reaches after its reads here)
        }
        // ---- stage the positive rows (a row is `bins` vectors: vector v belongs to row v / bins = (slot of its first element) / 4)
        {
            int rs = walk.rs0, i = walk.i0;
            for (int v = tid; v < n4; v += kIntThreads) {
                if (s_pos[rs >> 2]) {
                    const float4 x4 = logits[g0 + v];
                    const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
                    int rs_ = rs, i_ = i;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        s_tile[rs_ * pitch + i_] = xs[j];
                        if (++i_ == bins) { i_ = 0; ++rs_; }
                    }
                }
                rs += walk.step_rs; i += walk.step_i;
                if (i >= bins) { i -= bins; ++rs; }
            }
        }
        __syncthreads();
        // ---- one lane per positive (row, side): its gradient replaces its logits
        if (pos) {
            float* z = s_tile + tid * pitch;
            float m, s, d;
            int im;
            side_stats(z, bins, step, m, im, s, d);
            const float inv = 1.0f / s;
            const float dl = dlocs ? dlocs[r0 * 4 + tid] : 0.0f;
            int yl = -2;
            float wl = 0.0f, wr = 0.0f;
            if (g_dfl != 0.0f && target_cls) {
                const float y = ys[r0 * 4 + tid];
                yl = min((int)floorf(y), reg_max - 1);
                wl = (float)(yl + 1) - y; wr = y - (float)yl;
            }
            for (int i = 0; i < bins; ++i) {
                const float pi = __expf(z[i] - m) * inv;
                // v_i - loc = (v_i - v_im) - d
                float g = dl * pi * ((float)(i - im) * step - d);
                if (yl >= 0) g += g_dfl * (pi - (i == yl ? wl : 0.0f) - (i == yl + 1 ? wr : 0.0f));
                z[i] = g;
            }
        }
        __syncthreads();
        // ---- the tile leaves in 16-byte stores
        {
            int rs = walk.rs0, i = walk.i0;
            for (int v = tid; v < n4; v += kIntThreads) {
                float4 o = zero4;
                if (s_pos[rs >> 2]) {
                    float xs[4];
                    int rs_ = rs, i_ = i;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        xs[j] = s_tile[rs_ * pitch + i_];
                        if (++i_ == bins) { i_ = 0; ++rs_; }
                    }
                    o = make_float4(xs[0], xs[1], xs[2], xs[3]);
                }
                dlogits[g0 + v] = o;
                rs += walk.step_rs; i += walk.step_i;
                if (i >= bins) { i -= bins; ++rs; }
            }
        }
        __syncthreads();   // (s_pos and the tile are rewritten for the next one)
    }
}

static int integral_resident_blocks(const void* fn, size_t lds) {
    int dev = 0, cus = 256, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kIntThreads, lds) != hipSuccess || per_cu < 1) per_cu = 2;
    return cus * per_cu;
}

static int check_integral_params(const char* fn, const ssdk_integral_params* q) {
    SSDK_REQUIRE(q, SSDK_E_INVALID, "%s: null params", fn);
    SSDK_REQUIRE(q->bins >= 2 && q->bins <= kIntMaxBins, SSDK_E_INVALID, "%s: bins=%d outside [2, %d]", fn, q->bins, kIntMaxBins);
    SSDK_REQUIRE(q->xy_limit > 0.0f && q->wh_limit > 0.0f, SSDK_E_INVALID, "%s: xy_limit / wh_limit must be positive", fn);
    SSDK_REQUIRE(q->xy_scale > 0.0f && q->wh_scale > 0.0f, SSDK_E_INVALID, "%s: xy_scale / wh_scale must be positive", fn);
    return SSDK_OK;
}

// tile_rows * bins <= 2048 vectors: at most 8 per thread and tile
static IntegralParams to_device(const ssdk_integral_params* q) {
    IntegralParams p{};
    p.bins = q->bins; p.pitch = q->bins | 1;
    p.tile_rows = q->bins <= 32 ? 64 : 32;
    p.vec_steps = (p.tile_rows * p.bins + kIntThreads - 1) / kIntThreads;
    p.xy_limit = q->xy_limit; p.wh_limit = q->wh_limit; p.xy_scale = q->xy_scale; p.wh_scale = q->wh_scale; p.eps = q->eps;
    p.weight = q->distribution_weight;
    return p;
}

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_integral_workspace_bytes(int batch, int num_anchors) {
    size_t total = 0;
    carve_integral_ws(nullptr, (size_t)batch * (size_t)num_anchors, &total);
    return total;
}

extern "C" int ssdk_integral_fwd(const ssdk_integral_params* params, const float* logits, const float* anchors, const float* target, int batch,
                                 int num_anchors, float* locs, float* out2, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_integral_params("ssdk_integral_fwd", params);
    if (rc) return rc;
    SSDK_REQUIRE(batch > 0 && num_anchors > 0, SSDK_E_INVALID, "ssdk_integral_fwd: batch=%d anchors=%d", batch, num_anchors);
    SSDK_REQUIRE(logits && locs, SSDK_E_INVALID, "ssdk_integral_fwd: null logits / locs");
    SSDK_REQUIRE(((uintptr_t)logits & 15) == 0 && ((uintptr_t)locs & 3) == 0, SSDK_E_INVALID, "ssdk_integral_fwd: logits must be 16-byte aligned");
    SSDK_REQUIRE(!target || anchors, SSDK_E_INVALID, "ssdk_integral_fwd: a target needs the anchors");
    if (target) {
        SSDK_REQUIRE(out2, SSDK_E_INVALID, "ssdk_integral_fwd: a target needs out");
        SSDK_REQUIRE(((uintptr_t)anchors & 15) == 0 && ((uintptr_t)target & 7) == 0, SSDK_E_INVALID,
                     "ssdk_integral_fwd: anchors need 16-byte and target 8-byte alignment");
        SSDK_REQUIRE(workspace && workspace_bytes >= ssdk_integral_workspace_bytes(batch, num_anchors), SSDK_E_WORKSPACE,
                     "ssdk_integral_fwd: workspace too small");
    }
    hipStream_t s = (hipStream_t)stream;
    const long long n_rows = (long long)batch * num_anchors;
    const IntegralParams p = to_device(params);
    // LDS: every (row, side) slot that vec_steps * kIntThreads vectors can reach (the staging stores are unconditional)
    const size_t lds = align_up((size_t)(p.vec_steps * 4 * kIntThreads / p.bins + 2) * p.pitch * sizeof(float), 16);
    const void* fn = target ? (const void*)integral_fwd_kernel<true> : (const void*)integral_fwd_kernel<false>;
    const long long n_tiles = (n_rows + p.tile_rows - 1) / p.tile_rows;
    const int grid = (int)std::min<long long>(n_tiles, std::min(integral_resident_blocks(fn, lds), kIntMaxPartials));
    if (target) {
        IntegralWs w = carve_integral_ws(workspace, (size_t)n_rows, nullptr);
        hipLaunchKernelGGL(integral_fwd_kernel<true>, dim3(grid), dim3(kIntThreads), lds, s, p, (const float4*)logits, (const float4*)anchors, target,
                           n_rows, num_anchors, locs, w.y, w.partials, w.counts);
        SSDK_CHECK_LAUNCH("integral_fwd_kernel");
        hipLaunchKernelGGL(integral_finalize_kernel, dim3(1), dim3(256), 0, s, w.partials, w.counts, grid, p.weight, w.state, out2);
        SSDK_CHECK_LAUNCH("integral_finalize_kernel");
    } else {
        hipLaunchKernelGGL(integral_fwd_kernel<false>, dim3(grid), dim3(kIntThreads), lds, s, p, (const float4*)logits, (const float4*)nullptr,
                           (const float*)nullptr, n_rows, num_anchors, locs, (float*)nullptr, (float*)nullptr, (int*)nullptr);
        SSDK_CHECK_LAUNCH("integral_fwd_kernel");
    }
    return SSDK_OK;
}

extern "C" int ssdk_integral_bwd(const ssdk_integral_params* params, const float* logits, const float* dlocs, const float* target_classes,
                                 int class_stride, const float* grad_dfl, int batch, int num_anchors, float* dlogits, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    int rc = check_integral_params("ssdk_integral_bwd", params);
    if (rc) return rc;
    SSDK_REQUIRE(batch > 0 && num_anchors > 0, SSDK_E_INVALID, "ssdk_integral_bwd: batch=%d anchors=%d", batch, num_anchors);
    SSDK_REQUIRE(logits && dlogits, SSDK_E_INVALID, "ssdk_integral_bwd: null logits / dlogits");
    SSDK_REQUIRE(((uintptr_t)logits & 15) == 0 && ((uintptr_t)dlogits & 15) == 0, SSDK_E_INVALID,
                 "ssdk_integral_bwd: logits / dlogits must be 16-byte aligned");
    SSDK_REQUIRE(!target_classes || class_stride >= 1, SSDK_E_INVALID, "ssdk_integral_bwd: class_stride=%d", class_stride);
    SSDK_REQUIRE(!grad_dfl || target_classes, SSDK_E_INVALID, "ssdk_integral_bwd: a DFL gradient needs the target's class column");
    if (target_classes)
        SSDK_REQUIRE(workspace && workspace_bytes >= ssdk_integral_workspace_bytes(batch, num_anchors), SSDK_E_WORKSPACE,
                     "ssdk_integral_bwd: workspace too small");
    const long long n_rows = (long long)batch * num_anchors;
    const IntegralParams p = to_device(params);
    const size_t lds = align_up((size_t)p.tile_rows * 4 * p.pitch * sizeof(float), 16);
    const long long n_tiles = (n_rows + p.tile_rows - 1) / p.tile_rows;
    const int grid = (int)std::min<long long>(n_tiles, integral_resident_blocks((const void*)integral_bwd_kernel, lds));
    IntegralWs w = carve_integral_ws(target_classes ? workspace : nullptr, (size_t)n_rows, nullptr);
    hipLaunchKernelGGL(integral_bwd_kernel, dim3(grid), dim3(kIntThreads), lds, (hipStream_t)stream, p, (const float4*)logits, dlocs, target_classes,
                       class_stride, w.y, w.state, grad_dfl, n_rows, (float4*)dlogits);
    SSDK_CHECK_LAUNCH("integral_bwd_kernel");
    return SSDK_OK;
}
