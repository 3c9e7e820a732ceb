// match.hip -- IoU + matcher + target encoding, fused.
//
// Reference: detection/target_assigner.py:22-63 (python loop over images; per image a materialised [G,A] IoU
// matrix from bf/utils/box_utils.py:83-101 with ~10 [G,A,*] temporaries, then detection/matcher.py:33-56), all on
// the CPU because anchors live there -- 331 ms per SSD-300 batch of 32.
//
// Here nothing [G,A]-shaped exists.  Two launches over the whole batch:
//   1. gt_argmax_kernel   one workgroup per ground-truth box: it sweeps the anchors (16-byte coalesced loads,
//                         L2-resident: the anchor table is shared by every image) and reduces the box's best anchor as
//                         a 64-bit key (iou bits << 32 | ~anchor): argmax(dim=1) with torch's first-index tie rule
//                         (matcher.py:52).
//   2. assign_kernel      one thread per (image, anchor): re-derives the anchor's IoU with the image's boxes from
//                         LDS (cheaper than storing [G,A]), applies max(dim=0) with first-max ties, the two
//                         thresholds, then the force-match (last writer = highest box index wins, matcher.py:53-54),
//                         and writes the 24-byte target row through an LDS tile so HBM sees whole 8-byte lanes of a
//                         contiguous 6 KB block.  The target is written exactly once: B*A*24 bytes, the
//                         algorithmic minimum for this path.
// Opt-in (ssdk_encode_ground_truth_ex, SSDK_FORCE_MATCH_BIPARTITE): bipartite_resolve_kernel between the two, one workgroup per image,
// replaces the force-match rule by greedy bipartite matching (matcher.py:7-31); see further down.
// Beside it (ssdk_encode_ground_truth_atss; not in the reference): Adaptive Training Sample Selection, two launches of its own --
// atss_candidates_kernel (one workgroup per (box, level): the level's k nearest anchors as a cutoff key, their IoUs) and
// atss_assign_kernel (assign_kernel's shape with the box's own threshold in place of the two fixed ones); see further down.
// And ssdk_encode_ground_truth_tal (not in the reference either): Task Alignment Learning, three launches of its own -- tal_candidates_kernel (one
// workgroup per box: the topk inside anchors of largest s^alpha * u^beta, from the anchors' own predictions), tal_assign_kernel and
// tal_normalise_kernel (one wave per box: column 5 of the rows the box kept); see further down.
// And ssdk_encode_ground_truth_simota (not in the reference either): SimOTA, three launches of its own -- simota_class_sum_kernel (per region
// anchor the softplus sum of its logits, the class cost's per-anchor part), simota_candidates_kernel (one workgroup per box: the count k_g
// from its largest IoUs, then its k_g cheapest region anchors as a cutoff key) and simota_assign_kernel; see further down.
// The three later assigners share their building blocks, which stand in front of the kernels: the 64-bit keys, the
// four-in-flight anchor sweep, the two-keys-in-registers keeper, the workgroup's pop step with its advance, the chunk loop of the
// (image, anchor) kernels, the level table.  On the host one checker, one level-table builder and one carve function per assigner serve the
// ssdk_encode_ground_truth* entry points.
// IoU is computed op for op like the reference (this TU is built -ffp-contract=off, IEEE divide) so that
// assignments are bit-exact.
#include "common.h"

namespace ssdk {

constexpr int kAssignThreads = 256;
constexpr int kGtChunk = 128;
constexpr int kSegAnchors = 512;  // anchors swept by one wave of gt_argmax_kernel

// ---- what the assigners share -------------------------------------------------------------------------------------
// 64-bit keys: the value's order-preserving bits on top, below them ~index, so that the LARGER key is the larger value, then the lower index.
constexpr unsigned kOrdZero = 0x80000000u;  // ord_f32(0.0f)
__device__ __forceinline__ unsigned key_hi(unsigned long long k) { return (unsigned)(k >> 32); }
__device__ __forceinline__ int key_col(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)); }
__device__ __forceinline__ unsigned long long make_key(unsigned hi, int idx) { return ((unsigned long long)hi << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)idx); }
// Order-preserving bits of any float: -inf < ... < -0 == +0 < ... < +inf, all above 0; NaN -> 0, below everything (it never wins).
__device__ __forceinline__ unsigned ord_f32(float v) {
    if (v != v) return 0u;
    if (v == 0.0f) return kOrdZero;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
struct OpMinU64 {
    __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a < b ? a : b; }
};
// The two orders a workgroup pops keys in: which key comes first, and the key that comes after every real one.
template <typename Op> struct KeyOrder;
template <> struct KeyOrder<OpMinU64> {
    static constexpr unsigned long long none = ~0ull;
    static __device__ __forceinline__ bool before(unsigned long long a, unsigned long long b) { return a < b; }
};
template <> struct KeyOrder<OpMaxU64> {
    static constexpr unsigned long long none = 0ull;
    static __device__ __forceinline__ bool before(unsigned long long a, unsigned long long b) { return a > b; }
};

__device__ __forceinline__ float2 box_centre(float4 gb) { return make_float2((gb.x + gb.z) * 0.5f, (gb.y + gb.w) * 0.5f); }
__device__ __forceinline__ bool centre_inside(float4 gb, float4 p) { return gb.x < p.x && p.x < gb.z && gb.y < p.y && p.y < gb.w; }   // strictly
// column of the box's class in a row of logits, or -1 (the class is none of the columns: s = 0)
__device__ __forceinline__ int class_column(float cls, int C) { return (cls >= 1.0f && cls <= (float)C) ? (int)cls - 1 : -1; }
// image of row g (< gt_off[batch]): the last i with gt_off[i] <= g
__device__ __forceinline__ int image_of_row(const int32_t* __restrict__ gt_off, int batch, int g) {
    int lo = 0, hi = batch - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gt_off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// Pyramid levels by value (no table to upload): level l owns anchors [off[l], off[l + 1]); the entries past n repeat the total.
struct Levels { int n; int off[SSDK_ATSS_MAX_LEVELS + 1]; };

// The workgroup's kThreads threads sweep anchors [a_begin, a_end) with four 16-byte loads in flight; `take(a, p)` sees a thread's anchors
// in ascending order.
template <int kThreads, typename Take>
__device__ __forceinline__ void sweep_anchors(const float4* __restrict__ anchors, int a_begin, int a_end, const Take& take) {
    int a = a_begin + threadIdx.x;
    for (; a + 3 * kThreads < a_end; a += 4 * kThreads) {
        const float4 p0 = anchors[a], p1 = anchors[a + kThreads], p2 = anchors[a + 2 * kThreads], p3 = anchors[a + 3 * kThreads];
        take(a, p0);
        take(a + kThreads, p1);
        take(a + 2 * kThreads, p2);
        take(a + 3 * kThreads, p3);
    }
    for (; a < a_end; a += kThreads) take(a, anchors[a]);
}
// A thread's two first keys of a sweep stay in registers (selects: the branchy form made the compiler keep k1 and k2 in scratch).  Its
// anchors are kThreads apart, the anchors of one cell and of neighbouring cells are not, so a thread almost never owns more than one of a
// box's candidates.
template <typename Op>
__device__ __forceinline__ void keep_two(unsigned long long k, unsigned long long& k1, unsigned long long& k2) {
    const bool b1 = KeyOrder<Op>::before(k, k1), b2 = KeyOrder<Op>::before(k, k2);
    k2 = b1 ? k1 : (b2 ? k : k2);
    k1 = b1 ? k : k1;
}
// First key of the workgroup, returned to every thread: `red` = LDS [kThreads / kWave], one barrier; `red` is read after it, so the next
// call needs another array (or a barrier in between).
template <typename Op, int kThreads>
__device__ __forceinline__ unsigned long long block_first(unsigned long long k, unsigned long long* red) {
    k = wave_allreduce(k, Op());
    if (lane_id() == 0) red[threadIdx.x >> 6] = k;
    __syncthreads();
    unsigned long long r = red[0];
#pragma unroll
    for (int q = 1; q < kThreads / kWave; ++q) r = Op()(red[q], r);
    return r;
}
// One pop of the workgroup's first remaining key (`cur`: the thread's), one barrier: the two halves of s_red alternate with `step`, which
// counts EVERY pop of the kernel.
template <typename Op, int kThreads>
__device__ __forceinline__ unsigned long long pop_first(unsigned long long cur, unsigned long long (*s_red)[kThreads / kWave], int step) {
    return block_first<Op, kThreads>(cur, s_red[step & 1]);
}
// After a pop: the owner of the popped key moves on to its second key (k1, k2: keep_two's); only a thread that loses both calls `rescan`,
// which re-reads its own anchors for the next key behind the popped one (next_key_behind).
template <typename Rescan>
__device__ __forceinline__ void pop_advance(unsigned long long popped, unsigned long long& cur, unsigned long long k1, unsigned long long k2, Rescan rescan) {
    if (cur == popped) cur = cur == k1 ? k2 : rescan();   // (k2 is `none` when the thread swept a single key: it has nothing left)
}
template <typename Op, int kThreads, typename KeyOf>
__device__ __forceinline__ unsigned long long next_key_behind(unsigned long long popped, int a_begin, int a_end, KeyOf key_of) {
    unsigned long long cur = KeyOrder<Op>::none;
    for (int b = a_begin + threadIdx.x; b < a_end; b += kThreads) {
        const unsigned long long k = key_of(b);   // (`none` for an anchor without a key)
        if (KeyOrder<Op>::before(popped, k) && KeyOrder<Op>::before(k, cur)) cur = k;
    }
    return cur;
}
// One thread per (image, anchor): the image's G boxes pass through the kernel's own LDS arrays in chunks of kGtChunk.  `load(k, j)` puts box
// k of the image into slot j (one thread per box); `visit(base, n)` then sees boxes base .. base + n - 1 in slots 0 .. n - 1.
template <typename Load, typename Visit>
__device__ __forceinline__ void for_box_chunks(int G, const Load& load, const Visit& visit) {
    for (int base = 0; base < G; base += kGtChunk) {
        const int n = min(kGtChunk, G - base);
        __syncthreads();
        if (threadIdx.x < n) load(base + (int)threadIdx.x, (int)threadIdx.x);
        __syncthreads();
        visit(base, n);
    }
}

// One workgroup per ground-truth box: its 1 024 threads sweep ALL anchors and the result is stored, not accumulated -- no atomics and
// therefore no zero-fill launch in front (the first version folded (box, 512-anchor segment) partial results into a zeroed array with
// atomicMax: a third launch, and a memset node costs as much as a small kernel).
constexpr int kArgmaxThreads = 1024;   // (a box's sweep is a chain of dependent L2 round trips per thread: 8 anchors per thread at A = 8 108, not 32)
// Round 5: large anchor sets (RetinaNet: 47 961 -- 47 anchors per thread, 21 us for 144 boxes on 144 CUs) are swept by `segs` workgroups
// per box, each STORING the key of its anchor range (gt_best[g * segs + seg]); assign_kernel takes the maximum of a box's keys when it
// loads the box -- still no atomics and nothing to zero, and the same key as one sweep would produce (largest IoU, then smallest anchor).
constexpr int kArgmaxMaxSegs = 8;
static inline int argmax_segs(int A) { const int s = (A + kArgmaxThreads * 12 - 1) / (kArgmaxThreads * 12); return s < 1 ? 1 : (s > kArgmaxMaxSegs ? kArgmaxMaxSegs : s); }
__global__ void __launch_bounds__(kArgmaxThreads) gt_argmax_kernel(const float* __restrict__ gt_rows, int gt_stride,
                                                                   const float4* __restrict__ anchors, int A_all,
                                                                   unsigned long long* __restrict__ gt_best, const int32_t* __restrict__ gt_off,
                                                                   int batch) {
    __shared__ unsigned long long s_key[kArgmaxThreads / kWave];
    const int g = blockIdx.x;
    if (g >= gt_off[batch]) return;   // (a row buffer of fixed capacity, e.g. inside a captured HIP graph: rows past the last image's are padding)
    const int segs = gridDim.y, seg = blockIdx.y;
    const int seg_len = (A_all + segs - 1) / segs;
    const int a_begin = seg * seg_len, A = min(A_all, a_begin + seg_len);   // this workgroup's anchors: [a_begin, A)
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const float* r = gt_rows + (size_t)g * gt_stride;
    const float4 gb = make_float4(r[0], r[1], r[2], r[3]);
    const float garea = area4(gb.x, gb.y, gb.z, gb.w);
    float best = 0.0f;
    int bi = -1;
    auto take = [&](int a, const float4& p) {
        const float4 c = to_corners(p);
        const float v = iou_corner(gb, garea, c, area4(c.x, c.y, c.z, c.w));
        if (bi < 0 || v > best || (v != v && best == best)) { best = v; bi = a; }
    };
    // sweep_anchors spelled out (this kernel is on the training step's path, and through the helper its code came out different): taken in
    // ascending anchor order, first-index ties
    int a = a_begin + threadIdx.x;
    for (; a + 3 * kArgmaxThreads < A; a += 4 * kArgmaxThreads) {
        const float4 p0 = anchors[a], p1 = anchors[a + kArgmaxThreads], p2 = anchors[a + 2 * kArgmaxThreads], p3 = anchors[a + 3 * kArgmaxThreads];
        take(a, p0);
        take(a + kArgmaxThreads, p1);
        take(a + 2 * kArgmaxThreads, p2);
        take(a + 3 * kArgmaxThreads, p3);
    }
    for (; a < A; a += kArgmaxThreads) take(a, anchors[a]);
    unsigned long long key = 0ull;
    if (bi >= 0) key = make_key(__float_as_uint(best), bi);
    key = wave_allreduce(key, OpMaxU64());
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    if (threadIdx.x < kWave) {
        unsigned long long k = threadIdx.x < kArgmaxThreads / kWave ? s_key[threadIdx.x] : 0ull;
        k = wave_allreduce(k, OpMaxU64());
        if (threadIdx.x == 0) gt_best[(size_t)g * segs + seg] = k;
    }
}

// The end of both assign kernels: the thread's target row (box `bi` of the image whose rows start at g0, or the background / ignore row)
// goes to the LDS tile `s_out` [kAssignThreads * 6], then the block's rows leave as one contiguous run of 8-byte lanes.
__device__ __forceinline__ void write_target_rows(const float* __restrict__ gt_rows, int gt_stride, int g0, int bi, int i, int a0, int A,
                                                  float* s_out, float* __restrict__ target, int32_t* __restrict__ box_idx) {
    const int a = a0 + threadIdx.x;
    float* o = s_out + threadIdx.x * 6;
    if (bi >= 0) {  // target_assigner.py:52-54
        const float* r = gt_rows + (size_t)(g0 + bi) * gt_stride;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; o[4] = r[4]; o[5] = r[5];
    } else {
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f;
        o[4] = bi == SSDK_IGNORE ? -1.0f : 0.0f;  // :56-58 / :39
        o[5] = bi == SSDK_IGNORE ? -1.0f : 1.0f;  // :40
    }
    if (box_idx && a < A) box_idx[(size_t)i * A + a] = bi;
    __syncthreads();
    // 24-byte rows of this block are one contiguous run in HBM; (i*A + a0)*24 is always 8-byte aligned.
    const int rows = min(kAssignThreads, A - a0);
    float2* dst = reinterpret_cast<float2*>(target + ((size_t)i * A + a0) * 6);
    const float2* src = reinterpret_cast<const float2*>(s_out);
    for (int t = threadIdx.x; t < rows * 3; t += kAssignThreads) dst[t] = src[t];
}

__global__ void __launch_bounds__(kAssignThreads) assign_kernel(const float* __restrict__ gt_rows, int gt_stride,
                                                                const int32_t* __restrict__ gt_off,
                                                                const float4* __restrict__ anchors, int A, float matched_thr,
                                                                float unmatched_thr,
                                                                const unsigned long long* __restrict__ gt_best, int segs,
                                                                float* __restrict__ target, int32_t* __restrict__ box_idx) {
    __shared__ float4 s_box[kGtChunk];
    __shared__ float s_area[kGtChunk];
    __shared__ int s_best_anchor[kGtChunk];
    __shared__ __attribute__((aligned(16))) float s_out[kAssignThreads * 6];

    const int i = blockIdx.y;
    const int a0 = blockIdx.x * kAssignThreads;
    const int a = a0 + threadIdx.x;
    const int g0 = gt_off[i], G = gt_off[i + 1] - g0;

    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float carea = 0.f;
    if (a < A) {
        c = to_corners(anchors[a]);
        carea = area4(c.x, c.y, c.z, c.w);
    }
    float best = 0.0f;
    int bi = SSDK_NOT_MATCHED, forced = -1;
    for (int base = 0; base < G; base += kGtChunk) {   // for_box_chunks spelled out (on the training step's path, as gt_argmax_kernel)
        const int n = min(kGtChunk, G - base);
        __syncthreads();
        if (threadIdx.x < n) {
            const int g = g0 + base + threadIdx.x;
            const float* r = gt_rows + (size_t)g * gt_stride;
            const float4 gb = make_float4(r[0], r[1], r[2], r[3]);
            s_box[threadIdx.x] = gb;
            s_area[threadIdx.x] = area4(gb.x, gb.y, gb.z, gb.w);
            unsigned long long key = gt_best[(size_t)g * segs];
            for (int q = 1; q < segs; ++q) { const unsigned long long k2 = gt_best[(size_t)g * segs + q]; key = k2 > key ? k2 : key; }
            s_best_anchor[threadIdx.x] = key_col(key);
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const float v = iou_corner(s_box[k], s_area[k], c, carea);
            if ((base + k) == 0 || v > best || (v != v && best == best)) { best = v; bi = base + k; }  // max(dim=0)
            if (s_best_anchor[k] == a) forced = base + k;  // ascending k: the highest box index wins
        }
    }
    if (G > 0) {  // matcher.py:45-50
        if (best < unmatched_thr) bi = SSDK_NOT_MATCHED;
        else if (best < matched_thr) bi = SSDK_IGNORE;
        if (forced >= 0) bi = forced;
    }
    write_target_rows(gt_rows, gt_stride, g0, bi, i, a0, A, s_out, target, box_idx);
}

// ---- detection/matcher.py:33-56 on a materialised weight matrix [G, A] (the API the reference exposes; the training path uses the
// fused kernels above and never stores such a matrix) ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) mpp_row_argmax_kernel(const float* __restrict__ w, int A, unsigned long long* __restrict__ best) {
    const int g = blockIdx.y;
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = lane_id();
    const int a0 = seg * kSegAnchors;
    if (a0 >= A) return;
    const int a1 = min(A, a0 + kSegAnchors);
    const float* row = w + (size_t)g * A;
    float bv = 0.0f;
    int bi = -1;
    for (int a = a0 + lane; a < a1; a += kWave) {   // weights.argmax(dim=1): first maximum, NaN counts as the largest (matcher.py:52)
        const float v = row[a];
        if (bi < 0 || v > bv || (v != v && bv == bv)) { bv = v; bi = a; }
    }
    unsigned long long key = 0ull;
    if (bi >= 0) {
        // order-preserving bits for any sign: flip all bits of negatives, set the sign bit of the others; NaN above everything
        unsigned u = __float_as_uint(bv);
        u = (bv != bv) ? 0xFFFFFFFFu : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
        key = ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)bi);
    }
    key = wave_allreduce(key, OpMaxU64());
    if (lane == 0 && key) atomicMax(best + g, key);
}

__global__ void __launch_bounds__(kAssignThreads) mpp_assign_kernel(const float* __restrict__ w, int G, int A, float matched_thr, float unmatched_thr,
                                                                    int force, const unsigned long long* __restrict__ best,
                                                                    long long* __restrict__ box_idx) {
    __shared__ int s_best_anchor[kGtChunk];
    const int a = blockIdx.x * kAssignThreads + threadIdx.x;
    float bv = 0.0f;
    int bi = 0, forced = -1;
    for (int base = 0; base < G; base += kGtChunk) {
        const int n = min(kGtChunk, G - base);
        __syncthreads();
        if (threadIdx.x < n) s_best_anchor[threadIdx.x] = force ? (int)(0xFFFFFFFFu - (unsigned)(best[base + threadIdx.x] & 0xFFFFFFFFull)) : -1;
        __syncthreads();
        if (a < A)
            for (int k = 0; k < n; ++k) {
                const float v = w[(size_t)(base + k) * A + a];
                if ((base + k) == 0 || v > bv || (v != v && bv == bv)) { bv = v; bi = base + k; }   // weights.max(dim=0), :45
                if (s_best_anchor[k] == a) forced = base + k;                                            // :52-54, the highest box index wins
            }
    }
    if (a >= A) return;
    if (bv < unmatched_thr) bi = SSDK_NOT_MATCHED;        // :49
    else if (bv < matched_thr) bi = SSDK_IGNORE;          // :50
    if (forced >= 0) bi = forced;
    box_idx[a] = bi;
}


// ---- detection/matcher.py:7-31 match_bipartite --------------------------------------------------------------------------------------
// Greedy bipartite matching: repeat { argmax of the whole matrix; that row gets that column; zero the column and the row }.  Both forms
// below keep ONE 64-bit key per box -- its best remaining (value, ~column) -- and redo a box's row only when its column was just taken,
// so a round costs one reduction over the boxes plus the rescans of the boxes that collided.  One workgroup owns a whole problem (an
// image, or the matrix): no workgroup waits on another, every loop is counted by G or A, and a NaN never wins a comparison.
constexpr int kBipThreads = 1024;
constexpr int kBipWaves = kBipThreads / kWave;
constexpr int kBipLdsBoxes = 1024;        // per image: more boxes than this keep their keys in the workspace instead of LDS (same code, flat pointers)
constexpr int kBipMaxAnchors = 262144;    // the taken-column bit mask of the fused form is 32 KB of LDS

// Maximum of a key over the workgroup, returned to every thread.  `red` = LDS [kBipWaves]; two barriers, `red` is free again afterwards.
__device__ __forceinline__ unsigned long long bip_block_max(unsigned long long k, unsigned long long* red) {
    const unsigned long long r = block_first<OpMaxU64, kBipThreads>(k, red);
    __syncthreads();
    return r;
}
// The workgroup rescans n rows (rows[j], or j itself when rows == NULL): `sweep(row)` is every thread's best key over its share of the
// row's columns; the row's key (largest value, then lowest column) goes to keys[row].  Rows go in batches of kBipWaves with two barriers
// per batch: each wave leaves its partial key per row in LDS, then wave j folds row j's partials.
template <typename Sweep>
__device__ __forceinline__ void bip_rescan(const int* rows, int n, unsigned long long* keys, unsigned long long (*part)[kBipWaves], Sweep sweep) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (int base = 0; base < n; base += kBipWaves) {
        const int m = min(kBipWaves, n - base);
        for (int j = 0; j < m; ++j) {
            const int r = rows ? rows[base + j] : base + j;
            const unsigned long long k = wave_allreduce(sweep(r), OpMaxU64());
            if (lane == 0) part[j][wave] = k;
        }
        __syncthreads();
        if (wave < m) {
            unsigned long long k = lane < kBipWaves ? part[wave][lane] : 0ull;
            k = wave_allreduce(k, OpMaxU64());
            if (lane == 0) keys[rows ? rows[base + wave] : base + wave] = k;
        }
        __syncthreads();
    }
}

// Fused form (the force stage of TargetAssigner(force_match='bipartite')): one workgroup per image, between gt_argmax_kernel and
// assign_kernel.  It takes every box's best (iou, ~anchor) key from gt_best, resolves the collisions and writes the result back in key
// form into gt_best[g * segs + 0] (the other segments' slots and the boxes without a forced anchor: 0, which decodes to anchor -1), so
// assign_kernel runs unchanged.  A rescan recomputes the box's IoUs exactly as gt_argmax_kernel does, skipping the taken anchors.  The
// stage ends at the first maximum that is not above 0 (NaN counts as not above 0): the boxes left over get no forced anchor.
__global__ void __launch_bounds__(kBipThreads) bipartite_resolve_kernel(const float* __restrict__ gt_rows, int gt_stride, const int32_t* __restrict__ gt_off,
                                                                        const float4* __restrict__ anchors, int A, unsigned long long* gt_best, int segs,
                                                                        unsigned long long* spill_keys, int* spill_rows) {
    __shared__ unsigned long long s_key[kBipLdsBoxes];
    __shared__ int s_rows[kBipLdsBoxes];
    __shared__ unsigned s_taken[kBipMaxAnchors / 32];
    __shared__ unsigned long long s_red[kBipWaves];
    __shared__ unsigned long long s_part[kBipWaves][kBipWaves];
    __shared__ int s_n;
    const int i = blockIdx.x;
    const int g0 = gt_off[i], G = gt_off[i + 1] - g0;
    if (G <= 0) return;
    unsigned long long* keys = G <= kBipLdsBoxes ? s_key : spill_keys + g0;
    int* rows = G <= kBipLdsBoxes ? s_rows : spill_rows + g0;
    for (int w = threadIdx.x; w < (A + 31) / 32; w += kBipThreads) s_taken[w] = 0u;
    for (int r = threadIdx.x; r < G; r += kBipThreads) {
        unsigned long long* slot = gt_best + (size_t)(g0 + r) * segs;
        unsigned long long key = slot[0];
        slot[0] = 0ull;
        for (int q = 1; q < segs; ++q) { const unsigned long long k2 = slot[q]; key = k2 > key ? k2 : key; slot[q] = 0ull; }
        keys[r] = __uint_as_float(key_hi(key)) > 0.0f ? key : 0ull;   // (an IoU of 0 or NaN: nothing to force)
    }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (int it = 0; it < G; ++it) {
        unsigned long long k = 0ull;
        for (int r = threadIdx.x; r < G; r += kBipThreads) {   // largest IoU among the unassigned boxes, then the lowest box index
            const unsigned hi = key_hi(keys[r]);
            if (hi) { const unsigned long long c = make_key(hi, r); k = c > k ? c : k; }
        }
        k = bip_block_max(k, s_red);
        if (key_hi(k) == 0u) break;   // (the same value in every thread) every anchor the remaining boxes overlap is taken
        const int rs = key_col(k);
        const unsigned long long kstar = keys[rs];
        const int cs = key_col(kstar);
        for (int r = threadIdx.x; r < G; r += kBipThreads) {
            const unsigned long long kr = keys[r];
            if (r != rs && key_hi(kr) && key_col(kr) == cs) rows[atomicAdd(&s_n, 1)] = r;
        }
        __syncthreads();
        const int n = s_n;
        if (threadIdx.x == 0) {
            keys[rs] = 0ull;
            s_taken[cs >> 5] |= 1u << (cs & 31);
            gt_best[(size_t)(g0 + rs) * segs] = kstar;
        }
        __syncthreads();
        if (threadIdx.x == 0) s_n = 0;   // (the next append is behind bip_block_max's barriers)
        bip_rescan(rows, n, keys, s_part, [&](int r) {
            const float* b = gt_rows + (size_t)(g0 + r) * gt_stride;
            const float4 gb = make_float4(b[0], b[1], b[2], b[3]);
            const float garea = area4(gb.x, gb.y, gb.z, gb.w);
            unsigned bu = 0u;
            int bi = 0;
            for (int a = threadIdx.x; a < A; a += kBipThreads) {   // ascending anchors, strict >: the first maximum
                const float4 c = to_corners(anchors[a]);
                const float v = iou_corner(gb, garea, c, area4(c.x, c.y, c.z, c.w));
                const bool taken = (s_taken[a >> 5] >> (a & 31)) & 1u;
                const unsigned u = (!taken && v > 0.0f) ? __float_as_uint(v) : 0u;
                if (u > bu) { bu = u; bi = a; }
            }
            return bu ? make_key(bu, bi) : 0ull;
        });
    }
}

// Matrix form: ONE workgroup plays the reference's loop on the working matrix `w` (the caller's for inplace, else a copy in the
// workspace) literally -- G rounds, each zeroing a column and a row in memory -- so the matrix it leaves, and what exhaustion does
// (every later round lands on flat index 0), are the reference's.  keys[r] is always the (ord(value), ~column) of row r's first maximum
// in the CURRENT matrix, assigned (all-zero) rows included: zeroing column c can only matter to a row whose maximum sat in c (rescan)
// or whose maximum is <= 0 (the new 0 at c may now be its first maximum).
__global__ void __launch_bounds__(kBipThreads) match_bipartite_kernel(float* w, int G, int A, long long* __restrict__ anchor_idx,
                                                                      int* __restrict__ num_matched, unsigned long long* keys, int* rows) {
    __shared__ unsigned long long s_red[kBipWaves];
    __shared__ unsigned long long s_part[kBipWaves][kBipWaves];
    __shared__ int s_n;
    auto sweep = [&](int r) {
        const float* row = w + (size_t)r * A;
        unsigned bu = 0u;
        int bi = 0;
        for (int a = threadIdx.x; a < A; a += kBipThreads) {
            const unsigned u = ord_f32(row[a]);
            if (u > bu) { bu = u; bi = a; }
        }
        return make_key(bu, bi);   // (a row of NaNs only: column 0)
    };
    for (int r = threadIdx.x; r < G; r += kBipThreads) anchor_idx[r] = -1;
    if (threadIdx.x == 0) s_n = 0;
    bip_rescan(nullptr, G, keys, s_part, sweep);
    int matched = 0;
    for (int it = 0; it < G; ++it) {
        unsigned long long k = 0ull;
        for (int r = threadIdx.x; r < G; r += kBipThreads) { const unsigned long long c = make_key(key_hi(keys[r]), r); k = c > k ? c : k; }
        k = bip_block_max(k, s_red);   // the largest value, then the lowest row; its key holds the lowest column: the first flat index
        const int rs = key_col(k);
        const unsigned long long kstar = keys[rs];
        const int cs = key_col(kstar);
        for (int r = threadIdx.x; r < G; r += kBipThreads) {
            if (r == rs) continue;
            const unsigned long long kr = keys[r];
            const int col = key_col(kr);
            if (col == cs) { if (key_hi(kr) != kOrdZero) rows[atomicAdd(&s_n, 1)] = r; }   // (a maximum of 0 at cs stays where it is)
            else if (kOrdZero > key_hi(kr) || (kOrdZero == key_hi(kr) && cs < col)) keys[r] = make_key(kOrdZero, cs);
            w[(size_t)r * A + cs] = 0.0f;          // weights[:, idx % num_priors] = 0
        }
        for (int a = threadIdx.x; a < A; a += kBipThreads) w[(size_t)rs * A + a] = 0.0f;   // weights[idx // num_priors] = 0
        __syncthreads();
        const int n = s_n;
        if (threadIdx.x == 0) {
            keys[rs] = make_key(kOrdZero, 0);
            anchor_idx[rs] = cs;
            matched += key_hi(kstar) > kOrdZero;
        }
        __syncthreads();
        if (threadIdx.x == 0) s_n = 0;
        bip_rescan(rows, n, keys, s_part, sweep);
    }
    if (threadIdx.x == 0) *num_matched = matched;
}

__global__ void __launch_bounds__(256) copy_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// ---- Adaptive Training Sample Selection (arXiv:1912.02424, Algorithm 1; not in the reference) ------------------------------------------
// Per box: the min(k, n_l) anchors of every pyramid level nearest to the box centre are its candidates; mean + unbiased standard deviation
// of their IoUs (fp64, two passes) is the box's own threshold t_g; a candidate whose IoU reaches t_g and whose centre lies strictly inside
// the box is positive; an anchor positive for several boxes takes the largest IoU, then the lowest box index.  No ignore band, no force
// stage.  Two launches, nothing [G, A]-shaped, no atomics, nothing zero-filled, every sum in a fixed order:
//   1. atss_candidates_kernel  one workgroup per (box, level): ONE sweep of the level's anchors (16-byte loads), every anchor a 64-bit key
//                              (centre-distance bits << 32 | anchor), smaller = nearer, ties to the lower anchor, a NaN distance last.
//                              The workgroup pops its kk = min(k, n_l) smallest keys and stores the LAST one -- the level's cutoff key --
//                              and the kk candidates' IoUs.  No candidate list leaves the kernel.
//   2. atss_assign_kernel      one thread per (image, anchor), on the pattern of assign_kernel: it re-derives its key against each box of
//                              the image and is that box's candidate exactly when key <= cutoff(box, its level).  The thread that loads
//                              a box into LDS finishes t_g from the stored candidate IoUs (level order, then rank order).
constexpr int kAtssThreads = 1024;
constexpr int kAtssWaves = kAtssThreads / kWave;
constexpr unsigned long long kAtssNoKey = ~0ull;   // above every key (an anchor index is below 2^31)

// An anchor's key against a box centre gc = box_centre(gb): two subtractions, two products, one add, all fp32 and uncontracted.  The sum of
// two squares is never negative, so its bits order like the value; NaN goes above +inf.
__device__ __forceinline__ unsigned long long atss_key(float4 p, float2 gc, int a) {
    const float dx = p.x - gc.x, dy = p.y - gc.y;
    const float d2 = dx * dx + dy * dy;
    const unsigned u = (d2 != d2) ? 0xFFFFFFFFu : __float_as_uint(d2);
    return ((unsigned long long)u << 32) | (unsigned long long)(unsigned)a;
}

__global__ void __launch_bounds__(kAtssThreads) atss_candidates_kernel(const float* __restrict__ gt_rows, int gt_stride, const int32_t* __restrict__ gt_off,
                                                                       int batch, const float4* __restrict__ anchors, Levels lv, int topk,
                                                                       unsigned long long* __restrict__ cutoff, float* __restrict__ cand_iou) {
    __shared__ unsigned long long s_red[2][kAtssWaves];
    const int g = blockIdx.x, l = blockIdx.y;
    if (g >= gt_off[batch]) return;   // rows past the last image's are padding (a row buffer of fixed capacity)
    int a_begin = 0, a_end = 0;
#pragma unroll
    for (int q = 0; q < SSDK_ATSS_MAX_LEVELS; ++q)   // (constant indices: a by-value table indexed by a variable would be copied to scratch)
        if (q == l) { a_begin = lv.off[q]; a_end = lv.off[q + 1]; }
    const int kk = min(topk, a_end - a_begin);
    const float* r = gt_rows + (size_t)g * gt_stride;
    const float4 gb = make_float4(r[0], r[1], r[2], r[3]);
    const float2 gc = box_centre(gb);
    unsigned long long k1 = kAtssNoKey, k2 = kAtssNoKey;   // the thread's two smallest keys
    sweep_anchors<kAtssThreads>(anchors, a_begin, a_end, [&](int a, const float4& p) { keep_two<OpMinU64>(atss_key(p, gc, a), k1, k2); });
    // kk pops of the workgroup's smallest remaining key.
    unsigned long long cur = k1, mine = kAtssNoKey, popped = 0ull;
    for (int j = 0; j < kk; ++j) {
        popped = pop_first<OpMinU64, kAtssThreads>(cur, s_red, j);
        if (threadIdx.x == j) mine = popped;   // (kk <= 32: thread j keeps the j-th candidate)
        pop_advance(popped, cur, k1, k2, [&] {
            return next_key_behind<OpMinU64, kAtssThreads>(popped, a_begin, a_end, [&](int b) { return atss_key(anchors[b], gc, b); });
        });
    }
    if (threadIdx.x < kk) {   // rule 3's v_i, the IoU assign_kernel computes, in rank order
        const float4 c = to_corners(anchors[min((unsigned)(mine & 0xFFFFFFFFull), (unsigned)(a_end - 1))]);   // (a popped key is always an anchor of the level; the clamp costs nothing)
        cand_iou[((size_t)g * lv.n + l) * SSDK_ATSS_MAX_TOPK + threadIdx.x] = iou_corner(gb, area4(gb.x, gb.y, gb.z, gb.w), c, area4(c.x, c.y, c.z, c.w));
    }
    if (threadIdx.x == 0) cutoff[(size_t)g * lv.n + l] = popped;
}

__global__ void __launch_bounds__(kAssignThreads) atss_assign_kernel(const float* __restrict__ gt_rows, int gt_stride, const int32_t* __restrict__ gt_off,
                                                                     const float4* __restrict__ anchors, int A, Levels lv, int topk,
                                                                     const unsigned long long* __restrict__ cutoff, const float* __restrict__ cand_iou,
                                                                     float* __restrict__ target, int32_t* __restrict__ box_idx) {
    __shared__ float4 s_box[kGtChunk];
    __shared__ float s_area[kGtChunk];
    __shared__ float2 s_centre[kGtChunk];
    __shared__ float s_thr[kGtChunk];
    __shared__ unsigned long long s_cut[kGtChunk * SSDK_ATSS_MAX_LEVELS];
    __shared__ __attribute__((aligned(16))) float s_out[kAssignThreads * 6];

    const int i = blockIdx.y;
    const int a0 = blockIdx.x * kAssignThreads;
    const int a = a0 + threadIdx.x;
    const int g0 = gt_off[i], G = gt_off[i + 1] - g0;
    const int L = lv.n;

    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), c = p;
    float carea = 0.f;
    int l = 0;
    if (a < A) {
        p = anchors[a];
        c = to_corners(p);
        carea = area4(c.x, c.y, c.z, c.w);
        while (l + 1 < L && a >= lv.off[l + 1]) ++l;
    }
    float best = 0.0f;
    int bi = SSDK_NOT_MATCHED;
    // for_box_chunks spelled out: beside the one-thread-per-box load, ALL threads of the block copy the chunk's n * L cutoffs together
    // between the two barriers, which the helper's load functor has no place for.
    for (int base = 0; base < G; base += kGtChunk) {
        const int n = min(kGtChunk, G - base);
        __syncthreads();
        if (threadIdx.x < n) {
            const int j = threadIdx.x, g = g0 + base + j;
            const float* r = gt_rows + (size_t)g * gt_stride;
            const float4 gb = make_float4(r[0], r[1], r[2], r[3]);
            s_box[j] = gb;
            s_area[j] = area4(gb.x, gb.y, gb.z, gb.w);
            s_centre[j] = box_centre(gb);
            // t_g: fp64, two passes over the box's candidates in (level, rank) order -- the same order in every workgroup
            const float* v = cand_iou + (size_t)g * L * SSDK_ATSS_MAX_TOPK;
            double sum = 0.0;
            int cnt = 0;
            for (int q = 0; q < L; ++q) {
                const int kk = min(topk, lv.off[q + 1] - lv.off[q]);
                for (int t = 0; t < kk; ++t) sum += (double)v[q * SSDK_ATSS_MAX_TOPK + t];
                cnt += kk;
            }
            const double mean = sum / (double)cnt;
            double dev = 0.0;
            for (int q = 0; q < L; ++q) {
                const int kk = min(topk, lv.off[q + 1] - lv.off[q]);
                for (int t = 0; t < kk; ++t) { const double d = (double)v[q * SSDK_ATSS_MAX_TOPK + t] - mean; dev += d * d; }
            }
            s_thr[j] = (float)(mean + (cnt > 1 ? sqrt(dev / (double)(cnt - 1)) : 0.0));
        }
        for (int t = threadIdx.x; t < n * L; t += kAssignThreads) s_cut[t] = cutoff[(size_t)(g0 + base) * L + t];
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            if (atss_key(p, s_centre[k], a) > s_cut[k * L + l]) continue;   // not among the box's nearest on this level
            const float4 gb = s_box[k];
            const float v = iou_corner(gb, s_area[k], c, carea);
            if (centre_inside(gb, p) && v >= s_thr[k] && (bi < 0 || v > best)) { best = v; bi = base + k; }   // ascending k, strict >: the lowest box index keeps a tie
        }
    }
    write_target_rows(gt_rows, gt_stride, g0, bi, i, a0, A, s_out, target, box_idx);
}

// ---- Task Alignment Learning (TOOD, arXiv:2108.07755 section 3.2; not in the reference) ---------------------------------------------------
// Per box: among the anchors whose centre lies strictly inside it, the topk of largest m = s^alpha * u^beta are its candidates -- s the
// anchor's own predicted probability of the box's class, u the IoU of the anchor's own decoded box with it; an anchor that is a candidate
// of several boxes goes to the largest u, then the lowest box index; column 5 of a kept anchor is score * m / (m_max + 1e-9) * u_max over
// the anchors the box kept (include/ssdk.h has the rule operation by operation).  Three launches, nothing [G, A]-shaped, no atomics,
// nothing zero-filled by a launch of its own:
//   1. tal_candidates_kernel  one workgroup per box: ONE sweep of the anchor table (16-byte loads), the inside test first; only an inside
//                             anchor loads its 16-byte loc and the one logit of the box's class and becomes the key
//                             (ord_f32(m) << 32 | ~a), larger = better, ties to the lower anchor.  The workgroup pops its kk =
//                             min(topk, #inside) largest keys and stores the LAST one -- the box's cutoff key -- and the kk candidates
//                             (anchor, m, u) in rank order, each with a `kept` flag of 0.
//   2. tal_assign_kernel      one thread per (image, anchor), on the pattern of atss_assign_kernel: it decodes its own box once, recomputes
//                             its key against each box that holds its centre with the SAME device functions (the bits are launch 1's) and
//                             is a candidate exactly when key >= cutoff(box).  The winner's row leaves through write_target_rows with the
//                             box's score in column 5, and the thread raises its `kept` flag in the winner's candidate list.
//   3. tal_normalise_kernel   one wave per box: m_max and u_max over the box's kept candidates, then column 5 of their rows.  It touches
//                             total_gt * topk elements, not A.
// (The kept flag, not box_idx, tells launch 3 which candidates a box kept: box_idx is optional, and a workspace sized without the anchor
// count has no room for a private copy.  The flag is written by launch 1 and raised by exactly one thread of launch 2: no zero-fill.)
constexpr int kTalThreads = 1024;
constexpr int kTalWaves = kTalThreads / kWave;
constexpr int kTalNormThreads = 256;
constexpr unsigned long long kTalNoCutoff = ~0ull;   // above every key: a box without an inside anchor has no candidate
struct TalParams { float xy_scale, wh_scale, alpha, beta; int C; };

// x^e for x >= 0, e >= 0 (rule 5): 0, 1, 2 -- and 6 where `six` allows it, the default beta -- are multiplies, the rest one __powf
__device__ __forceinline__ float tal_pow(float x, float e, bool six) {
    if (e == 0.0f) return 1.0f;
    if (e == 1.0f) return x;
    if (e == 2.0f) return x * x;
    if (six && e == 6.0f) { const float x2 = x * x; return x2 * x2 * x2; }
    return __powf(x, e);
}
// rules 1 - 3 and 5 for one (anchor, box): P the anchor's decoded corners, gb the box's, x the logit of the box's class (has_class: the class
// is one of the columns).  Both launches call this, and decode_corners, on the same inputs: the same bits.
__device__ __forceinline__ float tal_metric(float4 P, float4 gb, float x, bool has_class, const TalParams& tp, float& u) {
    u = box_quality(P, gb);
    const float s = has_class ? 1.0f / (1.0f + __expf(-x)) : 0.0f;
    return tal_pow(s, tp.alpha, false) * tal_pow(u, tp.beta, true);
}
__device__ __forceinline__ unsigned long long tal_key(float m, int a) { return make_key(ord_f32(m), a); }   // never 0: the low word is ~a >= 2^31

__global__ void __launch_bounds__(kTalThreads) tal_candidates_kernel(const float* __restrict__ gt_rows, int gt_stride, const int32_t* __restrict__ gt_off,
                                                                     int batch, const float4* __restrict__ anchors, int A,
                                                                     const float* __restrict__ scores, const float4* __restrict__ locs, TalParams tp,
                                                                     int topk, unsigned long long* __restrict__ cutoff, int* __restrict__ cand_anchor,
                                                                     float* __restrict__ cand_m, float* __restrict__ cand_u, int* __restrict__ cand_kept) {
    __shared__ unsigned long long s_red[2][kTalWaves];
    const int g = blockIdx.x;
    if (g >= gt_off[batch]) return;   // rows past the last image's are padding (a row buffer of fixed capacity)
    const int i = image_of_row(gt_off, batch, g);
    const float* r = gt_rows + (size_t)g * gt_stride;
    const float4 gb = make_float4(r[0], r[1], r[2], r[3]);
    const int col = class_column(r[4], tp.C);
    const size_t row0 = (size_t)i * A;
    auto metric = [&](int a, const float4& p, float& u) {   // of an inside anchor
        float4 cen;
        const float4 P = decode_corners(locs[row0 + a], p, tp.xy_scale, tp.wh_scale, cen);
        const float x = col >= 0 ? scores[(row0 + a) * tp.C + col] : 0.0f;
        return tal_metric(P, gb, x, col >= 0, tp, u);
    };
    auto key_of = [&](int a, const float4& p) {   // the inside test first; 0 = no key
        unsigned long long k = 0ull;
        if (centre_inside(gb, p)) { float u; k = tal_key(metric(a, p, u), a); }
        return k;
    };
    unsigned long long k1 = 0ull, k2 = 0ull;   // the thread's two largest keys
    sweep_anchors<kTalThreads>(anchors, 0, A, [&](int a, const float4& p) { keep_two<OpMaxU64>(key_of(a, p), k1, k2); });
    // Up to topk pops of the workgroup's largest remaining key; the first empty pop ends them: the box has fewer inside anchors than topk.
    unsigned long long cur = k1, mine = 0ull, last = kTalNoCutoff;
    for (int j = 0; j < topk; ++j) {
        const unsigned long long popped = pop_first<OpMaxU64, kTalThreads>(cur, s_red, j);
        if (popped == 0ull) break;   // (the same value in every thread)
        last = popped;
        if (threadIdx.x == j) mine = popped;   // (topk <= 32: thread j keeps the j-th candidate)
        pop_advance(popped, cur, k1, k2, [&] {
            return next_key_behind<OpMaxU64, kTalThreads>(popped, 0, A, [&](int b) { return key_of(b, anchors[b]); });
        });
    }
    if (threadIdx.x < SSDK_TAL_MAX_TOPK) {   // the candidate list in rank order; the slots past kk say so
        const size_t slot = (size_t)g * SSDK_TAL_MAX_TOPK + threadIdx.x;
        int ca = -1;
        float m = 0.0f, u = 0.0f;
        if (mine != 0ull) {
            ca = min(key_col(mine), A - 1);   // (a popped key is always an anchor; the clamp costs nothing)
            m = metric(ca, anchors[ca], u);
        }
        cand_anchor[slot] = ca;
        cand_m[slot] = m;
        cand_u[slot] = u;
        cand_kept[slot] = 0;
    }
    if (threadIdx.x == 0) cutoff[g] = last;
}

__global__ void __launch_bounds__(kAssignThreads) tal_assign_kernel(const float* __restrict__ gt_rows, int gt_stride, const int32_t* __restrict__ gt_off,
                                                                    const float4* __restrict__ anchors, int A, const float* __restrict__ scores,
                                                                    const float4* __restrict__ locs, TalParams tp, const unsigned long long* __restrict__ cutoff,
                                                                    const int* __restrict__ cand_anchor, int* __restrict__ cand_kept,
                                                                    float* __restrict__ target, int32_t* __restrict__ box_idx) {
    __shared__ float4 s_box[kGtChunk];
    __shared__ int s_col[kGtChunk];
    __shared__ unsigned long long s_cut[kGtChunk];
    __shared__ __attribute__((aligned(16))) float s_out[kAssignThreads * 6];

    const int i = blockIdx.y;
    const int a0 = blockIdx.x * kAssignThreads;
    const int a = a0 + threadIdx.x;
    const int g0 = gt_off[i], G = gt_off[i + 1] - g0;
    const bool live = a < A;
    const size_t row = (size_t)i * A + (live ? a : 0);

    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), P = p;
    if (live && G > 0) {
        float4 cen;
        p = anchors[a];
        P = decode_corners(locs[row], p, tp.xy_scale, tp.wh_scale, cen);
    }
    float best = 0.0f;
    int bi = SSDK_NOT_MATCHED;
    for_box_chunks(G, [&](int k, int j) {
        const float* r = gt_rows + (size_t)(g0 + k) * gt_stride;
        s_box[j] = make_float4(r[0], r[1], r[2], r[3]);
        s_col[j] = class_column(r[4], tp.C);
        s_cut[j] = cutoff[g0 + k];
    }, [&](int base, int n) {
        if (!live) return;
        for (int k = 0; k < n; ++k) {
            const float4 gb = s_box[k];
            if (!centre_inside(gb, p)) continue;
            const int col = s_col[k];
            const float x = col >= 0 ? scores[row * tp.C + col] : 0.0f;
            float u;
            const float m = tal_metric(P, gb, x, col >= 0, tp, u);
            if (tal_key(m, a) < s_cut[k]) continue;                      // not among the box's topk
            if (bi < 0 || u > best) { best = u; bi = base + k; }         // rule 7: ascending k, strict >: the lowest box index keeps a tie
        }
    });
    if (bi >= 0) {   // the thread is one of its box's candidates: its slot in the box's list (at most 32 entries, positives only)
        const size_t slot0 = (size_t)(g0 + bi) * SSDK_TAL_MAX_TOPK;
        for (int j = 0; j < SSDK_TAL_MAX_TOPK; ++j)
            if (cand_anchor[slot0 + j] == a) { cand_kept[slot0 + j] = 1; break; }
    }
    write_target_rows(gt_rows, gt_stride, g0, bi, i, a0, A, s_out, target, box_idx);
}

__global__ void __launch_bounds__(kTalNormThreads) tal_normalise_kernel(const float* __restrict__ gt_rows, int gt_stride, const int32_t* __restrict__ gt_off,
                                                                        int batch, int A, const int* __restrict__ cand_anchor,
                                                                        const float* __restrict__ cand_m, const float* __restrict__ cand_u,
                                                                        const int* __restrict__ cand_kept, float* __restrict__ target) {
    const int g = blockIdx.x * (kTalNormThreads / kWave) + (threadIdx.x >> 6);
    if (g >= gt_off[batch]) return;   // (a whole wave leaves: no barrier in this kernel)
    const int lane = lane_id();
    const int i = image_of_row(gt_off, batch, g);
    const size_t slot = (size_t)g * SSDK_TAL_MAX_TOPK + (lane < SSDK_TAL_MAX_TOPK ? lane : 0);
    const int a = lane < SSDK_TAL_MAX_TOPK ? cand_anchor[slot] : -1;
    const bool kept = a >= 0 && cand_kept[slot] != 0;
    const float m = kept ? cand_m[slot] : 0.0f, u = kept ? cand_u[slot] : 0.0f;
    // m >= 0 and u >= 0; fmaxf skips a NaN m (rule 5: below every number)
    const float m_max = wave_allreduce(m, OpMaxF()), u_max = wave_allreduce(u, OpMaxF());
    if (!kept) return;
    const float t = m / (m_max + 1e-9f) * u_max;
    target[((size_t)i * A + a) * 6 + 5] = gt_rows[(size_t)g * gt_stride + 5] * t;
}

// ---- SimOTA (YOLOX, arXiv:2107.08430 section 2.4; not in the reference) ----------------------------------------------------------------
// Per box: its REGION is the anchors whose centre lies strictly inside the box or inside a square of center_radius cells of the anchor's
// own level around the box centre; an anchor outside either of the two is `penalised`.  cost = class BCE + iou_weight * -log(u) from the
// anchor's own prediction; the box gets k_g = clamp((int)(sum of its q largest u), 1, #region) positives -- the count itself is a
// reduction -- and they are its k_g region anchors smallest by (penalised, cost, anchor); a candidate of several boxes goes to the
// smallest (penalised, cost), then the lowest box index (include/ssdk.h has the rule operation by operation).  The class BCE of anchor a
// against the one-hot row of class k is S_a - x[a, k - 1] with S_a = sum_c softplus(x[a, c]): a number per anchor and one logit per
// (anchor, box), so nothing [G, A, C]-shaped is ever read.  Three launches, no atomics, nothing zero-filled:
//   1. simota_class_sum_kernel   one thread per (image, anchor) for the region test against the image's boxes from LDS; only the anchors in
//                                some box's region have their C logits read -- eight lanes per row -- and S_a stored in the workspace.
//                                Launches 2 and 3 both READ that value (and only at region anchors), which is why their keys agree bit
//                                for bit.
//   2. simota_candidates_kernel  one workgroup per box: ONE sweep of the anchor table, the region test first; a region anchor loads its loc,
//                                S_a and the one logit of the box's class and becomes two keys -- (ord(u) << 32 | ~a), larger = better,
//                                and (penalised << 63 | ord(cost) << 31 | a), smaller = better.  Up to q pops of the largest u-key give
//                                the fp64 sum and k_g, then k_g pops of the smallest cost-key give the box's cutoff key.
//   3. simota_assign_kernel      one thread per (image, anchor), on the pattern of tal_assign_kernel: it recomputes its cost-key against
//                                every box whose region holds it with the SAME device functions and is a candidate exactly when
//                                key <= cutoff(box).
// (No candidate list leaves launch 2: nothing after it would read one -- column 5 is the box's score, there is no normalise pass.)
constexpr int kSimotaThreads = 1024;
constexpr int kSimotaWaves = kSimotaThreads / kWave;
constexpr unsigned long long kSimotaNoKey = ~0ull;   // above every cost-key (an anchor index is below 2^31 - 1)
// by value: beside the level table, every level's centre square's half sides (rx, ry) = center_radius * (sx, sy), one fp32 product each,
// formed on the host
struct SimotaLevels { Levels lv; float rx[SSDK_ATSS_MAX_LEVELS]; float ry[SSDK_ATSS_MAX_LEVELS]; };
struct SimotaParams { float xy_scale, wh_scale, iou_weight; int C; };

// (rx, ry) of anchor a's level (constant indices: a by-value table indexed by a variable would be copied to scratch)
__device__ __forceinline__ float2 simota_radius(const SimotaLevels& sl, int a) {
    float2 r = make_float2(sl.rx[0], sl.ry[0]);
#pragma unroll
    for (int q = 1; q < SSDK_ATSS_MAX_LEVELS; ++q) {
        if (q >= sl.lv.n) break;   // (the same in every lane: a scalar branch past the levels that do not exist)
        if (a >= sl.lv.off[q]) r = make_float2(sl.rx[q], sl.ry[q]);
    }
    return r;
}
// rule 2 on the inputs: exact.  gc = box_centre(gb), r = simota_radius(level of p)
__device__ __forceinline__ bool simota_region(float4 gb, float2 gc, float4 p, float2 r, bool& penalised) {
    const bool in_box = centre_inside(gb, p);
    const bool in_centre = gc.x - r.x < p.x && p.x < gc.x + r.x && gc.y - r.y < p.y && p.y < gc.y + r.y;
    penalised = !(in_box && in_centre);
    return in_box || in_centre;
}
__device__ __forceinline__ float simota_softplus(float x) { return fmaxf(x, 0.0f) + __logf(1.0f + __expf(-fabsf(x))); }
// rules 3 and 4: S the anchor's class sum, x the logit of the box's class (has_class: the class is one of the columns), u rule 1's quality
__device__ __forceinline__ float simota_cost(float S, float x, bool has_class, float u, float iou_weight) {
    const float cls = has_class ? S - x : S;
    return cls + iou_weight * (-__logf(u + 1e-8f));
}
// smaller = better: the unpenalised before the penalised, then the lower cost (NaN above every number), then the lower anchor
__device__ __forceinline__ unsigned long long simota_key(bool penalised, float cost, int a) {
    const unsigned hi = (cost != cost) ? 0xFFFFFFFFu : ord_f32(cost);
    return ((unsigned long long)(penalised ? 1u : 0u) << 63) | ((unsigned long long)hi << 31) | (unsigned long long)(unsigned)a;
}
// Rule 3's S_a of one row of logits, by the kSimotaRowLanes lanes of a lane group: lane l adds the softplus terms of the column quads
// 4j..4j+3 with j = l, l + 8, ... in ascending column order into one accumulator (a quad is one 16-byte load where the row allows it: the
// same additions in the same order either way), then the eight partial sums meet in a butterfly (xor 4, 2, 1), which leaves the same bits
// in every lane.
constexpr int kSimotaRowLanes = 8;
__device__ __forceinline__ float simota_class_sum_lane(const float* __restrict__ x, int C, int l) {
    const bool vec = (((uintptr_t)x) & 15) == 0;
    const int full = C >> 2;
    float s = 0.0f;
    for (int j = l; j * 4 < C; j += kSimotaRowLanes) {
        if (vec && j < full) {
            const float4 v = reinterpret_cast<const float4*>(x)[j];
            s += simota_softplus(v.x);
            s += simota_softplus(v.y);
            s += simota_softplus(v.z);
            s += simota_softplus(v.w);
        } else {
            for (int c = 4 * j; c < min(4 * j + 4, C); ++c) s += simota_softplus(x[c]);
        }
    }
    return s;
}

__global__ void __launch_bounds__(kAssignThreads) simota_class_sum_kernel(const float* __restrict__ gt_rows, int gt_stride, const int32_t* __restrict__ gt_off,
                                                                          const float4* __restrict__ anchors, int A, SimotaLevels lv,
                                                                          const float* __restrict__ scores, int C, float* __restrict__ class_sum) {
    __shared__ float4 s_box[kGtChunk];
    __shared__ float2 s_centre[kGtChunk];
    __shared__ int s_rows[kAssignThreads];
    __shared__ int s_cnt[kAssignThreads / kWave];
    const int i = blockIdx.y;
    const int a = blockIdx.x * kAssignThreads + threadIdx.x;
    const int g0 = gt_off[i], G = gt_off[i + 1] - g0;
    const bool live = a < A;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 r = make_float2(0.f, 0.f);
    if (live && G > 0) {
        p = anchors[a];
        r = simota_radius(lv, a);
    }
    bool hit = false;   // the anchor lies in some box's region
    for_box_chunks(G, [&](int k, int j) {
        const float* row = gt_rows + (size_t)(g0 + k) * gt_stride;
        const float4 gb = make_float4(row[0], row[1], row[2], row[3]);
        s_box[j] = gb;
        s_centre[j] = box_centre(gb);
    }, [&](int base, int n) {
        if (live && !hit)
            for (int k = 0; k < n; ++k) {
                bool pen;
                if (simota_region(s_box[k], s_centre[k], p, r, pen)) { hit = true; break; }
            }
    });
    // The block's region anchors, in anchor order, into s_rows (ballot + popcount: no atomics); then eight lanes per row, so that a row of
    // logits is read as whole 128-byte runs instead of one 16-byte piece per lane and row.
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, rows = 0;
#pragma unroll
    for (int w = 0; w < kAssignThreads / kWave; ++w) {
        const int c = s_cnt[w];
        before += w < wave ? c : 0;
        rows += c;
    }
    if (hit) s_rows[before + __popcll(mask & ((1ull << lane) - 1ull))] = a;
    __syncthreads();
    const int l = threadIdx.x & (kSimotaRowLanes - 1), group = threadIdx.x / kSimotaRowLanes;
    for (int r0 = 0; r0 < rows; r0 += kAssignThreads / kSimotaRowLanes) {   // (the same trip count in every lane: the shuffles below are unconditional)
        const int slot = r0 + group;
        const bool on = slot < rows;
        const size_t row = (size_t)i * A + (on ? s_rows[slot] : 0);
        float v = on ? simota_class_sum_lane(scores + row * C, C, l) : 0.0f;
#pragma unroll
        for (int m = kSimotaRowLanes / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
        if (on && l == 0) class_sum[row] = v;
    }
}

__global__ void __launch_bounds__(kSimotaThreads) simota_candidates_kernel(const float* __restrict__ gt_rows, int gt_stride, const int32_t* __restrict__ gt_off,
                                                                           int batch, const float4* __restrict__ anchors, int A, SimotaLevels lv,
                                                                           const float* __restrict__ scores, const float4* __restrict__ locs,
                                                                           const float* __restrict__ class_sum, SimotaParams sp, int topk,
                                                                           unsigned long long* __restrict__ cutoff, int32_t* __restrict__ dynamic_k) {
    __shared__ unsigned long long s_red[2][kSimotaWaves];
    const int g = blockIdx.x;
    if (g >= gt_off[batch]) {   // rows past the last image's are padding (a row buffer of fixed capacity)
        if (dynamic_k && threadIdx.x == 0) dynamic_k[g] = 0;
        return;
    }
    const int i = image_of_row(gt_off, batch, g);
    const float* r = gt_rows + (size_t)g * gt_stride;
    const float4 gb = make_float4(r[0], r[1], r[2], r[3]);
    const float2 gc = box_centre(gb);
    const int col = class_column(r[4], sp.C);
    const size_t row0 = (size_t)i * A;
    // An anchor against the box in two steps, so that a sweep round can have the gathered loads of its four anchors in flight together:
    // `fetch` is the region test and, for a region anchor, the loads of its loc, class sum and the one logit of the box's class; `finish`
    // turns what was fetched into the two keys (and leaves them as they were for an anchor outside the region).
    struct Fetched { float4 t; float x, S; bool in, pen; };
    auto fetch = [&](int a, const float4& p, Fetched& f) {
        f.in = simota_region(gb, gc, p, simota_radius(lv, a), f.pen);
        if (f.in) {
            f.t = locs[row0 + a];
            f.x = col >= 0 ? scores[(row0 + a) * sp.C + col] : 0.0f;
            f.S = class_sum[row0 + a];
        }
    };
    auto finish = [&](int a, const float4& p, const Fetched& f, unsigned long long& ku, unsigned long long& kc) {
        if (!f.in) return;
        float4 cen;
        const float4 P = decode_corners(f.t, p, sp.xy_scale, sp.wh_scale, cen);
        const float u = box_quality(P, gb);
        ku = make_key(ord_f32(u), a);   // never 0: the low word is ~a >= 2^31
        kc = simota_key(f.pen, simota_cost(f.S, f.x, col >= 0, u, sp.iou_weight), a);
    };
    // The sweep: the thread's two largest u-keys (0 = none) and two smallest cost-keys (kSimotaNoKey = none).
    unsigned long long u1 = 0ull, u2 = 0ull, c1 = kSimotaNoKey, c2 = kSimotaNoKey;
    auto take = [&](int a, const float4& p, const Fetched& f) {
        unsigned long long ku = 0ull, kc = kSimotaNoKey;
        finish(a, p, f, ku, kc);
        keep_two<OpMaxU64>(ku, u1, u2);
        keep_two<OpMinU64>(kc, c1, c2);
    };
    int a = threadIdx.x;
    for (; a + 3 * kSimotaThreads < A; a += 4 * kSimotaThreads) {   // four anchor loads in flight, then the four anchors' gathered loads
        const float4 p0 = anchors[a], p1 = anchors[a + kSimotaThreads], p2 = anchors[a + 2 * kSimotaThreads], p3 = anchors[a + 3 * kSimotaThreads];
        Fetched f0, f1, f2, f3;
        fetch(a, p0, f0);
        fetch(a + kSimotaThreads, p1, f1);
        fetch(a + 2 * kSimotaThreads, p2, f2);
        fetch(a + 3 * kSimotaThreads, p3, f3);
        take(a, p0, f0);
        take(a + kSimotaThreads, p1, f1);
        take(a + 2 * kSimotaThreads, p2, f2);
        take(a + 3 * kSimotaThreads, p3, f3);
    }
    for (; a < A; a += kSimotaThreads) {
        const float4 p = anchors[a];
        Fetched f;
        fetch(a, p, f);
        take(a, p, f);
    }
    // A re-read of the thread's own anchors: anchor b's u-key (want_u) or cost-key, `none` outside the region.
    auto key_of = [&](int b, bool want_u) {
        const float4 p = anchors[b];
        Fetched f;
        fetch(b, p, f);
        unsigned long long ku = 0ull, kc = kSimotaNoKey;
        finish(b, p, f, ku, kc);
        return want_u ? ku : kc;
    };
    // Rule 5: up to topk pops of the workgroup's largest remaining u-key (`step` counts the pops of BOTH loops: they share s_red's
    // halves); the first empty pop ends them: the box has fewer region anchors than topk.  Every thread adds the popped u to its own copy
    // of the sum, in rank order.
    int step = 0, qq = 0;
    double sum = 0.0;
    unsigned long long cur = u1;
    for (int j = 0; j < topk; ++j) {
        const unsigned long long popped = pop_first<OpMaxU64, kSimotaThreads>(cur, s_red, step++);
        if (popped == 0ull) break;   // (the same value in every thread)
        ++qq;
        sum += (double)__uint_as_float(key_hi(popped) & 0x7FFFFFFFu);   // u >= 0: ord_f32 set the sign bit, 0 is kOrdZero
        pop_advance(popped, cur, u1, u2, [&] {
            return next_key_behind<OpMaxU64, kSimotaThreads>(popped, 0, A, [&](int b) { return key_of(b, true); });
        });
    }
    int kg = 0;
    if (qq > 0) kg = min(max((int)sum, 1), qq);   // (sum <= 32)
    // Rule 6: kg pops of the smallest remaining cost-key; the last is the box's cutoff.  kg <= #region: no pop is empty.
    unsigned long long last = 0ull;   // below every key: a box without a region anchor has no candidate
    cur = c1;
    for (int j = 0; j < kg; ++j) {
        last = pop_first<OpMinU64, kSimotaThreads>(cur, s_red, step++);
        pop_advance(last, cur, c1, c2, [&] {
            return next_key_behind<OpMinU64, kSimotaThreads>(last, 0, A, [&](int b) { return key_of(b, false); });
        });
    }
    if (threadIdx.x == 0) {
        cutoff[g] = last;
        if (dynamic_k) dynamic_k[g] = kg;
    }
}

__global__ void __launch_bounds__(kAssignThreads) simota_assign_kernel(const float* __restrict__ gt_rows, int gt_stride, const int32_t* __restrict__ gt_off,
                                                                       const float4* __restrict__ anchors, int A, SimotaLevels lv,
                                                                       const float* __restrict__ scores, const float4* __restrict__ locs,
                                                                       const float* __restrict__ class_sum, SimotaParams sp,
                                                                       const unsigned long long* __restrict__ cutoff, float* __restrict__ target,
                                                                       int32_t* __restrict__ box_idx) {
    __shared__ float4 s_box[kGtChunk];
    __shared__ float2 s_centre[kGtChunk];
    __shared__ int s_col[kGtChunk];
    __shared__ unsigned long long s_cut[kGtChunk];
    __shared__ __attribute__((aligned(16))) float s_out[kAssignThreads * 6];

    const int i = blockIdx.y;
    const int a0 = blockIdx.x * kAssignThreads;
    const int a = a0 + threadIdx.x;
    const int g0 = gt_off[i], G = gt_off[i + 1] - g0;
    const bool live = a < A;
    const size_t row = (size_t)i * A + (live ? a : 0);

    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), P = p;
    float2 rad = make_float2(0.f, 0.f);
    if (live && G > 0) {
        float4 cen;
        p = anchors[a];
        rad = simota_radius(lv, a);
        P = decode_corners(locs[row], p, sp.xy_scale, sp.wh_scale, cen);
    }
    float S = 0.0f;
    bool have_S = false;   // (launch 1 stored S only where some box's region holds the anchor: read it on the first hit)
    unsigned long long best = 0ull;
    int bi = SSDK_NOT_MATCHED;
    for_box_chunks(G, [&](int k, int j) {
        const float* r = gt_rows + (size_t)(g0 + k) * gt_stride;
        const float4 gb = make_float4(r[0], r[1], r[2], r[3]);
        s_box[j] = gb;
        s_centre[j] = box_centre(gb);
        s_col[j] = class_column(r[4], sp.C);
        s_cut[j] = cutoff[g0 + k];
    }, [&](int base, int n) {
        if (!live) return;
        for (int k = 0; k < n; ++k) {
            const float4 gb = s_box[k];
            bool pen;
            if (!simota_region(gb, s_centre[k], p, rad, pen)) continue;
            if (!have_S) { S = class_sum[row]; have_S = true; }
            const int col = s_col[k];
            const float x = col >= 0 ? scores[row * sp.C + col] : 0.0f;
            const float u = box_quality(P, gb);
            const unsigned long long key = simota_key(pen, simota_cost(S, x, col >= 0, u, sp.iou_weight), a);
            if (key > s_cut[k]) continue;                                           // not among the box's k_g
            const unsigned long long rank = key >> 31;                              // rule 7: (penalised, cost) without the anchor
            if (bi < 0 || rank < best) { best = rank; bi = base + k; }              // ascending k, strict <: the lowest box index keeps a tie
        }
    });
    write_target_rows(gt_rows, gt_stride, g0, bi, i, a0, A, s_out, target, box_idx);
}

}  // namespace ssdk

using namespace ssdk;

extern "C" size_t ssdk_match_per_prediction_workspace_bytes(int num_boxes) {
    Carver c(nullptr);
    c.take<unsigned long long>((size_t)(num_boxes > 0 ? num_boxes : 1));
    return c.off;
}

extern "C" int ssdk_match_per_prediction(const float* weights, int num_boxes, int num_anchors, float matched_threshold,
                                         float unmatched_threshold, int force_match_for_each_target, int64_t* box_idx, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    SSDK_REQUIRE(weights && box_idx && num_boxes > 0 && num_anchors > 0, SSDK_E_INVALID,
                 "ssdk_match_per_prediction: boxes=%d anchors=%d (weights.max(dim=0) of an empty matrix is an error in the reference too)",
                 num_boxes, num_anchors);
    SSDK_REQUIRE(num_boxes <= 65535, SSDK_E_INVALID, "ssdk_match_per_prediction: more than 65535 boxes");
    SSDK_REQUIRE(matched_threshold >= unmatched_threshold, SSDK_E_INVALID,
                 "ssdk_match_per_prediction: matched_threshold < unmatched_threshold (matcher.py:43)");
    SSDK_REQUIRE(workspace && workspace_bytes >= ssdk_match_per_prediction_workspace_bytes(num_boxes), SSDK_E_WORKSPACE,
                 "ssdk_match_per_prediction: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* best = (unsigned long long*)workspace;
    if (force_match_for_each_target) {
        SSDK_CHECK_HIP(zero_async(best, sizeof(unsigned long long) * (size_t)num_boxes, s));
        hipLaunchKernelGGL(mpp_row_argmax_kernel, dim3(cdiv(num_anchors, kSegAnchors * 4), num_boxes), dim3(256), 0, s, weights, num_anchors, best);
        SSDK_CHECK_LAUNCH("mpp_row_argmax_kernel");
    }
    hipLaunchKernelGGL(mpp_assign_kernel, dim3(cdiv(num_anchors, kAssignThreads)), dim3(kAssignThreads), 0, s, weights, num_boxes, num_anchors,
                       matched_threshold, unmatched_threshold, force_match_for_each_target, best, (long long*)box_idx);
    SSDK_CHECK_LAUNCH("mpp_assign_kernel");
    return SSDK_OK;
}

extern "C" size_t ssdk_match_bipartite_workspace_bytes(int num_boxes, int num_anchors) {
    const size_t g = (size_t)(num_boxes > 0 ? num_boxes : 1), a = (size_t)(num_anchors > 0 ? num_anchors : 1);
    Carver c(nullptr);
    c.take<unsigned long long>(g);
    c.take<int>(g);
    c.take<float>(g * a);   // the working copy of a matrix that is not matched in place
    return c.off;
}

extern "C" int ssdk_match_bipartite(float* weights, int num_boxes, int num_anchors, int inplace, int64_t* anchor_idx, int32_t* num_matched,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    SSDK_REQUIRE(num_boxes > 0 && num_anchors > 0, SSDK_E_INVALID, "ssdk_match_bipartite: boxes=%d anchors=%d", num_boxes, num_anchors);
    SSDK_REQUIRE(weights && anchor_idx && num_matched, SSDK_E_INVALID, "ssdk_match_bipartite: null pointer");
    SSDK_REQUIRE(num_boxes <= 65535, SSDK_E_INVALID, "ssdk_match_bipartite: more than 65535 boxes");
    SSDK_REQUIRE(workspace && workspace_bytes >= ssdk_match_bipartite_workspace_bytes(num_boxes, num_anchors), SSDK_E_WORKSPACE,
                 "ssdk_match_bipartite: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Carver c(workspace);
    unsigned long long* keys = c.take<unsigned long long>((size_t)num_boxes);
    int* rows = c.take<int>((size_t)num_boxes);
    float* w = weights;
    if (!inplace) {
        const size_t n = (size_t)num_boxes * (size_t)num_anchors;
        w = c.take<float>(n);
        const size_t want = (n + 255) / 256;
        hipLaunchKernelGGL(copy_f32_kernel, dim3((unsigned)(want > 2048 ? 2048 : want)), dim3(256), 0, s, weights, w, n);
        SSDK_CHECK_LAUNCH("copy_f32_kernel");
    }
    hipLaunchKernelGGL(match_bipartite_kernel, dim3(1), dim3(kBipThreads), 0, s, w, num_boxes, num_anchors, (long long*)anchor_idx, num_matched, keys, rows);
    SSDK_CHECK_LAUNCH("match_bipartite_kernel");
    return SSDK_OK;
}

// ---- the ssdk_encode_ground_truth* entry points -------------------------------------------------------------------------------------------
// What they all require, under the entry's own name.  `further_ptrs`: the entry's further mandatory pointers are there;
// `total_gt_limit`: the two IoU entries also bound total_gt.
constexpr bool kNoFurtherPointers = true;
enum TotalGtLimit { kBatchLimitOnly, kBatchAndTotalGtLimit };
static int check_encode_args(const char* entry, const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                             const float* anchors, int num_anchors, const float* target, bool further_ptrs, TotalGtLimit total_gt_limit) {
    SSDK_REQUIRE(batch > 0 && num_anchors > 0 && total_gt >= 0, SSDK_E_INVALID, "%s: batch=%d anchors=%d total_gt=%d", entry, batch, num_anchors,
                 total_gt);
    if (total_gt_limit == kBatchAndTotalGtLimit)
        SSDK_REQUIRE(batch <= 65535 && total_gt <= 65535, SSDK_E_INVALID, "%s: batch/total_gt exceed grid limits", entry);
    else
        SSDK_REQUIRE(batch <= 65535, SSDK_E_INVALID, "%s: batch exceeds grid limits", entry);
    SSDK_REQUIRE(gt_offsets && anchors && target && further_ptrs && (gt_rows || total_gt == 0), SSDK_E_INVALID, "%s: null pointer", entry);
    SSDK_REQUIRE(gt_stride >= 6, SSDK_E_INVALID, "%s: gt_stride=%d < 6", entry, gt_stride);
    return SSDK_OK;
}
// The last check of every entry, after its own arguments are known to be valid: `need` is the entry's carve of the workspace.
static int check_workspace(const char* entry, const void* workspace, size_t workspace_bytes, size_t need) {
    SSDK_REQUIRE(workspace && workspace_bytes >= need, SSDK_E_WORKSPACE, "%s: workspace too small", entry);
    return SSDK_OK;
}
// What the two prediction-aware entries (TAL, SimOTA) require of the anchors' own predictions.
static int check_prediction_args(const char* entry, const float* anchors, const float* scores, int num_columns, const float* locs) {
    SSDK_REQUIRE(scores && locs, SSDK_E_INVALID, "%s: null scores or locs (the rule reads the anchors' own predictions)", entry);
    SSDK_REQUIRE(num_columns >= 1, SSDK_E_INVALID, "%s: num_columns=%d < 1", entry, num_columns);
    SSDK_REQUIRE((((uintptr_t)anchors | (uintptr_t)locs) & 15) == 0, SSDK_E_UNSUPPORTED, "%s: anchors and locs must be 16-byte aligned", entry);
    return SSDK_OK;
}
// The by-value level table of ATSS and SimOTA from the caller's level sizes, which must be positive and sum to the anchors.
static int build_levels(const char* entry, const int32_t* level_sizes, int n_levels, int num_anchors, Levels& lv) {
    SSDK_REQUIRE(n_levels >= 1 && n_levels <= SSDK_ATSS_MAX_LEVELS, SSDK_E_INVALID, "%s: n_levels=%d outside 1..%d", entry, n_levels,
                 SSDK_ATSS_MAX_LEVELS);
    lv.n = n_levels;
    long long sum = 0;
    for (int l = 0; l <= SSDK_ATSS_MAX_LEVELS; ++l) {
        lv.off[l] = (int)sum;   // (the entries past n_levels repeat the total)
        if (l < n_levels) {
            SSDK_REQUIRE(level_sizes[l] > 0, SSDK_E_INVALID, "%s: level_sizes[%d]=%d", entry, l, level_sizes[l]);
            sum += level_sizes[l];
            SSDK_REQUIRE(sum <= num_anchors, SSDK_E_INVALID, "%s: level sizes exceed the %d anchors", entry, num_anchors);
        }
    }
    SSDK_REQUIRE(sum == num_anchors, SSDK_E_INVALID, "%s: level sizes sum to %lld, not to the %d anchors", entry, sum, num_anchors);
    return SSDK_OK;
}
static inline size_t box_slots(int total_gt) { return (size_t)(total_gt > 0 ? total_gt : 1); }

// Every workspace is carved by ONE function: *_workspace_bytes calls it on a null base for `bytes`, the entry point on the workspace.
struct IouWorkspace { unsigned long long* gt_best; unsigned long long* spill_keys; int* spill_rows; size_t bytes; };
static IouWorkspace carve_iou(void* base, int total_gt, int force_match) {
    Carver c(base);
    IouWorkspace w = {};
    w.gt_best = c.take<unsigned long long>(box_slots(total_gt) * kArgmaxMaxSegs);
    if (force_match == SSDK_FORCE_MATCH_BIPARTITE) {
        w.spill_keys = c.take<unsigned long long>(box_slots(total_gt));
        w.spill_rows = c.take<int>(box_slots(total_gt));
    }
    w.bytes = c.off;
    return w;
}

extern "C" size_t ssdk_encode_ground_truth_workspace_bytes(int batch, int total_gt) {
    (void)batch;
    return carve_iou(nullptr, total_gt, SSDK_FORCE_MATCH_PER_PREDICTION).bytes;
}

extern "C" size_t ssdk_encode_ground_truth_ex_workspace_bytes(int batch, int total_gt, int force_match) {
    (void)batch;
    return carve_iou(nullptr, total_gt, force_match).bytes;
}

// Both IoU entry points: gt_argmax_kernel, the bipartite stage where asked for, assign_kernel.
static int encode_iou(const char* entry, const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                      const float* anchors, int num_anchors, float matched_threshold, float unmatched_threshold, int force_match, float* target,
                      int32_t* box_idx, void* workspace, size_t workspace_bytes, void* stream) {
    const bool bipartite = force_match == SSDK_FORCE_MATCH_BIPARTITE;
    const IouWorkspace w = carve_iou(workspace, total_gt, force_match);
    int e = check_encode_args(entry, gt_rows, gt_stride, gt_offsets, batch, total_gt, anchors, num_anchors, target, kNoFurtherPointers,
                              kBatchAndTotalGtLimit);
    if (e != SSDK_OK) return e;
    SSDK_REQUIRE(!bipartite || num_anchors <= kBipMaxAnchors, SSDK_E_UNSUPPORTED, "%s: bipartite matching takes at most %d anchors, got %d", entry,
                 kBipMaxAnchors, num_anchors);
    SSDK_REQUIRE(matched_threshold >= unmatched_threshold, SSDK_E_INVALID, "%s: matched_threshold < unmatched_threshold (matcher.py:43)", entry);
    if ((e = check_workspace(entry, workspace, workspace_bytes, w.bytes)) != SSDK_OK) return e;
    hipStream_t s = (hipStream_t)stream;
    const int segs = argmax_segs(num_anchors);
    if (total_gt > 0) {
        hipLaunchKernelGGL(gt_argmax_kernel, dim3(total_gt, segs), dim3(kArgmaxThreads), 0, s, gt_rows, gt_stride, (const float4*)anchors, num_anchors, w.gt_best, gt_offsets, batch);
        SSDK_CHECK_LAUNCH("gt_argmax_kernel");
        if (bipartite) {
            hipLaunchKernelGGL(bipartite_resolve_kernel, dim3(batch), dim3(kBipThreads), 0, s, gt_rows, gt_stride, gt_offsets, (const float4*)anchors,
                               num_anchors, w.gt_best, segs, w.spill_keys, w.spill_rows);
            SSDK_CHECK_LAUNCH("bipartite_resolve_kernel");
        }
    }
    dim3 grid(cdiv(num_anchors, kAssignThreads), batch);
    hipLaunchKernelGGL(assign_kernel, grid, dim3(kAssignThreads), 0, s, gt_rows, gt_stride, gt_offsets, (const float4*)anchors,
                       num_anchors, matched_threshold, unmatched_threshold, w.gt_best, segs, target, box_idx);
    SSDK_CHECK_LAUNCH("assign_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_encode_ground_truth(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch,
                                        int total_gt, const float* anchors, int num_anchors, float matched_threshold,
                                        float unmatched_threshold, float* target, int32_t* box_idx, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    return encode_iou("ssdk_encode_ground_truth", gt_rows, gt_stride, gt_offsets, batch, total_gt, anchors, num_anchors, matched_threshold,
                      unmatched_threshold, SSDK_FORCE_MATCH_PER_PREDICTION, target, box_idx, workspace, workspace_bytes, stream);
}

extern "C" int ssdk_encode_ground_truth_ex(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                                           const float* anchors, int num_anchors, float matched_threshold, float unmatched_threshold,
                                           int force_match, float* target, int32_t* box_idx, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    SSDK_REQUIRE(force_match == SSDK_FORCE_MATCH_PER_PREDICTION || force_match == SSDK_FORCE_MATCH_BIPARTITE, SSDK_E_INVALID,
                 "ssdk_encode_ground_truth_ex: force_match=%d", force_match);
    // (the default rule keeps the messages it always had: ssdk_encode_ground_truth's)
    return encode_iou(force_match == SSDK_FORCE_MATCH_BIPARTITE ? "ssdk_encode_ground_truth_ex" : "ssdk_encode_ground_truth", gt_rows, gt_stride,
                      gt_offsets, batch, total_gt, anchors, num_anchors, matched_threshold, unmatched_threshold, force_match, target, box_idx,
                      workspace, workspace_bytes, stream);
}

struct AtssWorkspace { unsigned long long* cutoff; float* cand_iou; size_t bytes; };
static AtssWorkspace carve_atss(void* base, int total_gt, int n_levels) {
    const size_t slots = box_slots(total_gt) * (size_t)(n_levels > 0 ? n_levels : 1);
    Carver c(base);
    AtssWorkspace w;
    w.cutoff = c.take<unsigned long long>(slots);
    w.cand_iou = c.take<float>(slots * SSDK_ATSS_MAX_TOPK);
    w.bytes = c.off;
    return w;
}

extern "C" size_t ssdk_encode_ground_truth_atss_workspace_bytes(int batch, int total_gt, int n_levels) {
    (void)batch;
    return carve_atss(nullptr, total_gt, n_levels).bytes;
}

extern "C" int ssdk_encode_ground_truth_atss(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                                             const float* anchors, int num_anchors, const int32_t* level_sizes, int n_levels, int topk,
                                             float* target, int32_t* box_idx, void* workspace, size_t workspace_bytes, void* stream) {
    const char* entry = "ssdk_encode_ground_truth_atss";
    const AtssWorkspace w = carve_atss(workspace, total_gt, n_levels);
    int e = check_encode_args(entry, gt_rows, gt_stride, gt_offsets, batch, total_gt, anchors, num_anchors, target, level_sizes != nullptr,
                              kBatchLimitOnly);
    if (e != SSDK_OK) return e;
    Levels lv;
    if ((e = build_levels(entry, level_sizes, n_levels, num_anchors, lv)) != SSDK_OK) return e;
    SSDK_REQUIRE(topk >= 1 && topk <= SSDK_ATSS_MAX_TOPK, SSDK_E_INVALID, "%s: topk=%d outside 1..%d", entry, topk, SSDK_ATSS_MAX_TOPK);
    if ((e = check_workspace(entry, workspace, workspace_bytes, w.bytes)) != SSDK_OK) return e;
    hipStream_t s = (hipStream_t)stream;
    if (total_gt > 0) {
        hipLaunchKernelGGL(atss_candidates_kernel, dim3(total_gt, n_levels), dim3(kAtssThreads), 0, s, gt_rows, gt_stride, gt_offsets, batch,
                           (const float4*)anchors, lv, topk, w.cutoff, w.cand_iou);
        SSDK_CHECK_LAUNCH("atss_candidates_kernel");
    }
    dim3 grid(cdiv(num_anchors, kAssignThreads), batch);
    hipLaunchKernelGGL(atss_assign_kernel, grid, dim3(kAssignThreads), 0, s, gt_rows, gt_stride, gt_offsets, (const float4*)anchors, num_anchors, lv,
                       topk, w.cutoff, w.cand_iou, target, box_idx);
    SSDK_CHECK_LAUNCH("atss_assign_kernel");
    return SSDK_OK;
}

struct TalWorkspace { unsigned long long* cutoff; int* cand_anchor; float* cand_m; float* cand_u; int* cand_kept; size_t bytes; };
// (a box's list has SSDK_TAL_MAX_TOPK slots whatever topk is: the slot of (box, rank) does not move with it)
static TalWorkspace carve_tal(void* base, int total_gt) {
    const size_t list = box_slots(total_gt) * SSDK_TAL_MAX_TOPK;
    Carver c(base);
    TalWorkspace w;
    w.cutoff = c.take<unsigned long long>(box_slots(total_gt));
    w.cand_anchor = c.take<int>(list);
    w.cand_m = c.take<float>(list);
    w.cand_u = c.take<float>(list);
    w.cand_kept = c.take<int>(list);
    w.bytes = c.off;
    return w;
}

extern "C" size_t ssdk_encode_ground_truth_tal_workspace_bytes(int batch, int total_gt, int topk) {
    (void)batch;
    (void)topk;
    return carve_tal(nullptr, total_gt).bytes;
}

extern "C" int ssdk_encode_ground_truth_tal(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                                            const float* anchors, int num_anchors, const float* scores, int num_columns, const float* locs,
                                            float xy_scale, float wh_scale, int topk, float alpha, float beta, float* target, int32_t* box_idx,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* entry = "ssdk_encode_ground_truth_tal";
    const TalWorkspace w = carve_tal(workspace, total_gt);
    int e = check_encode_args(entry, gt_rows, gt_stride, gt_offsets, batch, total_gt, anchors, num_anchors, target, kNoFurtherPointers,
                              kBatchLimitOnly);
    if (e != SSDK_OK) return e;
    if ((e = check_prediction_args(entry, anchors, scores, num_columns, locs)) != SSDK_OK) return e;
    SSDK_REQUIRE(topk >= 1 && topk <= SSDK_TAL_MAX_TOPK, SSDK_E_INVALID, "%s: topk=%d outside 1..%d", entry, topk, SSDK_TAL_MAX_TOPK);
    SSDK_REQUIRE(alpha >= 0.0f && alpha <= FLT_MAX && beta >= 0.0f && beta <= FLT_MAX, SSDK_E_INVALID,
                 "%s: alpha=%g beta=%g must be finite and not negative", entry, (double)alpha, (double)beta);
    if ((e = check_workspace(entry, workspace, workspace_bytes, w.bytes)) != SSDK_OK) return e;
    hipStream_t s = (hipStream_t)stream;
    TalParams tp;
    tp.xy_scale = xy_scale; tp.wh_scale = wh_scale; tp.alpha = alpha; tp.beta = beta; tp.C = num_columns;
    if (total_gt > 0) {
        hipLaunchKernelGGL(tal_candidates_kernel, dim3(total_gt), dim3(kTalThreads), 0, s, gt_rows, gt_stride, gt_offsets, batch,
                           (const float4*)anchors, num_anchors, scores, (const float4*)locs, tp, topk, w.cutoff, w.cand_anchor, w.cand_m, w.cand_u,
                           w.cand_kept);
        SSDK_CHECK_LAUNCH("tal_candidates_kernel");
    }
    dim3 grid(cdiv(num_anchors, kAssignThreads), batch);
    hipLaunchKernelGGL(tal_assign_kernel, grid, dim3(kAssignThreads), 0, s, gt_rows, gt_stride, gt_offsets, (const float4*)anchors, num_anchors,
                       scores, (const float4*)locs, tp, w.cutoff, w.cand_anchor, w.cand_kept, target, box_idx);
    SSDK_CHECK_LAUNCH("tal_assign_kernel");
    if (total_gt > 0) {
        hipLaunchKernelGGL(tal_normalise_kernel, dim3(cdiv(total_gt, kTalNormThreads / kWave)), dim3(kTalNormThreads), 0, s, gt_rows, gt_stride,
                           gt_offsets, batch, num_anchors, w.cand_anchor, w.cand_m, w.cand_u, w.cand_kept, target);
        SSDK_CHECK_LAUNCH("tal_normalise_kernel");
    }
    return SSDK_OK;
}

struct SimotaWorkspace { float* class_sum; unsigned long long* cutoff; size_t bytes; };
static SimotaWorkspace carve_simota(void* base, int batch, int total_gt, int num_anchors) {
    Carver c(base);
    SimotaWorkspace w;
    w.class_sum = c.take<float>((size_t)(batch > 0 ? batch : 1) * (size_t)(num_anchors > 0 ? num_anchors : 1));   // S_a, written at region anchors only
    w.cutoff = c.take<unsigned long long>(box_slots(total_gt));                                                   // the boxes' cutoff keys
    w.bytes = c.off;
    return w;
}

extern "C" size_t ssdk_encode_ground_truth_simota_workspace_bytes(int batch, int total_gt, int num_anchors, int n_levels) {
    (void)n_levels;   // (the level table travels by value)
    return carve_simota(nullptr, batch, total_gt, num_anchors).bytes;
}

extern "C" int ssdk_encode_ground_truth_simota(const float* gt_rows, int gt_stride, const int32_t* gt_offsets, int batch, int total_gt,
                                               const float* anchors, int num_anchors, const int32_t* level_sizes, const float* level_strides,
                                               int n_levels, const float* scores, int num_columns, const float* locs, float xy_scale,
                                               float wh_scale, float center_radius, int candidate_topk, float iou_weight, float* target,
                                               int32_t* box_idx, int32_t* dynamic_k, void* workspace, size_t workspace_bytes, void* stream) {
    const char* entry = "ssdk_encode_ground_truth_simota";
    const SimotaWorkspace w = carve_simota(workspace, batch, total_gt, num_anchors);
    int e = check_encode_args(entry, gt_rows, gt_stride, gt_offsets, batch, total_gt, anchors, num_anchors, target, level_sizes && level_strides,
                              kBatchLimitOnly);
    if (e != SSDK_OK) return e;
    if ((e = check_prediction_args(entry, anchors, scores, num_columns, locs)) != SSDK_OK) return e;
    SSDK_REQUIRE(candidate_topk >= 1 && candidate_topk <= SSDK_SIMOTA_MAX_TOPK, SSDK_E_INVALID, "%s: candidate_topk=%d outside 1..%d", entry,
                 candidate_topk, SSDK_SIMOTA_MAX_TOPK);
    SSDK_REQUIRE(center_radius > 0.0f && center_radius <= FLT_MAX, SSDK_E_INVALID, "%s: center_radius=%g must be finite and positive", entry,
                 (double)center_radius);
    SSDK_REQUIRE(iou_weight >= 0.0f && iou_weight <= FLT_MAX, SSDK_E_INVALID, "%s: iou_weight=%g must be finite and not negative", entry,
                 (double)iou_weight);
    SimotaLevels lv = {};
    if ((e = build_levels(entry, level_sizes, n_levels, num_anchors, lv.lv)) != SSDK_OK) return e;
    for (int l = 0; l < n_levels; ++l) {
        const float sx = level_strides[2 * l], sy = level_strides[2 * l + 1];
        SSDK_REQUIRE(sx > 0.0f && sx <= FLT_MAX && sy > 0.0f && sy <= FLT_MAX, SSDK_E_INVALID,
                     "%s: level_strides[%d]=(%g, %g) must be finite and positive", entry, l, (double)sx, (double)sy);
        const volatile float rx = center_radius * sx, ry = center_radius * sy;   // rule 2: one fp32 product each
        lv.rx[l] = rx;
        lv.ry[l] = ry;
    }
    if ((e = check_workspace(entry, workspace, workspace_bytes, w.bytes)) != SSDK_OK) return e;
    hipStream_t s = (hipStream_t)stream;
    SimotaParams sp;
    sp.xy_scale = xy_scale; sp.wh_scale = wh_scale; sp.iou_weight = iou_weight; sp.C = num_columns;
    dim3 grid(cdiv(num_anchors, kAssignThreads), batch);
    if (total_gt > 0) {
        hipLaunchKernelGGL(simota_class_sum_kernel, grid, dim3(kAssignThreads), 0, s, gt_rows, gt_stride, gt_offsets, (const float4*)anchors,
                           num_anchors, lv, scores, num_columns, w.class_sum);
        SSDK_CHECK_LAUNCH("simota_class_sum_kernel");
        hipLaunchKernelGGL(simota_candidates_kernel, dim3(total_gt), dim3(kSimotaThreads), 0, s, gt_rows, gt_stride, gt_offsets, batch,
                           (const float4*)anchors, num_anchors, lv, scores, (const float4*)locs, w.class_sum, sp, candidate_topk, w.cutoff,
                           dynamic_k);
        SSDK_CHECK_LAUNCH("simota_candidates_kernel");
    }
    hipLaunchKernelGGL(simota_assign_kernel, grid, dim3(kAssignThreads), 0, s, gt_rows, gt_stride, gt_offsets, (const float4*)anchors, num_anchors, lv,
                       scores, (const float4*)locs, w.class_sum, sp, w.cutoff, target, box_idx);
    SSDK_CHECK_LAUNCH("simota_assign_kernel");
    return SSDK_OK;
}
