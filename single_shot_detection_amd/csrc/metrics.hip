// metrics.hip -- mean average precision on the device.
//
// Reference: detection/metrics/mean_average_precision.py:10-116 -- a Python loop over every prediction in descending score
// order (one box_utils.iou call, several .item() syncs and dict updates per prediction), then per class a Python loop for the
// running maximum of the precision.  bf/eval.py:63-69 moves all predictions to the host first.
//
// Here: two stable radix sorts (radix_* kernels below: 8-bit digits, per-tile digit histograms -> row scans -> stable scatter with
// wave-level ballot matching) give the predictions in (class, score desc) order -- the order of the
// per-class cumulative counts -- and in (image, class, score desc) order, in which the greedy matching of :47-70 is
// independent between (image, class) groups: one thread walks one group, against the <= G_i ground truths of that image.
// A workgroup per class then does the cumulative sums, precision / recall, the reverse NaN-propagating running maximum and
// the area / 11-point integration with block scans (common.h), in fp32 like the reference's tensors.
#include "common.h"

namespace ssdk {

constexpr int kMapThreads = 256;

struct MapWs {
    unsigned long long* key_a;   // [n]
    unsigned long long* key_b;   // [n]  sorted (class, score) keys -- read by map_ap_kernel
    unsigned long long* key_c;   // [n]  sorted image keys (scratch)
    unsigned* val_a;             // [n]
    unsigned* val_b;             // [n]
    unsigned* perm_b;            // [n]  prediction row at position j of the (class, score desc) order
    unsigned char* flag;         // [n]  by prediction row: 0 = neither, 1 = true positive, 2 = false positive
    unsigned char* matched;      // [total_gt]
    float* prec;                 // [n]  by (class, score) position
    float* rec;                  // [n]
    int* total_positive;         // [num_classes]
    unsigned* table;             // [256][kSortMaxBlocks] per-tile digit counts, then their row-wise exclusive scans
    unsigned* digit_total;       // [256]
    size_t total;
};

constexpr int kSortThreads = 256;
constexpr int kSortMaxBlocks = 4096;   // tiles of a sort pass (the tile grows with n beyond 4096 * 4096 keys)

static MapWs carve_map(void* base, long long n, long long total_gt, int num_classes) {
    Carver c(base);
    MapWs w;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    w.key_a = c.take<unsigned long long>(nn);
    w.key_b = c.take<unsigned long long>(nn);
    w.key_c = c.take<unsigned long long>(nn);
    w.val_a = c.take<unsigned>(nn);
    w.val_b = c.take<unsigned>(nn);
    w.perm_b = c.take<unsigned>(nn);
    w.flag = c.take<unsigned char>(nn);
    w.matched = c.take<unsigned char>((size_t)(total_gt > 0 ? total_gt : 1));
    w.prec = c.take<float>(nn);
    w.rec = c.take<float>(nn);
    w.total_positive = c.take<int>((size_t)num_classes);
    w.table = c.take<unsigned>((size_t)256 * kSortMaxBlocks);
    w.digit_total = c.take<unsigned>(256);
    w.total = c.off;
    return w;
}

// order-preserving map of a float onto unsigned, inverted: ascending key = descending score.  -0.0 + 0.0 = +0.0: the two zeros compare
// equal in the reference's sort (and the oracle's), so they share one key and fall back to row order
__device__ __forceinline__ unsigned desc_key(float s) {
    const unsigned u = __float_as_uint(s + 0.0f);
    return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

// keys of the (class, score desc) order; counted ground truths per class (:27-35)
__global__ void map_prepare_kernel(const float* __restrict__ pred, long long n, const float* __restrict__ gt, int gstride, long long total_gt,
                                   int num_classes, unsigned long long* key, unsigned* val, int* total_positive) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int c = (int)pred[i * 7 + 5];
        const bool ok = c >= 0 && c < num_classes;
        key[i] = ok ? ((unsigned long long)(unsigned)c << 32) | desc_key(pred[i * 7 + 6])
                    : ((unsigned long long)(unsigned)num_classes << 32) | 0xFFFFFFFFull;                        // foreign classes sort last
        val[i] = (unsigned)i;
    }
    if (i < total_gt) {
        const int c = (int)gt[i * gstride + 4];
        if (c >= 0 && c < num_classes && (gstride <= 6 || gt[i * gstride + 6] == 0.0f)) atomicAdd(&total_positive[c], 1);
    }
}

// second sort key: the image of the prediction at position j of the (class, score) order
__global__ void map_image_key_kernel(const float* __restrict__ pred, long long n, const unsigned* __restrict__ perm_b, unsigned long long* key,
                                     unsigned* val) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned r = perm_b[j];
    key[j] = (unsigned long long)(unsigned)(int)pred[(long long)r * 7];
    val[j] = r;
}

// greedy matching (:47-70): the thread at the head of an (image, class) group walks the group in score order
__global__ void map_match_kernel(const float* __restrict__ pred, long long n, const unsigned* __restrict__ perm_a, const float* __restrict__ gt,
                                 int gstride, const int* __restrict__ gt_off, int num_images, int num_classes, float thr,
                                 unsigned char* matched, unsigned char* flag) {
    const long long j0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j0 >= n) return;
    const float* p0 = pred + (long long)perm_a[j0] * 7;
    const int id = (int)p0[0], c = (int)p0[5];
    if (c < 0 || c >= num_classes) { flag[perm_a[j0]] = 0; return; }
    if (j0 > 0) {
        const float* q = pred + (long long)perm_a[j0 - 1] * 7;
        if ((int)q[0] == id && (int)q[5] == c) return;   // not the head of its group
    }
    const bool ignore_difficult = gstride > 6;
    const int g_begin = (id >= 0 && id < num_images) ? gt_off[id] : 0, g_end = (id >= 0 && id < num_images) ? gt_off[id + 1] : 0;
    for (long long j = j0; j < n; ++j) {
        const unsigned row = perm_a[j];
        const float* p = pred + (long long)row * 7;
        if ((int)p[0] != id || (int)p[5] != c) break;
        const float4 pb = make_float4(p[1], p[2], p[3], p[4]);
        const float parea = area4(pb.x, pb.y, pb.z, pb.w);
        bool have = false;
        int best_g = -1;
        float best = 0.0f;
        for (int g = g_begin; g < g_end; ++g) {
            const float* q = gt + (long long)g * gstride;
            if ((int)q[4] != c) continue;
            const float4 qb = make_float4(q[0], q[1], q[2], q[3]);
            const float v = iou_corner(pb, parea, qb, area4(qb.x, qb.y, qb.z, qb.w));
            if (!have || (v > best && best == best) || (v != v && best == best)) { best = v; best_g = g; }   // first max, NaN propagates
            have = true;
        }
        unsigned char f = 2;                                                        // :54-56, :68: false positive
        if (have && best > thr) {                                                   // :60
            if (!ignore_difficult || gt[(long long)best_g * gstride + 6] == 0.0f) { // :61
                if (!matched[best_g]) { matched[best_g] = 1; f = 1; }              // :62-64
            } else {
                f = 0;                                                              // difficult hit: neither counter moves
            }
        }
        flag[row] = f;
    }
}

struct OpTmax { __device__ __forceinline__ float operator()(float a, float b) const { return tmaxf(a, b); } };

// one workgroup per class: cumulative counts -> precision / recall -> reverse running max -> AP (:77-108)
__global__ void __launch_bounds__(kMapThreads) map_ap_kernel(const unsigned long long* __restrict__ key_b, const unsigned* __restrict__ perm_b, long long n,
                                                             const unsigned char* __restrict__ flag, const int* __restrict__ total_positive, int voc,
                                                             float* prec, float* rec, float* ap_out) {
    __shared__ unsigned long long s_scan_i[17];   // (tp, fp) counts packed as two 32-bit halves
    __shared__ float s_scan_f[17];
    __shared__ long long s_range[2];
    __shared__ int s_cnt[11];
    __shared__ float s_vocp[11];
    __shared__ float s_carry_f;

    const int c = blockIdx.x, tid = threadIdx.x;
    const int tot_i = total_positive[c];
    if (tot_i == 0) {   // class without counted ground truth: not part of the mean (:74-75, :80)
        if (tid == 0) ap_out[c] = __uint_as_float(0x7FC00000u);
        return;
    }
    if (tid < 2) {      // segment of this class in the (class, score) order: lower bounds of c << 32 and (c + 1) << 32
        const unsigned long long want = (unsigned long long)(unsigned)(c + tid) << 32;
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (key_b[mid] < want) lo = mid + 1; else hi = mid;
        }
        s_range[tid] = lo;
    }
    if (tid < 11) { s_cnt[tid] = 0; s_vocp[tid] = 0.0f; }
    __syncthreads();
    const long long begin = s_range[0], m = s_range[1] - s_range[0];
    const float tot = (float)tot_i;
    if (m == 0) {       // no prediction of this class: tp = [0], fp = [1] (:81-89) -> AP = 0 either way
        if (tid == 0) ap_out[c] = 0.0f;
        return;
    }
    float thr[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) thr[k] = (float)(0.0 + k * 0.1);   // torch.arange(0, 1.1, .1)
    int my_cnt[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) my_cnt[k] = 0;

    // pass 1, forward: cumulative (tp, fp) -> precision, recall
    int2 carry = make_int2(0, 0);
    struct AddU64 { __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; } };
    for (long long base = 0; base < m; base += kMapThreads) {
        const long long i = base + tid;
        unsigned long long v = 0ull;   // tp in the low half, fp in the high half (a class has < 2^31 predictions: no carry between them)
        if (i < m) {
            const unsigned char f = flag[perm_b[begin + i]];
            v = (unsigned long long)(f == 1) | ((unsigned long long)(f == 2) << 32);
        }
        unsigned long long aggv;
        const unsigned long long inclv = block_inclusive_scan(v, AddU64(), s_scan_i, &aggv);
        const int2 incl = make_int2((int)(unsigned)inclv, (int)(unsigned)(inclv >> 32)), agg = make_int2((int)(unsigned)aggv, (int)(unsigned)(aggv >> 32));
        __syncthreads();
        if (i < m) {
            const float tp = (float)(carry.x + incl.x), fp = (float)(carry.y + incl.y);
            const float p = tp / (tp + fp), r = tp / tot;      // :91, :97
            prec[begin + i] = p;
            rec[begin + i] = r;
#pragma unroll
            for (int k = 0; k < 11; ++k) my_cnt[k] += thr[k] > r;
        }
        carry = make_int2(carry.x + agg.x, carry.y + agg.y);
    }
    if (voc) {
#pragma unroll
        for (int k = 0; k < 11; ++k)
            if (my_cnt[k]) atomicAdd(&s_cnt[k], my_cnt[k]);
    }
    if (tid == 0) s_carry_f = 0.0f;   // precision[m] = 0 (:92)
    __syncthreads();

    // pass 2, backward: running maximum (:94-95), then the integral
    float acc = 0.0f;
    const long long chunks = (m + kMapThreads - 1) / kMapThreads;
    for (long long ch = chunks - 1; ch >= 0; --ch) {
        // thread t handles position i = ch * T + (T - 1 - t): scanning t upwards walks i downwards
        const long long i = ch * kMapThreads + (kMapThreads - 1 - tid);
        const float neg_inf = __uint_as_float(0xFF800000u);
        float v = i < m ? prec[begin + i] : neg_inf;
        const float incl = block_inclusive_scan(v, OpTmax(), s_scan_f, (float*)nullptr);
        const float carry_f = s_carry_f;
        __syncthreads();
        const float pm = tmaxf(incl, carry_f);
        if (i < m) {
            if (voc) {
#pragma unroll
                for (int k = 0; k < 11; ++k)
                    if ((long long)s_cnt[k] == i) s_vocp[k] = pm;
            } else {
                const float r = rec[begin + i], r_prev = i > 0 ? rec[begin + i - 1] : 0.0f;
                acc += (r - r_prev) * pm;                         // (recall[1:] - recall[:-1]) . precision (:105-106)
            }
        }
        if (tid == kMapThreads - 1) s_carry_f = pm;               // lowest position of the chunk
        __syncthreads();
    }
    if (voc) {
        if (tid == 0) {
            float s = 0.0f;
            for (int k = 0; k < 11; ++k) s += s_vocp[k];          // indexes == m select precision[m] = 0 (s_vocp stays 0)
            ap_out[c] = s / 11.0f;
        }
    } else {
        // the last term (1 - recall[m-1]) * precision[m] is (finite) * 0
        const float sum = block_sum(acc, s_scan_f);
        if (tid == 0) ap_out[c] = sum;
    }
}

// ---- stable LSD radix sort of (64-bit key, 32-bit value) pairs, 8 bits per pass ---------------------------------------------------
// Pass = three launches.  radix_hist: every tile (a contiguous run of `tile` keys, one workgroup) counts its digits -> table[digit][tile].
// radix_rowscan: one workgroup per digit turns its row into exclusive prefixes (and the row total).  radix_scatter: a tile's four waves
// own four contiguous quarters of it; a key's slot = (keys with a smaller digit anywhere) + (same digit in earlier tiles) + (same digit
// in earlier waves of the tile) + (same digit earlier in the wave's walk), the last found 64 keys at a time by ballot matching -- every
// term follows input order, so the sort is stable (equal scores keep the lower prediction row first, like the oracle's stable sort).
struct SortPass {
    const unsigned long long* kin;
    unsigned long long* kout;
    const unsigned* vin;
    unsigned* vout;
    long long n;
    int shift, tile, nblocks;
    unsigned mask;          // 255, or fewer low bits for the top digit when end_bit is no multiple of 8: key bits >= end_bit are ignored
    unsigned* table;        // [256][nblocks]
    unsigned* digit_total;  // [256]
};

__global__ void __launch_bounds__(kSortThreads) radix_hist_kernel(SortPass a) {
    __shared__ unsigned s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const long long b0 = (long long)blockIdx.x * a.tile, b1 = min(a.n, b0 + a.tile);
    for (long long i = b0 + threadIdx.x; i < b1; i += kSortThreads) atomicAdd(&s_hist[(unsigned)(a.kin[i] >> a.shift) & a.mask], 1u);
    __syncthreads();
    a.table[(size_t)threadIdx.x * a.nblocks + blockIdx.x] = s_hist[threadIdx.x];
}

__global__ void __launch_bounds__(kSortThreads) radix_rowscan_kernel(SortPass a) {
    __shared__ unsigned s_tmp[17];
    unsigned* row = a.table + (size_t)blockIdx.x * a.nblocks;
    struct AddU { __device__ __forceinline__ unsigned operator()(unsigned x, unsigned y) const { return x + y; } };
    unsigned carry = 0;
    for (int base = 0; base < a.nblocks; base += kSortThreads) {
        const int i = base + threadIdx.x;
        const unsigned v = i < a.nblocks ? row[i] : 0u;
        unsigned agg;
        const unsigned incl = block_inclusive_scan(v, AddU(), s_tmp, &agg);
        if (i < a.nblocks) row[i] = carry + incl - v;
        carry += agg;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.digit_total[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kSortThreads) radix_scatter_kernel(SortPass a) {
    __shared__ unsigned s_base[256];        // keys with a smaller digit + same digit in earlier tiles
    __shared__ volatile unsigned s_wcnt[4][256];   // per wave: its digit counts, then its running slots (volatile: lanes of a wave hand
                                                   // the slot of a digit to each other through it from one 64-key round to the next)
    __shared__ unsigned s_tmp[17];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    struct AddU { __device__ __forceinline__ unsigned operator()(unsigned x, unsigned y) const { return x + y; } };
    {
        const unsigned t = a.digit_total[tid];
        const unsigned incl = block_inclusive_scan(t, AddU(), s_tmp, (unsigned*)nullptr);
        s_base[tid] = incl - t + a.table[(size_t)tid * a.nblocks + blockIdx.x];
    }
    for (int w = 0; w < 4; ++w) s_wcnt[w][tid] = 0;
    __syncthreads();
    const long long b0 = (long long)blockIdx.x * a.tile, b1 = min(a.n, b0 + a.tile);
    const long long quarter = a.tile / 4;
    const long long w0 = b0 + wave * quarter, w1 = min(b1, w0 + quarter);
    for (long long i = w0 + lane; i < w1; i += kWave) atomicAdd(const_cast<unsigned*>(&s_wcnt[wave][(unsigned)(a.kin[i] >> a.shift) & a.mask]), 1u);
    __syncthreads();
    {   // thread d: the four waves' starting slots for digit d
        unsigned run = s_base[tid];
        for (int w = 0; w < 4; ++w) { const unsigned c = s_wcnt[w][tid]; s_wcnt[w][tid] = run; run += c; }
    }
    __syncthreads();
    for (long long i0 = w0; i0 < w1; i0 += kWave) {
        const long long i = i0 + lane;
        const bool valid = i < w1;
        const unsigned long long key = valid ? a.kin[i] : 0ull;
        const unsigned d = (unsigned)(key >> a.shift) & a.mask;
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long bal = __ballot(one);
            m &= one ? bal : ~bal;
        }
        const int rank = __popcll(m & ((1ull << lane) - 1ull)), cnt = __popcll(m);
        if (valid) {
            const unsigned pos = s_wcnt[wave][d] + (unsigned)rank;
            a.kout[pos] = key;
            a.vout[pos] = a.vin[i];
        }
        __builtin_amdgcn_wave_barrier();   // (every lane has read its digit's slot before the group's last lane moves it on)
        if (valid && rank == cnt - 1) s_wcnt[wave][d] = s_wcnt[wave][d] + (unsigned)cnt;
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ void map_mean_kernel(const float* __restrict__ ap, const int* __restrict__ total_positive, int num_classes, double* map_out) {
    if (threadIdx.x || blockIdx.x) return;
    double s = 0.0;
    int cnt = 0;
    for (int c = 0; c < num_classes; ++c)
        if (total_positive[c]) { s += (double)ap[c]; ++cnt; }   // :111 (python floats)
    *map_out = cnt ? s / cnt : (double)__uint_as_float(0x7FC00000u);
}

}  // namespace ssdk

using namespace ssdk;

// stable sort of n (key, value) pairs on key bits [0, end_bit); the result lands in kb / vb.  ka / va are overwritten.
static int radix_sort_pairs(unsigned long long* ka, unsigned long long* kb, unsigned* va, unsigned* vb, long long n, int end_bit, unsigned* table,
                            unsigned* digit_total, hipStream_t s) {
    SortPass a;
    a.n = n;
    long long tile = 4096;
    while ((n + tile - 1) / tile > kSortMaxBlocks) tile *= 2;
    a.tile = (int)tile;
    a.nblocks = (int)((n + tile - 1) / tile);
    a.table = table;
    a.digit_total = digit_total;
    const int digits = (end_bit + 7) / 8;
    // pass p reads a (p even) or b (p odd) and writes the other: an odd number of passes ends in kb / vb.  With an even number of digits
    // the most significant one is sorted once more -- a stable sort by a digit the data is already ordered by is a copy.
    const int passes = (digits & 1) ? digits : digits + 1;
    for (int p = 0; p < passes; ++p) {
        a.shift = 8 * (p < digits ? p : digits - 1);
        a.mask = (a.shift + 8 > end_bit) ? (1u << (end_bit - a.shift)) - 1u : 255u;
        a.kin = (p & 1) ? kb : ka; a.kout = (p & 1) ? ka : kb;
        a.vin = (p & 1) ? vb : va; a.vout = (p & 1) ? va : vb;
        hipLaunchKernelGGL(radix_hist_kernel, dim3(a.nblocks), dim3(kSortThreads), 0, s, a);
        SSDK_CHECK_LAUNCH("radix_hist_kernel");
        hipLaunchKernelGGL(radix_rowscan_kernel, dim3(256), dim3(kSortThreads), 0, s, a);
        SSDK_CHECK_LAUNCH("radix_rowscan_kernel");
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(a.nblocks), dim3(kSortThreads), 0, s, a);
        SSDK_CHECK_LAUNCH("radix_scatter_kernel");
    }
    return SSDK_OK;
}

extern "C" size_t ssdk_mean_average_precision_workspace_bytes(long long n_pred, long long total_gt, int num_classes) {
    if (n_pred < 0 || total_gt < 0 || num_classes <= 0) return 0;
    return carve_map(nullptr, n_pred, total_gt, num_classes).total;
}

// the u64 / u32 pair sort on its own: keys and vals are staged in the workspace (radix_sort_pairs overwrites its input buffers), so the
// caller's inputs stay as they were and may even be the outputs
struct SortWs { unsigned long long* key; unsigned* val; unsigned* table; unsigned* digit_total; size_t total; };
static SortWs carve_sort(void* base, long long n) {
    Carver c(base);
    SortWs w;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    w.key = c.take<unsigned long long>(nn);
    w.val = c.take<unsigned>(nn);
    w.table = c.take<unsigned>((size_t)256 * kSortMaxBlocks);
    w.digit_total = c.take<unsigned>(256);
    w.total = c.off;
    return w;
}

extern "C" size_t ssdk_sort_pairs_u64_workspace_bytes(long long n) {
    if (n < 0 || n >= (1LL << 31)) return 0;
    return carve_sort(nullptr, n).total;
}

extern "C" int ssdk_sort_pairs_u64(const uint64_t* keys, const uint32_t* vals, long long n, int end_bit, uint64_t* keys_out, uint32_t* vals_out,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long) && sizeof(uint32_t) == sizeof(unsigned), "key / value widths");
    SSDK_REQUIRE(n >= 0 && n < (1LL << 31) && end_bit >= 1 && end_bit <= 64, SSDK_E_INVALID, "ssdk_sort_pairs_u64: n=%lld end_bit=%d (0 <= n < 2^31, 1 <= end_bit <= 64)", n,
                 end_bit);
    SSDK_REQUIRE(n == 0 || (keys && vals && keys_out && vals_out), SSDK_E_INVALID, "ssdk_sort_pairs_u64: null pointer");
    const SortWs w = carve_sort(workspace, n);
    SSDK_REQUIRE(workspace && workspace_bytes >= w.total, SSDK_E_WORKSPACE, "ssdk_sort_pairs_u64: workspace %zu < %zu bytes", workspace_bytes, w.total);
    if (n == 0) return SSDK_OK;
    hipStream_t s = (hipStream_t)stream;
    SSDK_CHECK_HIP(hipMemcpyAsync(w.key, keys, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToDevice, s));
    SSDK_CHECK_HIP(hipMemcpyAsync(w.val, vals, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToDevice, s));
    return radix_sort_pairs(w.key, reinterpret_cast<unsigned long long*>(keys_out), w.val, vals_out, n, end_bit, w.table, w.digit_total, s);
}

extern "C" int ssdk_mean_average_precision(const float* predictions, long long n_pred, const float* gt_rows, int gt_stride,
                                           const int* gt_offsets, int num_images, long long total_gt, int num_classes,
                                           float iou_threshold, int voc, float* ap_out, double* map_out, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    return ssdk_mean_average_precision_ex(predictions, n_pred, gt_rows, gt_stride, gt_offsets, num_images, total_gt, num_classes, iou_threshold, voc, ap_out,
                                          map_out, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int ssdk_mean_average_precision_ex(const float* predictions, long long n_pred, const float* gt_rows, int gt_stride,
                                              const int* gt_offsets, int num_images, long long total_gt, int num_classes,
                                              float iou_threshold, int voc, float* ap_out, double* map_out, uint32_t* order_out,
                                              uint8_t* outcome_out, void* workspace, size_t workspace_bytes, void* stream) {
    SSDK_REQUIRE(n_pred >= 0 && n_pred < (1LL << 31) && total_gt >= 0 && total_gt < (1LL << 31) && num_images >= 0 && num_classes > 0 && num_classes < (1 << 20),
                 SSDK_E_INVALID, "ssdk_mean_average_precision: n_pred=%lld total_gt=%lld num_images=%d num_classes=%d", n_pred, total_gt, num_images, num_classes);
    SSDK_REQUIRE(gt_stride >= 5 && gt_offsets && ap_out && map_out && (n_pred == 0 || predictions) && (total_gt == 0 || gt_rows), SSDK_E_INVALID,
                 "ssdk_mean_average_precision: null pointer or gt_stride=%d < 5", gt_stride);
    MapWs w = carve_map(workspace, n_pred, total_gt, num_classes);
    SSDK_REQUIRE(workspace && workspace_bytes >= w.total, SSDK_E_WORKSPACE, "ssdk_mean_average_precision: workspace %zu < %zu bytes", workspace_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    SSDK_CHECK_HIP(zero_async(w.total_positive, sizeof(int) * (size_t)num_classes, s));
    SSDK_CHECK_HIP(zero_async(w.matched, (size_t)(total_gt > 0 ? total_gt : 1), s));
    const long long work = n_pred > total_gt ? n_pred : total_gt;
    if (work > 0) {
        hipLaunchKernelGGL(map_prepare_kernel, dim3((unsigned)cdiv((int)work, 256)), dim3(256), 0, s, predictions, n_pred, gt_rows, gt_stride, total_gt, num_classes,
                           w.key_a, w.val_a, w.total_positive);
        SSDK_CHECK_LAUNCH("map_prepare_kernel");
    }
    if (n_pred > 0) {
        const int n = (int)n_pred;
        int class_bits = 1;
        while ((1 << class_bits) <= num_classes) ++class_bits;   // keys go up to num_classes << 32 (foreign classes)
        // (class, score desc): stable, so equal scores keep the lower row first
        int rc = radix_sort_pairs(w.key_a, w.key_b, w.val_a, w.perm_b, n_pred, 32 + class_bits, w.table, w.digit_total, s);
        if (rc) return rc;
        hipLaunchKernelGGL(map_image_key_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, predictions, n_pred, w.perm_b, w.key_a, w.val_a);
        SSDK_CHECK_LAUNCH("map_image_key_kernel");
        // stable sort by image on top: (image, class, score desc); val_b = prediction rows in that order
        rc = radix_sort_pairs(w.key_a, w.key_c, w.val_a, w.val_b, n_pred, 32, w.table, w.digit_total, s);
        if (rc) return rc;
        hipLaunchKernelGGL(map_match_kernel, dim3((unsigned)cdiv(n, 128)), dim3(128), 0, s, predictions, n_pred, w.val_b, gt_rows, gt_stride, gt_offsets, num_images,
                           num_classes, iou_threshold, w.matched, w.flag);
        SSDK_CHECK_LAUNCH("map_match_kernel");
        if (order_out) SSDK_CHECK_HIP(hipMemcpyAsync(order_out, w.perm_b, sizeof(unsigned) * (size_t)n_pred, hipMemcpyDeviceToDevice, s));
        if (outcome_out) SSDK_CHECK_HIP(hipMemcpyAsync(outcome_out, w.flag, (size_t)n_pred, hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(map_ap_kernel, dim3((unsigned)num_classes), dim3(kMapThreads), 0, s, w.key_b, w.perm_b, n_pred, w.flag, w.total_positive, voc, w.prec, w.rec, ap_out);
    SSDK_CHECK_LAUNCH("map_ap_kernel");
    hipLaunchKernelGGL(map_mean_kernel, dim3(1), dim3(64), 0, s, ap_out, w.total_positive, num_classes, map_out);
    SSDK_CHECK_LAUNCH("map_mean_kernel");
    return SSDK_OK;
}

// ---- device-resident input side: mixup (bf/core/batch_container.py:25-45) ----------------------------------------------
namespace ssdk {

// HBM-bound: 2 reads + 1 write of 16 B per lane for mixed images, a plain copy for the others
__global__ void mixup_images_kernel(const float4* __restrict__ in, float4* __restrict__ out, long long per_image4, const int* __restrict__ index,
                                    const unsigned char* __restrict__ roll, float lam, float oml) {
    const int b = blockIdx.y;
    const bool mix = roll[b] != 0;
    const float4* a = in + (long long)b * per_image4;
    const float4* o = in + (long long)index[b] * per_image4;
    float4* d = out + (long long)b * per_image4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per_image4; i += (long long)gridDim.x * blockDim.x) {
        float4 v = a[i];
        if (mix) {
            const float4 w = o[i];   // (this TU is built -ffp-contract=off: multiply and add round separately, like the two torch ops)
            v = make_float4(lam * v.x + oml * w.x, lam * v.y + oml * w.y, lam * v.z + oml * w.z, lam * v.w + oml * w.w);
        }
        d[i] = v;
    }
}
__global__ void mixup_images_tail_kernel(const float* __restrict__ in, float* __restrict__ out, long long per_image, long long done, const int* __restrict__ index,
                                         const unsigned char* __restrict__ roll, float lam, float oml) {
    const int b = blockIdx.y;
    const long long i = done + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_image) return;
    const float v = in[(long long)b * per_image + i];
    out[(long long)b * per_image + i] = roll[b] ? lam * v + oml * in[(long long)index[b] * per_image + i] : v;
}

// one workgroup: offsets by a serial scan over the (small) batch, then the row copies
__global__ void mixup_gt_kernel(const float* __restrict__ rows_in, int stride, const int* __restrict__ off_in, int batch, const int* __restrict__ index,
                                const unsigned char* __restrict__ roll, float lam, float oml, float* __restrict__ rows_out, int* __restrict__ off_out) {
    extern __shared__ int s_off[];
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int b = 0; b < batch; ++b) {
            s_off[b] = acc;
            acc += (off_in[b + 1] - off_in[b]) + (roll[b] ? off_in[index[b] + 1] - off_in[index[b]] : 0);
        }
        s_off[batch] = acc;
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= batch; b += blockDim.x) off_out[b] = s_off[b];
    for (int b = 0; b < batch; ++b) {
        const int own = off_in[b + 1] - off_in[b];
        const int other = roll[b] ? off_in[index[b] + 1] - off_in[index[b]] : 0;
        const int total = (own + other) * stride;
        for (int e = threadIdx.x; e < total; e += blockDim.x) {
            const int r = e / stride, c = e % stride;
            const bool second = r >= own;
            float v = second ? rows_in[(long long)(off_in[index[b]] + r - own) * stride + c] : rows_in[(long long)(off_in[b] + r) * stride + c];
            if (c == 5 && roll[b]) v *= second ? oml : lam;   // :38, :40 (SCORE_INDEX)
            rows_out[(long long)(s_off[b] + r) * stride + c] = v;
        }
    }
}

}  // namespace ssdk

extern "C" int ssdk_mixup_images(const float* in, float* out, int batch, long long per_image, const int* index, const unsigned char* roll,
                                 double lam, void* stream) {
    SSDK_REQUIRE(in && out && index && roll && batch > 0 && batch <= 65535 && per_image > 0 && in != out, SSDK_E_INVALID,
                 "ssdk_mixup_images: batch=%d per_image=%lld (out-of-place only)", batch, per_image);
    hipStream_t s = (hipStream_t)stream;
    const float lam_f = (float)lam, oml_f = (float)(1.0 - lam);
    const bool vec = (per_image % 4 == 0) && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    if (vec) {
        const long long n4 = per_image / 4;
        const unsigned gx = (unsigned)(n4 / 256 / 4 > 0 ? (n4 / 256 / 4 < 1024 ? n4 / 256 / 4 : 1024) : 1);
        hipLaunchKernelGGL(mixup_images_kernel, dim3(gx, (unsigned)batch), dim3(256), 0, s, reinterpret_cast<const float4*>(in), reinterpret_cast<float4*>(out), n4, index,
                           roll, lam_f, oml_f);
    } else {
        hipLaunchKernelGGL(mixup_images_tail_kernel, dim3((unsigned)((per_image + 255) / 256), (unsigned)batch), dim3(256), 0, s, in, out, per_image, 0LL, index, roll,
                           lam_f, oml_f);
    }
    SSDK_CHECK_LAUNCH("mixup_images_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_mixup_ground_truth(const float* rows_in, int gt_stride, const int* offsets_in, int batch, const int* index,
                                       const unsigned char* roll, double lam, float* rows_out, int* offsets_out, void* stream) {
    SSDK_REQUIRE(offsets_in && index && roll && rows_out && offsets_out && batch > 0 && batch <= 8192 && gt_stride >= 6, SSDK_E_INVALID,
                 "ssdk_mixup_ground_truth: batch=%d gt_stride=%d", batch, gt_stride);
    hipLaunchKernelGGL(mixup_gt_kernel, dim3(1), dim3(256), sizeof(int) * (size_t)(batch + 1), (hipStream_t)stream, rows_in, gt_stride, offsets_in, batch, index, roll,
                       (float)lam, (float)(1.0 - lam), rows_out, offsets_out);
    SSDK_CHECK_LAUNCH("mixup_gt_kernel");
    return SSDK_OK;
}

// ---- COCO-style bbox evaluation: AP@[.50:.95], area bins, AR (include/ssdk.h, ABI 131) ---------------------------------
// Three stable sorts give the predictions in (class, score desc, image, row) order -- the order of the per-class cumulative counts --
// and in (image, class, score desc, row) order, in which the greedy matching is independent between (image, class) groups.  One
// wavefront walks one group: lane l < T * A owns the pair (t, a) = (l / A, l % A) and carries its own matched-gt state.  One workgroup
// per (class, area, max_dets) turns the outcomes into recall[T, K, A, M] and precision[T, R, K, A, M]; twelve small workgroups write
// the summary.  All arithmetic is fp64 from the fp32 coordinates, every operation rounded on its own (-ffp-contract=off).
namespace ssdk {

constexpr int kCocoWaves = 4;          // waves (groups in flight) per workgroup of the matching kernel
constexpr int kCocoMaskGts = 64;       // a group with at most this many gts of its class keeps its matched state in a 64-bit register mask
constexpr int kCocoThreads = 256;
constexpr int kCocoMaxR = 1024, kCocoMaxPairs = 64, kCocoMaxM = 4;

struct CocoWs {
    unsigned long long* key_a;   // [n]
    unsigned long long* key_b;   // [n]  sorted (class, score) keys -- the class segments of the accumulation
    unsigned long long* key_c;   // [n]  sorted image keys of the (image, class, score, row) order
    unsigned* val_a;             // [n]
    unsigned* perm_a;            // [n]  prediction row at position j of the (image, class, score desc, row) order
    unsigned* perm_b;            // [n]  prediction row at position j of the (class, score desc, image, row) order
    unsigned* group_start;       // [n]  first position of every (image, class) group, in no particular order
    int* rank;                   // [n]  by prediction row
    unsigned char* flags;        // [n][T * A] by prediction row: bit 0 = matched, bit 1 = ignored
    unsigned char* gt_matched;   // [total_gt][T * A]  matched state of the groups with more than kCocoMaskGts gts of their class
    int* npig;                   // [K][A], then one word: the number of groups
    unsigned* table;
    unsigned* digit_total;
    size_t total;
};

static CocoWs carve_coco(void* base, long long n, long long total_gt, int num_classes, int pairs, int areas) {
    Carver c(base);
    CocoWs w;
    const size_t nn = (size_t)(n > 0 ? n : 1), ng = (size_t)(total_gt > 0 ? total_gt : 1);
    w.key_a = c.take<unsigned long long>(nn);
    w.key_b = c.take<unsigned long long>(nn);
    w.key_c = c.take<unsigned long long>(nn);
    w.val_a = c.take<unsigned>(nn);
    w.perm_a = c.take<unsigned>(nn);
    w.perm_b = c.take<unsigned>(nn);
    w.group_start = c.take<unsigned>(nn);
    w.rank = c.take<int>(nn);
    w.flags = c.take<unsigned char>(nn * (size_t)pairs);
    w.gt_matched = c.take<unsigned char>(ng * (size_t)pairs);
    w.npig = c.take<int>((size_t)num_classes * areas + 1);
    w.table = c.take<unsigned>((size_t)256 * kSortMaxBlocks);
    w.digit_total = c.take<unsigned>(256);
    w.total = c.off;
    return w;
}

// image ids as sort keys in their signed order; rows == nullptr: the identity
__global__ void coco_image_key_kernel(const float* __restrict__ pred, long long n, const unsigned* __restrict__ rows, unsigned long long* key, unsigned* val) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned r = rows ? rows[j] : (unsigned)j;
    key[j] = (unsigned long long)((unsigned)(int)pred[(long long)r * 7] ^ 0x80000000u);
    val[j] = r;
}

// (class, score desc) keys of the rows in (image, row) order; foreign classes sort last
__global__ void coco_class_key_kernel(const float* __restrict__ pred, long long n, const unsigned* __restrict__ rows, int num_classes, unsigned long long* key,
                                      unsigned* val) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned r = rows[j];
    const int c = (int)pred[(long long)r * 7 + 5];
    const bool ok = c >= 0 && c < num_classes;
    key[j] = ok ? ((unsigned long long)(unsigned)c << 32) | desc_key(pred[(long long)r * 7 + 6]) : ((unsigned long long)(unsigned)num_classes << 32) | 0xFFFFFFFFull;
    val[j] = r;
}

__device__ __forceinline__ double coco_box_area(const float* b) { return ((double)b[2] - (double)b[0]) * ((double)b[3] - (double)b[1]); }

// the area a gt is binned by: the annotation's area when given, the box area otherwise, times the image's scale
__device__ __forceinline__ double coco_gt_range_area(const float* __restrict__ gt, int gstride, long long g, const double* __restrict__ gt_area, double scale) {
    return (gt_area ? gt_area[g] : coco_box_area(gt + g * gstride)) * scale;
}

// npig[k][a]: gts of class k that are not crowd and whose area lies in range a (both ends inclusive), over all images
__global__ void coco_npig_kernel(const float* __restrict__ gt, int gstride, long long total_gt, const int* __restrict__ gt_off, int num_images, int num_classes,
                                 const double* __restrict__ gt_area, const double* __restrict__ image_area_scale, const double* __restrict__ area_rngs, int A,
                                 int* npig) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total_gt) return;
    const float* q = gt + g * gstride;
    const int c = (int)q[4];
    if (c < 0 || c >= num_classes || (gstride > 6 && q[6] != 0.0f)) return;
    int lo = 0, hi = num_images;     // the image of row g: the last i with gt_off[i] <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)gt_off[mid] <= g) lo = mid; else hi = mid;
    }
    const double area = coco_gt_range_area(gt, gstride, g, gt_area, image_area_scale ? image_area_scale[lo] : 1.0);
    for (int a = 0; a < A; ++a)
        if (!(area < area_rngs[2 * a] || area > area_rngs[2 * a + 1])) atomicAdd(&npig[c * A + a], 1);
}

// heads of the (image, class) groups of the (image, class, score, row) order, compacted with one atomic per wave
__global__ void coco_groups_kernel(const float* __restrict__ pred, long long n, const unsigned* __restrict__ perm_a, const unsigned long long* __restrict__ key_c,
                                   unsigned* group_start, int* ngroups) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool head = false;
    if (j < n) head = j == 0 || key_c[j] != key_c[j - 1] || (int)pred[(long long)perm_a[j] * 7 + 5] != (int)pred[(long long)perm_a[j - 1] * 7 + 5];
    const unsigned long long b = __ballot(head);
    if (b == 0ull) return;
    const int lane = lane_id();
    int base = 0;
    if (lane == 0) base = atomicAdd(ngroups, __popcll(b));
    base = __shfl(base, 0, kWave);
    if (head) group_start[base + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned)j;
}

// LDS written by some lanes of a wave and read by others: order the accesses (the wave runs in lockstep; this keeps the compiler from moving them)
__device__ __forceinline__ void coco_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// IoU of detection d against gt q (COCOeval: maskUtils.iou on boxes); a crowd gt divides by the detection's area; 0 / 0 -> 0
__device__ __forceinline__ double coco_iou(const double d[4], double area_d, const float* q, bool crowd) {
    const double gx1 = (double)q[0], gy1 = (double)q[1], gx2 = (double)q[2], gy2 = (double)q[3];
    const double iw = fmin(d[2], gx2) - fmax(d[0], gx1), ih = fmin(d[3], gy2) - fmax(d[1], gy1);
    const double inter = fmax(0.0, iw) * fmax(0.0, ih);
    const double area_g = (gx2 - gx1) * (gy2 - gy1);
    const double den = crowd ? area_d : area_d + area_g - inter;
    return den == 0.0 ? 0.0 : inter / den;
}

// The matching rule of COCOeval.evaluateImg for every (threshold, area range) pair at once: one wave per (image, class) group.
__global__ void __launch_bounds__(kCocoWaves * kWave) coco_match_kernel(
    const float* __restrict__ pred, long long n, const unsigned* __restrict__ perm_a, const unsigned long long* __restrict__ key_c,
    const unsigned* __restrict__ group_start, const int* __restrict__ ngroups_p, const float* __restrict__ gt, int gstride, const int* __restrict__ gt_off,
    int num_images, int num_classes, const double* __restrict__ gt_area, const double* __restrict__ image_area_scale, const double* __restrict__ iou_thrs, int T,
    const double* __restrict__ area_rngs, int A, int max_last, unsigned char* gt_matched, int* rank_out, unsigned char* flags_out) {
    __shared__ float s_box[kCocoWaves][kCocoMaskGts][4];
    __shared__ double s_area[kCocoWaves][kCocoMaskGts];
    __shared__ double s_iou[kCocoWaves][kCocoMaskGts];
    __shared__ unsigned char s_crowd[kCocoWaves][kCocoMaskGts];

    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int TA = T * A;
    const bool has = lane < TA;                      // this lane owns the pair (t, a)
    const int t = has ? lane / A : 0, a = has ? lane % A : 0;
    const double best0 = fmin(iou_thrs[t], 1.0 - 1e-10);
    const double lo = area_rngs[2 * a], hi = area_rngs[2 * a + 1];
    const int ngroups = *ngroups_p;
    const unsigned long long below = (1ull << lane) - 1ull;

    for (int grp = blockIdx.x * kCocoWaves + wave; grp < ngroups; grp += gridDim.x * kCocoWaves) {
        const long long j0 = group_start[grp];
        const long long row0 = perm_a[j0];
        const int id = (int)pred[row0 * 7], c = (int)pred[row0 * 7 + 5];
        const unsigned long long ikey = key_c[j0];
        long long j1 = j0 + 1;                       // end of the group: the first position of another image or class
        for (;;) {
            const long long j = j1 + lane;
            const bool same = j < n && key_c[j] == ikey && (int)pred[(long long)perm_a[j] * 7 + 5] == c;
            const unsigned long long b = __ballot(!same);
            if (b) { j1 += __ffsll((long long)b) - 1; break; }
            j1 += kWave;
        }
        if (c < 0 || c >= num_classes) {             // a foreign class takes part in nothing
            for (long long j = j0 + lane; j < j1; j += kWave) {
                const long long row = perm_a[j];
                rank_out[row] = -1;
                for (int p = 0; p < TA; ++p) flags_out[row * TA + p] = 0;
            }
            continue;
        }
        const bool in_range = id >= 0 && id < num_images;
        const int g_begin = in_range ? gt_off[id] : 0, g_end = in_range ? gt_off[id + 1] : 0;
        const double scale = (in_range && image_area_scale) ? image_area_scale[id] : 1.0;

        // the gts of class c of this image, in row order: staged in LDS while they fit the register mask
        int cnt = 0;
        for (int base = g_begin; base < g_end; base += kWave) {
            const int g = base + lane;
            const bool mine = g < g_end && (int)gt[(long long)g * gstride + 4] == c;
            const unsigned long long b = __ballot(mine);
            const int pos = cnt + __popcll(b & below);
            if (mine && pos < kCocoMaskGts) {
                const float* q = gt + (long long)g * gstride;
                s_box[wave][pos][0] = q[0]; s_box[wave][pos][1] = q[1]; s_box[wave][pos][2] = q[2]; s_box[wave][pos][3] = q[3];
                s_area[wave][pos] = coco_gt_range_area(gt, gstride, g, gt_area, scale);
                s_crowd[wave][pos] = (gstride > 6 && q[6] != 0.0f) ? 1 : 0;
            }
            cnt += __popcll(b);
        }
        const bool fast = cnt <= kCocoMaskGts;
        coco_wave_sync();
        unsigned long long ign_mask = 0ull, crowd_mask = 0ull, matched = 0ull;
        if (fast) {
            for (int i = 0; i < cnt; ++i) {
                const double ar = s_area[wave][i];
                const bool crowd = s_crowd[wave][i] != 0;
                if (crowd) crowd_mask |= 1ull << i;
                if (crowd || ar < lo || ar > hi) ign_mask |= 1ull << i;
            }
        } else if (has) {                            // this lane's matched bytes of the image's class-c gts (only this lane reads them back)
            for (int g = g_begin; g < g_end; ++g)
                if ((int)gt[(long long)g * gstride + 4] == c) gt_matched[(long long)g * TA + lane] = 0;
        }
        const unsigned long long valid = cnt >= 64 ? ~0ull : (1ull << cnt) - 1ull;

        const long long len = j1 - j0, take = len < (long long)max_last ? len : (long long)max_last;
        for (long long r = 0; r < take; ++r) {       // the detections in rank order
            const long long row = perm_a[j0 + r];
            const float* p = pred + row * 7;
            const double d[4] = {(double)p[1], (double)p[2], (double)p[3], (double)p[4]};
            const double area_d = (d[2] - d[0]) * (d[3] - d[1]);
            double best = best0;
            long long m = -1;
            bool m_ign = false;
            if (fast) {
                if (lane < cnt) s_iou[wave][lane] = coco_iou(d, area_d, s_box[wave][lane], s_crowd[wave][lane] != 0);
                coco_wave_sync();
                if (has) {
                    // the gts that count first, then the ignored ones -- and those only while nothing that counts is matched (the break rule)
                    unsigned long long cand = valid & ~ign_mask & ~matched;
                    while (cand) {
                        const int i = __ffsll((long long)cand) - 1;
                        cand &= cand - 1ull;
                        const double v = s_iou[wave][i];
                        if (v < best) continue;
                        best = v; m = i;             // >= : the last of equal IoUs wins
                    }
                    if (m < 0) {
                        cand = valid & ign_mask & (~matched | crowd_mask);   // a crowd gt may be matched again
                        while (cand) {
                            const int i = __ffsll((long long)cand) - 1;
                            cand &= cand - 1ull;
                            const double v = s_iou[wave][i];
                            if (v < best) continue;
                            best = v; m = i; m_ign = true;
                        }
                    }
                    if (m >= 0) matched |= 1ull << m;
                }
                coco_wave_sync();
            } else if (has) {
                for (int part = 0; part < 2 && m < 0; ++part) {
                    for (int g = g_begin; g < g_end; ++g) {                  // g is the same in every lane: the loads are broadcasts
                        const float* q = gt + (long long)g * gstride;
                        if ((int)q[4] != c) continue;
                        const bool crowd = gstride > 6 && q[6] != 0.0f;
                        const double ar = coco_gt_range_area(gt, gstride, g, gt_area, scale);
                        const bool ign = crowd || ar < lo || ar > hi;
                        if ((int)ign != part) continue;
                        if (gt_matched[(long long)g * TA + lane] && !crowd) continue;
                        const double v = coco_iou(d, area_d, q, crowd);
                        if (v < best) continue;
                        best = v; m = g; m_ign = ign;
                    }
                }
                if (m >= 0) gt_matched[m * TA + lane] = 1;
            }
            if (lane == 0) rank_out[row] = (int)r;
            if (has) {
                const double ar = area_d * scale;
                const bool ign = m >= 0 ? m_ign : (ar < lo || ar > hi);
                flags_out[row * TA + lane] = (unsigned char)((m >= 0 ? 1 : 0) | (ign ? 2 : 0));
            }
        }
        for (long long j = j0 + take + lane; j < j1; j += kWave) {           // past the largest max_dets: ranked, part of nothing
            const long long row = perm_a[j];
            rank_out[row] = (int)(j - j0);
            for (int p = 0; p < TA; ++p) flags_out[row * TA + p] = 0;
        }
        coco_wave_sync();                            // the next group restages the LDS rows
    }
}

struct OpMaxD { __device__ __forceinline__ double operator()(double a, double b) const { return a > b ? a : b; } };
struct OpAddU64 { __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; } };

// COCOeval.accumulate: one workgroup per (class k, area a, max_dets m) walks the class segment of the (class, score desc, image, row) order
// twice -- forward for the totals of every threshold, backward for the reverse running maximum of the precision, where the detection
// whose true-positive count is c serves every recall threshold that needs c true positives (need[r], an integer worked out once).
__global__ void __launch_bounds__(kCocoThreads) coco_accumulate_kernel(
    const unsigned long long* __restrict__ key_b, const unsigned* __restrict__ perm_b, long long n, const int* __restrict__ rank, const unsigned char* __restrict__ flags,
    const int* __restrict__ npig, const double* __restrict__ rec_thrs, int T, int R, int K, int A, int M, int4 max_dets, double* __restrict__ precision,
    double* __restrict__ recall) {
    __shared__ int s_need[kCocoMaxR];
    __shared__ double s_pm[kCocoThreads];
    __shared__ unsigned long long s_total[kCocoMaxPairs], s_suffix[kCocoMaxPairs];   // (tp, fp) packed as two 32-bit halves, per threshold
    __shared__ double s_best[kCocoMaxPairs];
    __shared__ unsigned long long s_scan_i[17];
    __shared__ double s_scan_d[17];
    __shared__ long long s_range[2];
    __shared__ int s_kept;

    const int k = blockIdx.x, a = blockIdx.y, m = blockIdx.z, tid = threadIdx.x, lane = lane_id();
    const int cap = m == 0 ? max_dets.x : m == 1 ? max_dets.y : m == 2 ? max_dets.z : max_dets.w;
    const int TA = T * A;
    const int np = npig[k * A + a];
    const long long pstride = (long long)K * A * M, pbase = ((long long)k * A + a) * M + m;   // precision[t][r][k][a][m], recall[t][k][a][m]
    if (np == 0) {
        for (long long e = tid; e < (long long)T * R; e += kCocoThreads) precision[e * pstride + pbase] = -1.0;
        for (int t = tid; t < T; t += kCocoThreads) recall[t * pstride + pbase] = -1.0;
        return;
    }
    if (tid < 2) {
        const unsigned long long want = (unsigned long long)(unsigned)(k + tid) << 32;
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (key_b[mid] < want) lo = mid + 1; else hi = mid;
        }
        s_range[tid] = lo;
    }
    if (tid < kCocoMaxPairs) { s_total[tid] = 0ull; s_suffix[tid] = 0ull; s_best[tid] = -1.0; }
    if (tid == 0) s_kept = 0;
    const double npd = (double)np;
    for (int r = tid; r < R; r += kCocoThreads) {   // need[r]: the least integer c with c / npig >= rec_thrs[r] in fp64 (np + 1: never reached)
        const double thr = rec_thrs[r];
        long long c = 0;
        if (thr > 0.0) {
            const double est = ceil(thr * npd);
            c = est >= npd + 1.0 ? (long long)np + 1 : (long long)est;
            while (c > 0 && (double)(c - 1) / npd >= thr) --c;
            while (c <= np && (double)c / npd < thr) ++c;
        } else if (thr != thr) {
            c = (long long)np + 1;
        }
        s_need[r] = (int)c;
    }
    __syncthreads();
    const long long begin = s_range[0], len = s_range[1] - s_range[0];
    const long long chunks = (len + kCocoThreads - 1) / kCocoThreads;

    // pass 1: per threshold the number of true and false positives among the kept detections
    int kept_mine = 0;
    for (long long ch = 0; ch < chunks; ++ch) {
        const long long i = ch * kCocoThreads + tid;
        bool kept = false;
        const unsigned char* f = flags;
        if (i < len) {
            const long long row = perm_b[begin + i];
            kept = rank[row] < cap;
            f = flags + row * TA + a;
        }
        kept_mine += kept;
        for (int t = 0; t < T; ++t) {
            const unsigned char v = kept ? f[t * A] : (unsigned char)2;
            const unsigned long long btp = __ballot(v == 1), bfp = __ballot(v == 0);
            if (lane == 0 && (btp | bfp)) atomicAdd(&s_total[t], (unsigned long long)__popcll(btp) | ((unsigned long long)__popcll(bfp) << 32));
        }
    }
    if (kept_mine) atomicAdd(&s_kept, kept_mine);
    __syncthreads();
    const int nd = s_kept;
    for (long long e = tid; e < (long long)T * R; e += kCocoThreads) {   // the thresholds no detection reaches: 0
        const int t = (int)(e / R), r = (int)(e % R);
        if (nd == 0 || (long long)s_need[r] > (long long)(unsigned)s_total[t]) precision[e * pstride + pbase] = 0.0;
    }
    for (int t = tid; t < T; t += kCocoThreads) recall[t * pstride + pbase] = nd ? (double)(unsigned)s_total[t] / npd : 0.0;
    if (nd == 0) return;

    // pass 2, backward: thread x of chunk ch holds position ch * 256 + 255 - x, so scanning x upwards walks the positions downwards
    const double neg_inf = -__builtin_huge_val();
    for (long long ch = chunks - 1; ch >= 0; --ch) {
        const long long i = ch * kCocoThreads + (kCocoThreads - 1 - tid);
        bool kept = false;
        const unsigned char* f = flags;
        if (i < len) {
            const long long row = perm_b[begin + i];
            kept = rank[row] < cap;
            f = flags + row * TA + a;
        }
        for (int t = 0; t < T; ++t) {
            const unsigned char v = kept ? f[t * A] : (unsigned char)2;
            const unsigned long long mine = (unsigned long long)(v == 1) | ((unsigned long long)(v == 0) << 32);
            unsigned long long agg;
            const unsigned long long incl = block_inclusive_scan(mine, OpAddU64(), s_scan_i, &agg);   // this position and everything behind it in the chunk
            const unsigned long long total = s_total[t], behind = s_suffix[t];
            const double carry = s_best[t];
            // counts up to and including this position = total - (what lies strictly behind it)
            const unsigned long long after = behind + incl - mine;
            const unsigned tp = (unsigned)total - (unsigned)after, fp = (unsigned)(total >> 32) - (unsigned)(after >> 32);
            const double tpd = (double)tp, fpd = (double)fp;
            const double pr = kept ? tpd / (fpd + tpd + 2.220446049250313e-16) : neg_inf;
            const double run = block_inclusive_scan(pr, OpMaxD(), s_scan_d, (double*)nullptr);
            const double pm = run > carry ? run : carry;             // the reverse running maximum at this position
            const unsigned c_hi = (unsigned)total - (unsigned)behind, c_lo = c_hi - (unsigned)agg;   // the chunk holds the true positives c_lo + 1 .. c_hi
            if (v == 1) s_pm[tp - c_lo - 1] = pm;
            __syncthreads();
            if (c_hi != c_lo)
                for (int r = tid; r < R; r += kCocoThreads) {
                    const unsigned need = (unsigned)s_need[r];
                    if (need > c_lo && need <= c_hi) precision[((long long)t * R + r) * pstride + pbase] = s_pm[need - c_lo - 1];
                }
            __syncthreads();
            if (tid == kCocoThreads - 1) { s_suffix[t] = behind + agg; s_best[t] = pm; }
        }
        __syncthreads();
    }
    // rec_thrs[r] <= 0 needs no true positive: the first kept detection, whose running maximum is the maximum of all
    for (long long e = tid; e < (long long)T * R; e += kCocoThreads) {
        const int t = (int)(e / R), r = (int)(e % R);
        if (s_need[r] == 0) precision[e * pstride + pbase] = s_best[t];
    }
}

// COCOeval.summarize: stats[12] = AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl -- the mean of the entries > -1 of a slice
__global__ void __launch_bounds__(kCocoThreads) coco_summary_kernel(const double* __restrict__ precision, const double* __restrict__ recall,
                                                                  const double* __restrict__ iou_thrs, int T, int R, int K, int A, int M, double* stats) {
    __shared__ double s_red[kCocoThreads / kWave];
    __shared__ long long s_cnt[kCocoThreads / kWave];
    const int s = blockIdx.x, tid = threadIdx.x;
    const bool ap = s < 6;
    int a = 0, m = M - 1, t_only = -1;
    bool exists = true;
    if (s == 1 || s == 2) {
        const double want = s == 1 ? 0.5 : 0.75;
        for (int t = 0; t < T; ++t)
            if (fabs(iou_thrs[t] - want) < 1e-9) { t_only = t; break; }
        exists = t_only >= 0;
    }
    if (s >= 3 && s <= 5) a = s - 2;
    if (s >= 6 && s <= 8) m = s - 6;
    if (s >= 9) a = s - 8;
    exists = exists && a < A && m < M;
    double sum = 0.0;
    long long cnt = 0;
    if (exists) {
        const int t0 = t_only >= 0 ? t_only : 0, t1 = t_only >= 0 ? t_only + 1 : T;
        const long long inner = ap ? (long long)R * K : (long long)K;           // entries per threshold
        const long long stride = (long long)A * M, off = (long long)a * M + m;
        const double* src = ap ? precision : recall;
        for (long long e = (long long)t0 * inner + tid; e < (long long)t1 * inner; e += kCocoThreads) {
            const double v = src[e * stride + off];
            if (v > -1.0) { sum += v; ++cnt; }
        }
    }
    const double total = block_sum(sum, s_red);
    const long long count = block_sum(cnt, s_cnt);
    if (tid == 0) stats[s] = count ? total / (double)count : -1.0;
}

}  // namespace ssdk

extern "C" size_t ssdk_coco_eval_workspace_bytes(long long n_pred, long long total_gt, int num_classes, int num_iou_thrs, int num_area_rngs) {
    if (n_pred < 0 || n_pred >= (1LL << 31) || total_gt < 0 || total_gt >= (1LL << 31) || num_classes <= 0 || num_classes >= (1 << 20) || num_iou_thrs < 1 ||
        num_area_rngs < 1 || (long long)num_iou_thrs * num_area_rngs > kCocoMaxPairs)
        return 0;
    return carve_coco(nullptr, n_pred, total_gt, num_classes, num_iou_thrs * num_area_rngs, num_area_rngs).total;
}

extern "C" int ssdk_coco_eval(const float* predictions, long long n_pred, const float* gt_rows, int gt_stride, const int* gt_offsets, int num_images,
                              long long total_gt, int num_classes, const double* gt_area, const double* image_area_scale, const double* iou_thrs,
                              int num_iou_thrs, const double* rec_thrs, int num_rec_thrs, const double* area_rngs, int num_area_rngs, const int* max_dets,
                              int num_max_dets, double* precision, double* recall, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    return ssdk_coco_eval_ex(predictions, n_pred, gt_rows, gt_stride, gt_offsets, num_images, total_gt, num_classes, gt_area, image_area_scale, iou_thrs,
                             num_iou_thrs, rec_thrs, num_rec_thrs, area_rngs, num_area_rngs, max_dets, num_max_dets, precision, recall, stats, nullptr, nullptr,
                             nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int ssdk_coco_eval_ex(const float* predictions, long long n_pred, const float* gt_rows, int gt_stride, const int* gt_offsets, int num_images,
                                 long long total_gt, int num_classes, const double* gt_area, const double* image_area_scale, const double* iou_thrs,
                                 int num_iou_thrs, const double* rec_thrs, int num_rec_thrs, const double* area_rngs, int num_area_rngs, const int* max_dets,
                                 int num_max_dets, double* precision, double* recall, double* stats, int32_t* rank_out, uint8_t* flags_out,
                                 uint32_t* order_out, int32_t* npig_out, void* workspace, size_t workspace_bytes, void* stream) {
    const int T = num_iou_thrs, R = num_rec_thrs, A = num_area_rngs, M = num_max_dets, K = num_classes;
    SSDK_REQUIRE(n_pred >= 0 && n_pred < (1LL << 31) && total_gt >= 0 && total_gt < (1LL << 31) && num_images >= 0 && K > 0 && K < (1 << 20), SSDK_E_INVALID,
                 "ssdk_coco_eval: n_pred=%lld total_gt=%lld num_images=%d num_classes=%d", n_pred, total_gt, num_images, K);
    SSDK_REQUIRE(T >= 1 && A >= 1 && M >= 1 && R >= 1 && (long long)T * A <= kCocoMaxPairs && M <= kCocoMaxM && R <= kCocoMaxR, SSDK_E_INVALID,
                 "ssdk_coco_eval: %d iou thresholds x %d area ranges (product <= %d), %d max_dets (<= %d), %d recall thresholds (1..%d)", T, A, kCocoMaxPairs, M,
                 kCocoMaxM, R, kCocoMaxR);
    SSDK_REQUIRE(gt_stride >= 5 && gt_offsets && iou_thrs && rec_thrs && area_rngs && max_dets && precision && recall && stats && (n_pred == 0 || predictions) &&
                     (total_gt == 0 || gt_rows),
                 SSDK_E_INVALID, "ssdk_coco_eval: null pointer or gt_stride=%d < 5", gt_stride);
    int md[kCocoMaxM];
    for (int i = 0; i < kCocoMaxM; ++i) md[i] = max_dets[i < M ? i : M - 1];
    for (int i = 0; i < M; ++i)
        SSDK_REQUIRE(md[i] >= 1 && (i == 0 || md[i] > md[i - 1]), SSDK_E_INVALID, "ssdk_coco_eval: max_dets[%d]=%d (host array, positive and ascending)", i, md[i]);
    SSDK_REQUIRE((double)T * R * K * A * M < 2147483648.0, SSDK_E_INVALID, "ssdk_coco_eval: precision[%d, %d, %d, %d, %d] has 2^31 entries or more", T, R, K, A, M);
    const int TA = T * A;
    CocoWs w = carve_coco(workspace, n_pred, total_gt, K, TA, A);
    SSDK_REQUIRE(workspace && workspace_bytes >= w.total, SSDK_E_WORKSPACE, "ssdk_coco_eval: workspace %zu < %zu bytes", workspace_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    int* ngroups = w.npig + (size_t)K * A;
    SSDK_CHECK_HIP(zero_async(w.npig, sizeof(int) * ((size_t)K * A + 1), s));
    if (total_gt > 0) {
        hipLaunchKernelGGL(coco_npig_kernel, dim3((unsigned)cdiv((int)total_gt, 256)), dim3(256), 0, s, gt_rows, gt_stride, total_gt, gt_offsets, num_images, K, gt_area,
                           image_area_scale, area_rngs, A, w.npig);
        SSDK_CHECK_LAUNCH("coco_npig_kernel");
    }
    if (n_pred > 0) {
        const int n = (int)n_pred;
        const unsigned blocks = (unsigned)cdiv(n, 256);
        int class_bits = 1;
        while ((1 << class_bits) <= K) ++class_bits;
        // (image, row)
        hipLaunchKernelGGL(coco_image_key_kernel, dim3(blocks), dim3(256), 0, s, predictions, n_pred, (const unsigned*)nullptr, w.key_a, w.val_a);
        SSDK_CHECK_LAUNCH("coco_image_key_kernel");
        int rc = radix_sort_pairs(w.key_a, w.key_c, w.val_a, w.perm_a, n_pred, 32, w.table, w.digit_total, s);
        if (rc) return rc;
        // stable by (class, score desc) on top: (class, score desc, image, row) -- COCOeval.accumulate's concatenate-then-mergesort order
        hipLaunchKernelGGL(coco_class_key_kernel, dim3(blocks), dim3(256), 0, s, predictions, n_pred, w.perm_a, K, w.key_a, w.val_a);
        SSDK_CHECK_LAUNCH("coco_class_key_kernel");
        rc = radix_sort_pairs(w.key_a, w.key_b, w.val_a, w.perm_b, n_pred, 32 + class_bits, w.table, w.digit_total, s);
        if (rc) return rc;
        // stable by image on top: (image, class, score desc, row) -- the order within COCOeval.evaluateImg's groups
        hipLaunchKernelGGL(coco_image_key_kernel, dim3(blocks), dim3(256), 0, s, predictions, n_pred, w.perm_b, w.key_a, w.val_a);
        SSDK_CHECK_LAUNCH("coco_image_key_kernel");
        rc = radix_sort_pairs(w.key_a, w.key_c, w.val_a, w.perm_a, n_pred, 32, w.table, w.digit_total, s);
        if (rc) return rc;
        hipLaunchKernelGGL(coco_groups_kernel, dim3(blocks), dim3(256), 0, s, predictions, n_pred, w.perm_a, w.key_c, w.group_start, ngroups);
        SSDK_CHECK_LAUNCH("coco_groups_kernel");
        const unsigned waves = (unsigned)cdiv(n, kCocoWaves);
        hipLaunchKernelGGL(coco_match_kernel, dim3(waves < 2048u ? waves : 2048u), dim3(kCocoWaves * kWave), 0, s, predictions, n_pred, w.perm_a, w.key_c, w.group_start,
                           ngroups, gt_rows, gt_stride, gt_offsets, num_images, K, gt_area, image_area_scale, iou_thrs, T, area_rngs, A, md[M - 1], w.gt_matched, w.rank,
                           w.flags);
        SSDK_CHECK_LAUNCH("coco_match_kernel");
        if (rank_out) SSDK_CHECK_HIP(hipMemcpyAsync(rank_out, w.rank, sizeof(int) * (size_t)n_pred, hipMemcpyDeviceToDevice, s));
        if (flags_out) SSDK_CHECK_HIP(hipMemcpyAsync(flags_out, w.flags, (size_t)n_pred * TA, hipMemcpyDeviceToDevice, s));
        if (order_out) SSDK_CHECK_HIP(hipMemcpyAsync(order_out, w.perm_b, sizeof(unsigned) * (size_t)n_pred, hipMemcpyDeviceToDevice, s));
    }
    if (npig_out) SSDK_CHECK_HIP(hipMemcpyAsync(npig_out, w.npig, sizeof(int) * (size_t)K * A, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)K, (unsigned)A, (unsigned)M), dim3(kCocoThreads), 0, s, w.key_b, w.perm_b, n_pred, w.rank, w.flags, w.npig,
                       rec_thrs, T, R, K, A, M, make_int4(md[0], md[1], md[2], md[3]), precision, recall);
    SSDK_CHECK_LAUNCH("coco_accumulate_kernel");
    hipLaunchKernelGGL(coco_summary_kernel, dim3(12), dim3(kCocoThreads), 0, s, precision, recall, iou_thrs, T, R, K, A, M, stats);
    SSDK_CHECK_LAUNCH("coco_summary_kernel");
    return SSDK_OK;
}
