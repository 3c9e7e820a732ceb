// norm.hip -- BatchNorm2d (+ optional ReLU) on NHWC rows, forward and backward.
//
// Reference: bf/modules/conv.py:30-36 (Conv2dBn: conv -> BatchNorm2d -> ReLU, the SSD pyramid tail built by
// detection/detector_builder.py:57-109) and detection/modules/predictors.py:60-76 (RetinaNet tower: conv -> ReLU ->
// a BatchNorm2d per level).  torch.nn.BatchNorm2d semantics: training mode normalises with the biased batch variance
// and updates running_mean / running_var (unbiased) with `momentum`; eval mode uses the running statistics.
//
// All three kernels are HBM-bound streams over a [rows = B*H*W][C] matrix (channels contiguous, so a wave reads whole
// lines): bn_reduce_kernel accumulates two per-channel sums -- a workgroup takes 64 or more rows x a slab of 16 float4 columns, a wave
// instruction four consecutive rows of the slab, in registers, then one fp64 atomic per channel (bn_reduce_plan: the grid is row blocks x
// column slabs) -- bn_apply_kernel turns them into mean / rstd itself (and updates the running statistics), bn_apply_kernel /
// bn_bwd_apply_kernel are the elementwise passes with the ReLU fused; both carry the side job of zero-filling the layer's other `sums`
// buffer, and bn_bwd_apply_kernel a second one, spread over its grid: zero-filling the dx of the producing strided convolution (zero_also).
#include "common.h"

namespace ssdk {

constexpr int kBnRows = 64;
// Rows per bn_reduce workgroup.  The figures of this paragraph and of the first one inside the function are those of the WHOLE-ROW form
// (every workgroup owns every channel: SSDK_BN_SLAB=0 today); the column slabs' own sweep is the last paragraph inside the function.
// Measured over the SSD-300 tail (rocprofv3, all eight layers; SSDK_BN_ROWS overrides): 64 rows is the best
// single value (8.3 us per launch on average; 128: 10.0, 256: 14.3 -- fewer, longer chains of dependent loads; 32: 10.4, 16: 16.3 --
// the big maps then queue 4x the same-address fp64 atomics per channel).  Picking 16 / 32 rows for the small maps only (2.7 - 2.9 us
// against 4.1) did not move the step time beyond run-to-run noise and is not done.
static inline int bn_rows_per_block(long long rows, bool slabs) {
    if (const char* e = getenv("SSDK_BN_ROWS")) return atoi(e);
    // Large maps (RetinaNet's 63 x 63 level at batch 32: 127 k rows): every workgroup ends with one fp64 atomic per channel and sum, all on
    // the same 2C addresses, and with 64 rows 1 984 workgroups queue there.  bn_reduce<0> per launch, averaged over the tower's five levels
    // (rocprofv3, tools/bnrows_retina.sh): 64 rows everywhere 53.4 us; 256 rows everywhere 30.2 (the small levels then take 17 instead of
    // 6 us); 64 rows until the launch has N workgroups, then more rows per workgroup: N = 1536: 42.3, 1024: 36.6, 768: 32.3, 512: 29.1,
    // 384: 24.8, 256: 23.0, 192: 23.1 (backward statistics alike: 60.7 -> 28.9).  retina_rn50_500_coco step 52.97 -> 50.17 ms.
    // (round 4, tools/ab_step.sh SSDK_BN_WGS 256 128 64 on one box: M2Det 31.45 / 31.28 / 31.73 ms per step, RetinaNet 46.57 / 46.53 / 46.82, SSD-300
    // unchanged: 128 -- the mid-size maps of the M2Det neck, 16 k rows, spent ~20 of their 36 us in the 256-way atomics)
    // With column slabs (bn_reduce_plan) the workgroups of a launch are row blocks x slabs and the chain of a workgroup is 64 / slab times
    // shorter, so the row blocks -- the adders per address -- can be fewer: 64 (tools/bn_slab_sweep.py, slab 16, 128 -> 64, us per forward /
    // backward launch summed over the maps: SSD-300 tail 44.9 / 67.3 -> 41.3 / 63.5, M2Det neck 141 / 300 -> 122 / 287, RetinaNet tower 68 / 135
    // -> 62 / 118; 256: 49.0 / 71.5, 183 / 339, 94 / 140).  Whole rows (SSDK_BN_SLAB=0) keep 128.
    const long long target = getenv("SSDK_BN_WGS") ? atoll(getenv("SSDK_BN_WGS")) : (slabs ? 64 : 128);
    long long r = (rows + target - 1) / target;
    r = (r + 15) / 16 * 16;
    // ... and at least 128 rows per workgroup with slabs (two trips of a workgroup over its rows; same tool, BN_SWEEP_RULES=1, floors 64 / 128 /
    // 256 at 64 row blocks: SSD-300 tail 45.6 / 69.6, 42.7 / 68.9, 46.0 / 68.6; M2Det neck 122.8 / 290.2, 118.3 / 286.8, 119.4 / 286.9; RetinaNet
    // tower 63.5 / 123.1, 62.7 / 123.3, 61.1 / 122.0; 32, 48 and 96 row blocks are no better on any of the three).
    const long long least = slabs ? 2 * kBnRows : kBnRows;
    return (int)(r < least ? least : (r > 4096 ? 4096 : r));
}

// The grid of a bn_reduce launch: (row blocks) x (column slabs), flattened with the slabs innermost so that neighbouring workgroups read
// neighbouring bytes.  A workgroup owns `slab` float4 columns (a power of two, at most 64) of its rows, and a wave instruction takes
// 64 / slab consecutive rows of them.  With whole rows per workgroup (the form before: slabs == 1) a map of 256 or 512 channels gave a wave
// instruction one row, a 64-row workgroup a chain of four dependent memory trips per 64 columns and the launch 41 - 108 workgroups on 256
// CUs; with 16-column slabs the same launch has 4 - 8x the workgroups, each with a quarter (an eighth) of the bytes and of the chain.  The
// number of workgroups that add to one address is the number of ROW blocks: the rows-per-workgroup rule above balances exactly that
// contention against the chain length, and with the shorter chains it aims at 64 row blocks instead of 128.
//   SSDK_BN_SLAB (read per call): 0 = whole rows per workgroup (the form before: the A side of a measurement on one binary), else the
//   slab width in float4 columns, rounded up to a power of two and capped at 64.  Default 16: 256-byte row segments.
//   C / 4 that the slab width does not divide (33 = 132 / 4, 224 = 896 / 4): the LAST SLAB IS NARROWER -- its spare lanes idle, as the
//   spare lanes of the last 64 columns always did; falling back to whole rows would have kept the M2Det reducers (C = 896) out.
//   C / 4 below the slab width: one slab of the next power of two (C / 4 = 12: 16 columns, 4 idle, four rows per instruction).
struct BnReducePlan {
    int rows_per_block, slab, slabs;   // slab: float4 columns per workgroup and trip; slabs: workgroups side by side over the columns
    int fold64;                        // folds across lanes and waves in fp64 (every layout but the packed / whole-row forms of before)
    long long row_blocks;
};
static inline int bn_pow2_at_least(int v) { int p = 1; while (p < v && p < 64) p <<= 1; return p; }
static inline BnReducePlan bn_reduce_plan(long long rows, int C) {
    BnReducePlan p;
    const int C4 = C >> 2;
    const char* e = getenv("SSDK_BN_SLAB");
    const int want = e ? atoi(e) : 16;
    p.rows_per_block = bn_rows_per_block(rows, want > 0);
    if (p.rows_per_block < 1) p.rows_per_block = 1;
    p.row_blocks = (rows + p.rows_per_block - 1) / p.rows_per_block;
    if (want <= 0) {   // whole rows: one workgroup walks all columns, 64 at a time (a row of at most 32 that divides 64: packed)
        p.slab = (C4 <= 32 && 64 % C4 == 0) ? C4 : 64;
        p.slabs = 1;
        p.fold64 = 0;
    } else {
        p.slab = bn_pow2_at_least(want < C4 ? want : C4);
        p.slabs = (C4 + p.slab - 1) / p.slab;
        p.fold64 = !(p.slabs == 1 && p.slab == C4);   // (one slab as wide as the row IS the packed form of before: its arithmetic, its bits)
    }
    return p;
}

// MODE 0: s0 = sum x, s1 = sum x^2.   MODE 1 (backward): s0 = sum dy', s1 = sum dy' * xhat, dy' = relu ? dy * (y > 0) : dy
// Workgroup = rows_per_block rows x one column slab (see bn_reduce_plan); lane l owns float4 column l % slab of the slab and row l / slab of
// the 64 / slab consecutive rows a wave instruction takes; wave w takes row groups w, w+4, ...  The lanes that share a column are folded
// with cross-lane adds, the four waves through LDS, and the workgroup ends with ONE atomic per channel and sum.
// MODE 0 accumulates in fp64 from the first add on: the variance is E[x^2] - mean^2, and with fp32 partial sums a channel whose mean is
// 100 standard deviations lost four digits of it ("BatchNorm statistics: conditioning").  The square of an fp32 value is exact
// in fp64; the kernel streams from HBM and the fp64 adds hide behind the loads.  MODE 1 sums centred, scaled values: a lane's own chain of
// adds stays in fp32; the folds across lanes and waves behind it are fp64 in the layouts the slabs introduce (fold64, see the fold below).
template <typename T> struct bn_acc4 { T x, y, z, w; };
template <int MODE>
__global__ void __launch_bounds__(256) bn_reduce_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                        long long rows, int rows_per_block, int C, int slab, int slabs, int fold64,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd, int relu,
                                                        double* __restrict__ sums) {
    using acc_t = typename std::conditional<MODE == 0, double, float>::type;
    using acc4 = bn_acc4<acc_t>;
    __shared__ bn_acc4<double> s_part[2 * 4 * 64];   // (16 KB: [sum][wave][lane], fp64 or the accumulator's type)
    const int my_slab = (int)(blockIdx.x % (unsigned)slabs);
    const long long r0 = (long long)(blockIdx.x / (unsigned)slabs) * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C4 = C >> 2;
    const int rpw = 64 / slab;            // rows per wave instruction (slab is a power of two)
    const int col = lane & (slab - 1);    // this lane's column inside the slab
    const int sub = lane / slab;          // ... and its row inside the rpw rows
    if (blockIdx.x == 0 && threadIdx.x == 0) sums[2 * C] = (double)rows;   // (slot 2C: the count behind the sums)
    // (slabs == 1: this workgroup walks all the columns, `slab` at a time -- whole rows)
    for (int cbase = my_slab * slab; cbase < C4; cbase += slabs * slab) {
        const int c4 = cbase + col;
        acc4 a0 = {0, 0, 0, 0}, a1 = a0;
        if (c4 < C4) {
            float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), rs4 = m4;
            if (MODE == 1) { m4 = reinterpret_cast<const float4*>(mean)[c4]; rs4 = reinterpret_cast<const float4*>(rstd)[c4]; }
            // four row groups per trip, all their loads issued before the first is consumed (a row per trip made every wave wait one
            // memory round trip per row: 10-24 us on the small pyramid maps); rows past the end re-read the last row, weight 0
            for (long long v = wave; r0 + v * rpw < r1; v += 16) {
                float4 xv[4], gv[4], yv[4];
                float wgt[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long ru = r0 + (v + 4 * u) * rpw + sub;
                    wgt[u] = ru < r1 ? 1.0f : 0.0f;
                    const long long rr = ru < r1 ? ru : r1 - 1;
                    xv[u] = reinterpret_cast<const float4*>(x + rr * C)[c4];
                    if (MODE == 1) {
                        gv[u] = reinterpret_cast<const float4*>(dy + rr * C)[c4];
                        if (relu) yv[u] = reinterpret_cast<const float4*>(y + rr * C)[c4];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (wgt[u] == 0.0f) continue;
                    const float4 xu = xv[u];
                    if (MODE == 0) {
                        const acc_t x0 = xu.x, x1 = xu.y, x2 = xu.z, x3 = xu.w;
                        a0.x += x0; a0.y += x1; a0.z += x2; a0.w += x3;
                        a1.x += x0 * x0; a1.y += x1 * x1; a1.z += x2 * x2; a1.w += x3 * x3;
                    } else {
                        float4 g = gv[u];
                        if (relu) {
                            if (!(yv[u].x > 0.f)) g.x = 0.f;
                            if (!(yv[u].y > 0.f)) g.y = 0.f;
                            if (!(yv[u].z > 0.f)) g.z = 0.f;
                            if (!(yv[u].w > 0.f)) g.w = 0.f;
                        }
                        a0.x += g.x; a0.y += g.y; a0.z += g.z; a0.w += g.w;
                        a1.x += g.x * ((xu.x - m4.x) * rs4.x); a1.y += g.y * ((xu.y - m4.y) * rs4.y);
                        a1.z += g.z * ((xu.z - m4.z) * rs4.z); a1.w += g.w * ((xu.w - m4.w) * rs4.w);
                    }
                }
            }
        }
        // (uniform) lanes col, col + slab, col + 2 slab, ... hold the same column: fold them into lane col, then the four waves through LDS.
        // fold64 == 0 (the workgroup is the packed or the whole-row form of before: one slab as wide as the row, or SSDK_BN_SLAB=0): the folds
        // are in the accumulator's type, fp32 in MODE 1, operation for operation what that form always did -- same bits.  fold64 != 0 (every
        // layout the slabs introduce): the folds are fp64 in both modes (the conversion is exact), so MODE 1's fp32 rounding is that of a
        // lane's own rows / (16 * rpw) adds and nothing else.  With fp32 folds the slab form, which folds 64 / slab lanes where the whole-row
        // form folded none, missed the dx bar of tests/test_batchnorm_kernels_gpu.py on a channel that is zero in most rows (1.6 x the bar;
        // tools/bn_fold_emulation.py reproduces both orders on the test's data).
        auto fold = [&](auto tag) {
            using F = decltype(tag);
            using fold4 = bn_acc4<F>;
            fold4* const part = reinterpret_cast<fold4*>(s_part);   // [2][4][64]
            fold4 f0 = {(F)a0.x, (F)a0.y, (F)a0.z, (F)a0.w}, f1 = {(F)a1.x, (F)a1.y, (F)a1.z, (F)a1.w};
            for (int d = slab; d < 64; d <<= 1) {
                f0.x += __shfl_xor(f0.x, d, 64); f0.y += __shfl_xor(f0.y, d, 64); f0.z += __shfl_xor(f0.z, d, 64); f0.w += __shfl_xor(f0.w, d, 64);
                f1.x += __shfl_xor(f1.x, d, 64); f1.y += __shfl_xor(f1.y, d, 64); f1.z += __shfl_xor(f1.z, d, 64); f1.w += __shfl_xor(f1.w, d, 64);
            }
            __syncthreads();
            part[(0 * 4 + wave) * 64 + lane] = f0;
            part[(1 * 4 + wave) * 64 + lane] = f1;
            __syncthreads();
            if (wave < 2 && lane < slab && c4 < C4) {  // wave 0 folds the s0 partials, wave 1 the s1 partials
                fold4 t = part[(wave * 4 + 0) * 64 + lane];
                for (int w = 1; w < 4; ++w) { const fold4 u = part[(wave * 4 + w) * 64 + lane]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
                double* dst = sums + (size_t)wave * C + (size_t)c4 * 4;
                atomicAdd(dst + 0, (double)t.x); atomicAdd(dst + 1, (double)t.y); atomicAdd(dst + 2, (double)t.z); atomicAdd(dst + 3, (double)t.w);
            }
        };
        if (fold64) fold(double{}); else fold(acc_t{});
    }
}

// sums != NULL (training): mean / rstd come straight from the fp64 sums of bn_reduce_kernel<0> (no separate finalize
// launch); workgroup 0 also publishes save_mean / save_rstd for the backward and updates the running statistics.
// (inv_n = 1 / rows and unbias = rows / (rows - 1) once per thread, multiplications and one reciprocal square root per channel: the
// form with three fp64 divisions and a square root per channel was ~600 instructions in front of a thread's first load -- every thread of
// every apply launch derives its four channels' constants this way)
__device__ __forceinline__ void stats_from_sums(const double* sums, double inv_n, double unbias, int C, int c, float eps, float& m, float& rs, float& var_out) {
    const double mu = sums[c] * inv_n;
    double var = sums[C + c] * inv_n - mu * mu;
    if (var < 0.0) var = 0.0;
    m = (float)mu;
    rs = (float)rsqrt(var + (double)eps);
    var_out = (float)(var * unbias);
}

// evaluation mode: 1 / sqrt(running_var + eps), rounded once (the fp32 form -- add, square root, division: three roundings -- was up to
// 2 ulp off, which a beta that cancels most of gamma * xhat turns into several ulp of y)
__device__ __forceinline__ float eval_rstd(float running_var, float eps) { return (float)rsqrt((double)running_var + (double)eps); }

// The evaluation-mode constants of channel quad c, and the affine form of every forward apply: ((v - mean) * rstd) * gamma + beta, four
// roundings.  Shared by bn_apply_kernel and the depthwise stencil's norm epilogue (dw_norm_fwd_kernel), which must give the same bits
// as the stencil followed by the norm: each operation is an explicitly rounded one, so neither inlined copy can be contracted into a
// multiply-add whatever flags the file is built with (bilinear_tap's argument).
__device__ __forceinline__ void bn_eval_consts(const float* running_mean, const float* running_var, const float4* gamma, const float4* beta, float eps,
                                               int c, float4& m, float4& rs, float4& ga, float4& be) {
    m = reinterpret_cast<const float4*>(running_mean)[c];
    const float4 rv = reinterpret_cast<const float4*>(running_var)[c];
    rs = make_float4(eval_rstd(rv.x, eps), eval_rstd(rv.y, eps), eval_rstd(rv.z, eps), eval_rstd(rv.w, eps));
    ga = gamma ? gamma[c] : make_float4(1.f, 1.f, 1.f, 1.f);
    be = beta ? beta[c] : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float bn_affine(float v, float m, float rs, float ga, float be) {
    return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(v, m), rs), ga), be);
}
__device__ __forceinline__ float4 bn_affine4(const float4 v, const float4 m, const float4 rs, const float4 ga, const float4 be, int relu) {
    float4 o = make_float4(bn_affine(v.x, m.x, rs.x, ga.x, be.x), bn_affine(v.y, m.y, rs.y, ga.y, be.y), bn_affine(v.z, m.z, rs.z, ga.z, be.z),
                           bn_affine(v.w, m.w, rs.w, ga.w, be.w));
    if (relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    return o;
}

__global__ void __launch_bounds__(256) bn_apply_kernel(const float4* __restrict__ x, long long n4, int C4, const float4* __restrict__ mean,
                                                       const float4* __restrict__ rstd, const float4* __restrict__ gamma,
                                                       const float4* __restrict__ beta, int relu, float4* __restrict__ y,
                                                       const double* __restrict__ sums, long long rows, float eps, float momentum,
                                                       float* __restrict__ running_mean, float* __restrict__ running_var,
                                                       float* __restrict__ save_mean, float* __restrict__ save_rstd,
                                                       long long* __restrict__ num_batches_tracked, int count_on_device,
                                                       double* __restrict__ zero_after) {
    const int C = C4 * 4;
    if (zero_after && blockIdx.x == gridDim.x - 1)   // side job: zero-fill another sums buffer (nobody reads or writes it during this launch)
        for (int c = threadIdx.x; c < 2 * C + 2; c += blockDim.x) zero_after[c] = 0.0;
    if (sums && count_on_device) rows = (long long)sums[2 * C];   // synchronised statistics: the row count of all ranks travels with the sums
    if (num_batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) *num_batches_tracked += 1;
    const double inv_n = sums ? 1.0 / (double)rows : 0.0, unbias = rows > 1 ? (double)rows / ((double)rows - 1.0) : 1.0;
    if (sums && blockIdx.x == 0) {
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            float m, rs, uv;
            stats_from_sums(sums, inv_n, unbias, C, c, eps, m, rs, uv);
            save_mean[c] = m;
            save_rstd[c] = rs;
            if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * m;
            if (running_var) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * uv;
        }
    }
    if (!sums && !mean && blockIdx.x == 0)   // evaluation mode: what the backward of a frozen norm needs
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            save_mean[c] = running_mean[c];
            save_rstd[c] = eval_rstd(running_var[c], eps);
        }
    // A thread's four channels do not change over its grid-stride trips when the stride is a multiple of the row length (always for
    // power-of-two C): mean / rstd -- four fp64 divisions and square roots from the sums -- gamma and beta are then worked out ONCE per
    // thread, not once per float4.
    const long long stride = (long long)gridDim.x * blockDim.x;
    const bool fixed_c = stride % C4 == 0;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f), rs = m, ga = m, be = m;
    auto load_consts = [&](int c) {
        if (sums) {
            float uv;
            stats_from_sums(sums, inv_n, unbias, C, 4 * c + 0, eps, m.x, rs.x, uv);
            stats_from_sums(sums, inv_n, unbias, C, 4 * c + 1, eps, m.y, rs.y, uv);
            stats_from_sums(sums, inv_n, unbias, C, 4 * c + 2, eps, m.z, rs.z, uv);
            stats_from_sums(sums, inv_n, unbias, C, 4 * c + 3, eps, m.w, rs.w, uv);
        } else if (mean) {
            m = mean[c];
            rs = rstd[c];
        } else {   // evaluation mode: the running statistics (torch: 1 / sqrt(running_var + eps))
            bn_eval_consts(running_mean, running_var, gamma, beta, eps, c, m, rs, ga, be);
            return;
        }
        ga = gamma ? gamma[c] : make_float4(1.f, 1.f, 1.f, 1.f);
        be = beta ? beta[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    const long long i0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (fixed_c && i0 < n4) load_consts((int)(i0 % C4));
    for (long long i = i0; i < n4; i += stride) {
        if (!fixed_c) load_consts((int)(i % C4));
        y[i] = bn_affine4(x[i], m, rs, ga, be, relu);
    }
}

// dx = gamma * rstd * (dy' - [training] (sum dy')/n - xhat * (sum dy' xhat)/n)
// sums: the sums the statistics are taken over (all ranks' when synchronised) with their row count in sums[2C] when count_on_device;
// sums_local: this rank's own sums -- the affine parameters' gradients (summed over ranks later by the gradient exchange, like any other).
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                           long long rows, int C, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const double* __restrict__ sums,
                                                           const double* __restrict__ sums_local, int count_on_device, int relu, int training,
                                                           float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           double* __restrict__ zero_after, float* __restrict__ zero_also, long long zero_also_n) {
    // relu bit 0: the norm's own fused ReLU (dy counts where y > 0); bit 1: the norm's INPUT is the output of a ReLU whose gradient is
    // taken here as well (dx = 0 where x <= 0: conv -> ReLU -> BatchNorm of the RetinaNet tower, the producing convolution then skips its
    // own ReLU-gradient pass)
    const bool own_relu = (relu & 1) != 0, mask_input = (relu & 2) != 0;
    const long long total4 = rows * C / 4;   // (C % 4 == 0, 16-byte aligned buffers: checked by the host)
    const int C4 = C >> 2;
    if (zero_after && blockIdx.x == gridDim.x - 1)
        for (int c = threadIdx.x; c < 2 * C + 2; c += blockDim.x) zero_after[c] = 0.0;
    // second side job: zero-fill zero_also[0 .. zero_also_n) -- the dx of the producing convolution when its data gradient is the atomic
    // scatter form, a buffer nobody reads or writes during this launch.  Spread over the whole grid (megabytes from one workgroup would
    // outlast the launch): float4 stores over the 16-byte aligned middle, the at most 3 + 3 floats around it by the last workgroup.
    if (zero_also) {
        long long head = (long long)(((16 - ((uintptr_t)zero_also & 15)) & 15) >> 2);
        if (head > zero_also_n) head = zero_also_n;
        const long long mid4 = (zero_also_n - head) >> 2, tail0 = head + 4 * mid4;
        float4* const mid = reinterpret_cast<float4*>(zero_also + head);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < mid4; i += (long long)gridDim.x * blockDim.x) mid[i] = z;
        if (blockIdx.x == gridDim.x - 1) {
            if ((long long)threadIdx.x < head) zero_also[threadIdx.x] = 0.0f;
            if (tail0 + (long long)threadIdx.x < zero_also_n) zero_also[tail0 + threadIdx.x] = 0.0f;   // (at most 3 floats)
        }
    }
    const double inv_n = 1.0 / (count_on_device ? sums[2 * C] : (double)rows);
    // A thread's four channels stay the same over its grid-stride trips whenever the stride is a multiple of the row length (C / 4 divides
    // 256 * gridDim for every power-of-two C): their five per-channel constants are then loaded and converted ONCE.  (Per element they
    // were five scattered loads and two fp64 multiplies: the float4 form of this kernel was slower than the scalar one until they moved.)
    const long long stride = (long long)gridDim.x * blockDim.x;
    const bool fixed_c = stride % C4 == 0;
    float k_mean[4], k_rs[4], k_ga[4], k_m1[4], k_m2[4];
    auto load_consts = [&](int c) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            k_mean[k] = mean[c + k];
            k_rs[k] = rstd[c + k];
            k_ga[k] = gamma ? gamma[c + k] : 1.0f;
            k_m1[k] = training ? (float)(sums[c + k] * inv_n) : 0.0f;
            k_m2[k] = training ? (float)(sums[C + c + k] * inv_n) : 0.0f;
        }
    };
    const long long i0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (fixed_c && i0 < total4) load_consts((int)(i0 % C4) * 4);
    for (long long i = i0; i < total4; i += stride) {
        if (!fixed_c) load_consts((int)(i % C4) * 4);
        const float4 g4 = reinterpret_cast<const float4*>(dy)[i];
        const float4 x4 = reinterpret_cast<const float4*>(x)[i];
        float4 y4 = make_float4(1.f, 1.f, 1.f, 1.f);
        if (own_relu) y4 = reinterpret_cast<const float4*>(y)[i];
        const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, xx[4] = {x4.x, x4.y, x4.z, x4.w}, yy[4] = {y4.x, y4.y, y4.z, y4.w};
        float out[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float g = gg[k];
            if (own_relu && !(yy[k] > 0.0f)) g = 0.0f;
            const float xhat = (xx[k] - k_mean[k]) * k_rs[k];
            float v = g;
            if (training) v -= k_m1[k] + xhat * k_m2[k];
            out[k] = (mask_input && !(xx[k] > 0.0f)) ? 0.0f : k_ga[k] * k_rs[k] * v;
        }
        reinterpret_cast<float4*>(dx)[i] = make_float4(out[0], out[1], out[2], out[3]);
    }
    if (blockIdx.x == 0)
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            if (dbeta) dbeta[c] = (float)sums_local[c];
            if (dgamma) dgamma[c] = (float)sums_local[C + c];
        }
}

static inline int stream_blocks(long long items, int per_block) {
    long long b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
// Grid of the BatchNorm apply kernels (256 threads, one float4 per thread and trip): a thread keeps its four channels over all its
// grid-stride trips -- and works out their constants once -- when the stride, 256 * blocks, is a multiple of the row length C4.  For a
// power-of-two C every grid does; for the others (the seven stacked 128-channel reducers of the M2Det neck: C4 = 224) the block count is
// rounded down to a multiple of C4 / gcd(C4, 256): at 4 096 blocks such a launch re-derived mean / rstd from the fp64 sums for every
// float4 (16 x 896 x 64 x 64: forward 282 us against 188 at the rate of the 512-channel map, backward 484 against 330).
static inline int apply_blocks(long long n4, int C4) {
    const int b = stream_blocks(n4, 256);
    int g = C4, r = 256;
    while (r) { const int t = g % r; g = r; r = t; }   // gcd(C4, 256)
    const int m = C4 / g;
    return b >= m ? b / m * m : b;
}

}  // namespace ssdk

using namespace ssdk;

// a `sums` buffer: 2C sums, the row count at [2C], one double of padding (an even number of doubles: the zero-fill of an odd number
// is two fill kernels in the runtime, one for the 16-byte aligned part and one for the tail)
extern "C" size_t ssdk_batchnorm_workspace_bytes(int channels) { return align_up(((size_t)2 * channels + 2) * sizeof(double), 256); }

// TEST HOOK, host only: the grid the statistics launches (bn_reduce_kernel<0> and <1> alike) take for this map under the environment of the call
extern "C" int ssdk_debug_batchnorm_plan(long long rows, int channels, long long* out) {
    SSDK_REQUIRE(out && rows > 0 && channels > 0 && channels % 4 == 0, SSDK_E_INVALID, "ssdk_debug_batchnorm_plan: bad arguments (channels %% 4 == 0)");
    const BnReducePlan p = bn_reduce_plan(rows, channels);
    out[0] = p.rows_per_block; out[1] = p.row_blocks; out[2] = p.slab; out[3] = p.slabs;
    return SSDK_OK;
}

// The composed entry points launch twice: everything either half would refuse is refused here, before the first launch.
static int bn_fwd_check(const char* fn, const float* x, const float* y, const float* save_mean, const float* save_rstd, long long rows, int channels) {
    SSDK_REQUIRE(x && y && save_mean && save_rstd && rows > 0 && channels > 0, SSDK_E_INVALID, "%s: bad arguments", fn);
    SSDK_REQUIRE(channels % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0, SSDK_E_UNSUPPORTED, "%s: channels %% 4 != 0 or buffers not 16-byte aligned", fn);
    return SSDK_OK;
}
static int bn_bwd_check(const char* fn, const float* x, const float* y, const float* dy, const float* dx, const float* save_mean, const float* save_rstd,
                        long long rows, int channels, int relu) {
    SSDK_REQUIRE(x && dy && dx && save_mean && save_rstd && rows > 0 && channels > 0 && (!(relu & 1) || y), SSDK_E_INVALID, "%s: bad arguments", fn);
    SSDK_REQUIRE(channels % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)y) & 15) == 0, SSDK_E_UNSUPPORTED,
                 "%s: channels %% 4 != 0 or buffers not 16-byte aligned", fn);
    return SSDK_OK;
}

static int bn_stats(const float* x, long long rows, int channels, double* sums, bool zero_first, void* stream) {
    SSDK_REQUIRE(x && sums && rows > 0 && channels > 0, SSDK_E_INVALID, "ssdk_batchnorm_stats: bad arguments");
    SSDK_REQUIRE(channels % 4 == 0 && ((uintptr_t)x & 15) == 0, SSDK_E_UNSUPPORTED, "ssdk_batchnorm_stats: channels %% 4 != 0 or x not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (zero_first) SSDK_CHECK_HIP(zero_async(sums, sizeof(double) * (2 * (size_t)channels + 2), s));
    const BnReducePlan p = bn_reduce_plan(rows, channels);
    SSDK_REQUIRE(p.row_blocks * p.slabs < (1ll << 31), SSDK_E_UNSUPPORTED, "ssdk_batchnorm_stats: %lld row blocks x %d slabs exceed the grid", p.row_blocks, p.slabs);
    hipLaunchKernelGGL(bn_reduce_kernel<0>, dim3((unsigned)(p.row_blocks * p.slabs)), dim3(256), 0, s, x, (const float*)nullptr,
                       (const float*)nullptr, rows, p.rows_per_block, channels, p.slab, p.slabs, p.fold64, (const float*)nullptr, (const float*)nullptr, 0,
                       sums);
    SSDK_CHECK_LAUNCH("bn_reduce_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_batchnorm_stats(const float* x, long long rows, int channels, double* sums, void* stream) {
    return bn_stats(x, rows, channels, sums, true, stream);
}

// sums += this call's partial sums (the caller holds a buffer of zeros, or is accumulating over several calls); sums[2C] = rows
extern "C" int ssdk_batchnorm_stats_accumulate(const float* x, long long rows, int channels, double* sums, void* stream) {
    return bn_stats(x, rows, channels, sums, false, stream);
}

static int bn_apply(const float* x, long long rows, int channels, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, int64_t* num_batches_tracked, float momentum, float eps, int relu, float* y, float* save_mean,
                    float* save_rstd, const double* sums, int count_in_sums, double* zero_after, void* stream) {
    SSDK_REQUIRE(x && y && save_mean && save_rstd && sums && rows > 0 && channels > 0, SSDK_E_INVALID, "ssdk_batchnorm_apply: bad arguments");
    SSDK_REQUIRE(channels % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, SSDK_E_UNSUPPORTED,
                 "ssdk_batchnorm_apply: channels %% 4 != 0 or buffers not 16-byte aligned");
    const long long n4 = rows * channels / 4;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(apply_blocks(n4, channels / 4)), dim3(256), 0, (hipStream_t)stream, (const float4*)x, n4, channels / 4,
                       (const float4*)save_mean, (const float4*)save_rstd, (const float4*)gamma, (const float4*)beta, relu, (float4*)y, sums, rows,
                       eps, momentum, running_mean, running_var, save_mean, save_rstd, (long long*)num_batches_tracked, count_in_sums, zero_after);
    SSDK_CHECK_LAUNCH("bn_apply_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_batchnorm_apply(const float* x, long long rows, int channels, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                                    int relu, float* y, float* save_mean, float* save_rstd, const double* sums, int count_in_sums,
                                    void* stream) {
    return bn_apply(x, rows, channels, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, relu, y, save_mean, save_rstd,
                    sums, count_in_sums, nullptr, stream);
}

// The layer keeps two sums buffers of its own: `sums` holds zeros on entry (the layer's previous backward call zeroed it), `zero_after`
// -- the buffer the backward will accumulate into -- is zero-filled by the apply launch.  No fill launch in front of the statistics.
extern "C" int ssdk_batchnorm_fwd_chained(const float* x, long long rows, int channels, const float* gamma, const float* beta,
                                          float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                                          int relu, float* y, float* save_mean, float* save_rstd, double* sums, double* zero_after,
                                          void* stream) {
    SSDK_REQUIRE(sums && sums != zero_after, SSDK_E_INVALID, "ssdk_batchnorm_fwd_chained: sums missing or equal to zero_after");
    if (const int bad = bn_fwd_check("ssdk_batchnorm_fwd_chained", x, y, save_mean, save_rstd, rows, channels)) return bad;
    const int rc = bn_stats(x, rows, channels, sums, false, stream);
    if (rc) return rc;
    return bn_apply(x, rows, channels, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, relu, y, save_mean, save_rstd,
                    sums, 0, zero_after, stream);
}

// ... and when the statistics are already in `sums` (accumulated by the producing convolution's epilogue, ssdk_conv_desc::stats): the apply
// half alone, with the same side job of zero-filling the layer's other buffer.
extern "C" int ssdk_batchnorm_apply_chained(const float* x, long long rows, int channels, const float* gamma, const float* beta,
                                            float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                                            int relu, float* y, float* save_mean, float* save_rstd, const double* sums, double* zero_after,
                                            void* stream) {
    SSDK_REQUIRE(sums && sums != zero_after, SSDK_E_INVALID, "ssdk_batchnorm_apply_chained: sums missing or equal to zero_after");
    return bn_apply(x, rows, channels, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, relu, y, save_mean, save_rstd,
                    sums, 0, zero_after, stream);
}

extern "C" int ssdk_batchnorm_fwd(const float* x, long long rows, int channels, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                                  int training, int relu, float* y, float* save_mean, float* save_rstd, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    SSDK_REQUIRE(x && y && save_mean && save_rstd && rows > 0 && channels > 0, SSDK_E_INVALID, "ssdk_batchnorm_fwd: bad arguments");
    SSDK_REQUIRE(channels % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, SSDK_E_UNSUPPORTED,
                 "ssdk_batchnorm_fwd: channels %% 4 != 0 or buffers not 16-byte aligned");
    SSDK_REQUIRE(training || (running_mean && running_var), SSDK_E_INVALID, "ssdk_batchnorm_fwd: eval mode needs running statistics");
    hipStream_t s = (hipStream_t)stream;
    if (training) {   // = ssdk_batchnorm_stats + ssdk_batchnorm_apply on this process's rows alone
        SSDK_REQUIRE(workspace && workspace_bytes >= ssdk_batchnorm_workspace_bytes(channels), SSDK_E_WORKSPACE, "ssdk_batchnorm_fwd: workspace too small");
        const int rc = ssdk_batchnorm_stats(x, rows, channels, (double*)workspace, stream);
        if (rc) return rc;
        return ssdk_batchnorm_apply(x, rows, channels, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, relu, y,
                                    save_mean, save_rstd, (const double*)workspace, 0, stream);
    }
    // evaluation mode: ONE launch -- the apply kernel takes mean / rstd from the running statistics itself (mean == NULL) and leaves
    // save_mean / save_rstd for a backward through the frozen norm (a launch of their own before: 8 per SSD-300 evaluation step)
    SSDK_REQUIRE((((uintptr_t)running_mean | (uintptr_t)running_var) & 15) == 0, SSDK_E_UNSUPPORTED, "ssdk_batchnorm_fwd: running statistics not 16-byte aligned");
    const long long n4 = rows * channels / 4;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(apply_blocks(n4, channels / 4)), dim3(256), 0, s, (const float4*)x, n4, channels / 4, (const float4*)nullptr,
                       (const float4*)nullptr, (const float4*)gamma, (const float4*)beta, relu, (float4*)y, (const double*)nullptr, rows, eps,
                       momentum, running_mean, running_var, save_mean, save_rstd, (long long*)nullptr, 0, (double*)nullptr);
    SSDK_CHECK_LAUNCH("bn_apply_kernel");
    return SSDK_OK;
}

static int bn_bwd_stats(const float* x, const float* y, const float* dy, long long rows, int channels, const float* save_mean,
                        const float* save_rstd, int relu, double* sums, bool zero_first, void* stream) {
    relu &= 1;   // (bit 1 -- the norm's input is a ReLU output -- concerns dx only: the sums are over the gradient of the norm's OUTPUT)
    SSDK_REQUIRE(x && dy && sums && save_mean && save_rstd && rows > 0 && channels > 0 && (!relu || y), SSDK_E_INVALID,
                 "ssdk_batchnorm_bwd_stats: bad arguments");
    SSDK_REQUIRE(channels % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)y) & 15) == 0, SSDK_E_UNSUPPORTED,
                 "ssdk_batchnorm_bwd_stats: channels %% 4 != 0 or buffers not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (zero_first) SSDK_CHECK_HIP(zero_async(sums, sizeof(double) * (2 * (size_t)channels + 2), s));
    const BnReducePlan p = bn_reduce_plan(rows, channels);
    SSDK_REQUIRE(p.row_blocks * p.slabs < (1ll << 31), SSDK_E_UNSUPPORTED, "ssdk_batchnorm_bwd_stats: %lld row blocks x %d slabs exceed the grid", p.row_blocks, p.slabs);
    hipLaunchKernelGGL(bn_reduce_kernel<1>, dim3((unsigned)(p.row_blocks * p.slabs)), dim3(256), 0, s, x, y, dy, rows, p.rows_per_block, channels,
                       p.slab, p.slabs, p.fold64, save_mean, save_rstd, relu, sums);
    SSDK_CHECK_LAUNCH("bn_reduce_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_batchnorm_bwd_stats(const float* x, const float* y, const float* dy, long long rows, int channels, const float* save_mean,
                                        const float* save_rstd, int relu, double* sums, void* stream) {
    return bn_bwd_stats(x, y, dy, rows, channels, save_mean, save_rstd, relu, sums, true, stream);
}

static int bn_bwd_apply(const float* x, const float* y, const float* dy, long long rows, int channels, const float* gamma,
                        const float* save_mean, const float* save_rstd, int relu, int training, const double* sums,
                        const double* sums_local, const double* total_rows, float* dx, float* dgamma, float* dbeta, double* zero_after,
                        float* zero_also, long long zero_also_floats, void* stream) {
    SSDK_REQUIRE(x && dy && dx && sums && save_mean && save_rstd && rows > 0 && channels > 0 && (!(relu & 1) || y), SSDK_E_INVALID,
                 "ssdk_batchnorm_bwd_apply: bad arguments");
    SSDK_REQUIRE(channels % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)y) & 15) == 0, SSDK_E_UNSUPPORTED,
                 "ssdk_batchnorm_bwd_apply: channels %% 4 != 0 or buffers not 16-byte aligned");
    SSDK_REQUIRE(!total_rows || total_rows == sums + 2 * (size_t)channels, SSDK_E_INVALID,
                 "ssdk_batchnorm_bwd_apply: total_rows must be the slot behind the sums (sums + 2 * channels) or NULL");
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(apply_blocks(rows * channels / 4, channels / 4)), dim3(256), 0, (hipStream_t)stream, x, y, dy, rows, channels,
                       save_mean, save_rstd, gamma, sums, sums_local ? sums_local : sums, total_rows ? 1 : 0, relu, training, dx, dgamma, dbeta,
                       zero_after, zero_also_floats > 0 ? zero_also : (float*)nullptr, zero_also_floats);
    SSDK_CHECK_LAUNCH("bn_bwd_apply_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_batchnorm_bwd_apply(const float* x, const float* y, const float* dy, long long rows, int channels, const float* gamma,
                                        const float* save_mean, const float* save_rstd, int relu, int training, const double* sums,
                                        const double* sums_local, const double* total_rows, float* dx, float* dgamma, float* dbeta,
                                        void* stream) {
    return bn_bwd_apply(x, y, dy, rows, channels, gamma, save_mean, save_rstd, relu, training, sums, sums_local, total_rows, dx, dgamma, dbeta,
                        nullptr, nullptr, 0, stream);
}

// backward of ssdk_batchnorm_fwd_chained: `sums` (zeroed by the forward's apply launch) takes the backward sums, `zero_after` -- the
// layer's forward buffer -- is zero-filled for the next forward.  _ex: the apply launch also zero-fills zero_also[0 .. zero_also_floats)
// (any float count, 4-byte aligned start; NULL or 0: none) -- the caller's next accumulation target, the producing convolution's dx.
extern "C" int ssdk_batchnorm_bwd_chained_ex(const float* x, const float* y, const float* dy, long long rows, int channels, const float* gamma,
                                             const float* save_mean, const float* save_rstd, int relu, float* dx, float* dgamma, float* dbeta,
                                             double* sums, double* zero_after, float* zero_also, long long zero_also_floats, void* stream) {
    SSDK_REQUIRE(sums && sums != zero_after && dx, SSDK_E_INVALID, "ssdk_batchnorm_bwd_chained: bad arguments");
    SSDK_REQUIRE(zero_also_floats >= 0 && ((uintptr_t)zero_also & 3) == 0, SSDK_E_INVALID,
                 "ssdk_batchnorm_bwd_chained_ex: zero_also must be 4-byte aligned, its float count not negative");
    if (const int bad = bn_bwd_check("ssdk_batchnorm_bwd_chained", x, y, dy, dx, save_mean, save_rstd, rows, channels, relu)) return bad;
    const int rc = bn_bwd_stats(x, y, dy, rows, channels, save_mean, save_rstd, relu, sums, false, stream);
    if (rc) return rc;
    return bn_bwd_apply(x, y, dy, rows, channels, gamma, save_mean, save_rstd, relu, 1, sums, nullptr, nullptr, dx, dgamma, dbeta, zero_after, zero_also,
                        zero_also_floats, stream);
}

extern "C" int ssdk_batchnorm_bwd_chained(const float* x, const float* y, const float* dy, long long rows, int channels, const float* gamma,
                                          const float* save_mean, const float* save_rstd, int relu, float* dx, float* dgamma, float* dbeta,
                                          double* sums, double* zero_after, void* stream) {
    return ssdk_batchnorm_bwd_chained_ex(x, y, dy, rows, channels, gamma, save_mean, save_rstd, relu, dx, dgamma, dbeta, sums, zero_after, nullptr, 0,
                                         stream);
}

extern "C" int ssdk_batchnorm_bwd(const float* x, const float* y, const float* dy, long long rows, int channels, const float* gamma,
                                  const float* save_mean, const float* save_rstd, int relu, int training, float* dx, float* dgamma,
                                  float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int bad = bn_bwd_check("ssdk_batchnorm_bwd", x, y, dy, dx, save_mean, save_rstd, rows, channels, relu)) return bad;
    SSDK_REQUIRE(workspace && workspace_bytes >= ssdk_batchnorm_workspace_bytes(channels), SSDK_E_WORKSPACE, "ssdk_batchnorm_bwd: workspace too small");
    const int rc = ssdk_batchnorm_bwd_stats(x, y, dy, rows, channels, save_mean, save_rstd, relu, (double*)workspace, stream);
    if (rc) return rc;
    return ssdk_batchnorm_bwd_apply(x, y, dy, rows, channels, gamma, save_mean, save_rstd, relu, training, (const double*)workspace, nullptr, nullptr,
                                    dx, dgamma, dbeta, stream);
}

// dx = (y > 0) ? dy : 0  -- undoes a ReLU that was fused into a convolution epilogue (predictors.py:67-68)
namespace ssdk {
__global__ void __launch_bounds__(256) relu_bwd_kernel(const float4* __restrict__ y, const float4* __restrict__ dy, long long n4, float4* __restrict__ dx) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 a = y[i], g = dy[i];
        dx[i] = make_float4(a.x > 0.f ? g.x : 0.f, a.y > 0.f ? g.y : 0.f, a.z > 0.f ? g.z : 0.f, a.w > 0.f ? g.w : 0.f);
    }
}
}  // namespace ssdk

extern "C" int ssdk_relu_bwd(const float* y, const float* dy, long long n, float* dx, void* stream) {
    SSDK_REQUIRE(y && dy && dx && n > 0 && n % 4 == 0, SSDK_E_INVALID, "ssdk_relu_bwd: bad arguments (n %% 4 == 0)");
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(stream_blocks(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)y, (const float4*)dy, n / 4, (float4*)dx);
    SSDK_CHECK_LAUNCH("relu_bwd_kernel");
    return SSDK_OK;
}

// ---- FPN top-down step: out = fine + nearest_upsample(coarse) -------------------------------------
// Reference: bf/modules/features.py:106-107  features[i] += F.interpolate(features[i+1], size=features[i].size()[2:],
// mode='nearest').  torch 'nearest': src = min(floor(dst * (float)in / out), in - 1).
namespace ssdk {
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}

__global__ void __launch_bounds__(256) upsample_add_kernel(const float4* __restrict__ fine, const float4* __restrict__ coarse, int B, int Hf,
                                                           int Wf, int Hc, int Wc, int C4, float4* __restrict__ out) {
    const long long total = (long long)B * Hf * Wf * C4;
    const float sh = (float)Hc / (float)Hf, sw = (float)Wc / (float)Wf;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long p = i / C4;
        const int x = (int)(p % Wf); p /= Wf;
        const int y = (int)(p % Hf);
        const int b = (int)(p / Hf);
        const float4 a = fine ? fine[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 u = coarse[(((long long)b * Hc + nearest_src(y, sh, Hc)) * Wc + nearest_src(x, sw, Wc)) * C4 + c];
        out[i] = make_float4(a.x + u.x, a.y + u.y, a.z + u.z, a.w + u.w);
    }
}

// dcoarse[yc][xc] = sum of dout over the fine pixels whose nearest source is (yc, xc)  (gather form: deterministic)
__global__ void __launch_bounds__(256) upsample_add_bwd_kernel(const float4* __restrict__ dout, int B, int Hf, int Wf, int Hc, int Wc, int C4,
                                                               float4* __restrict__ dcoarse) {
    const long long total = (long long)B * Hc * Wc * C4;
    const float sh = (float)Hc / (float)Hf, sw = (float)Wc / (float)Wf;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long p = i / C4;
        const int xc = (int)(p % Wc); p /= Wc;
        const int yc = (int)(p % Hc);
        const int b = (int)(p / Hc);
        // candidate fine rows/cols: around yc / sh
        const int y0 = max(0, (int)floorf((float)yc / sh) - 2), y1 = min(Hf - 1, (int)ceilf((float)(yc + 1) / sh) + 2);
        const int x0 = max(0, (int)floorf((float)xc / sw) - 2), x1 = min(Wf - 1, (int)ceilf((float)(xc + 1) / sw) + 2);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int y = y0; y <= y1; ++y) {
            if (nearest_src(y, sh, Hc) != yc) continue;
            for (int x = x0; x <= x1; ++x) {
                if (nearest_src(x, sw, Wc) != xc) continue;
                const float4 g = dout[(((long long)b * Hf + y) * Wf + x) * C4 + c];
                s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
            }
        }
        dcoarse[i] = s;
    }
}
}  // namespace ssdk

extern "C" int ssdk_upsample_nearest_add_fwd(const float* fine, const float* coarse, int batch, int hf, int wf, int hc, int wc, int channels,
                                             float* out, void* stream) {
    SSDK_REQUIRE(coarse && out && batch > 0 && hf > 0 && wf > 0 && hc > 0 && wc > 0 && channels > 0 && channels % 4 == 0, SSDK_E_INVALID,
                 "ssdk_upsample_nearest_add_fwd: bad arguments (channels %% 4 == 0)");
    const long long n4 = (long long)batch * hf * wf * channels / 4;
    hipLaunchKernelGGL(upsample_add_kernel, dim3(stream_blocks(n4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)fine, (const float4*)coarse,
                       batch, hf, wf, hc, wc, channels / 4, (float4*)out);
    SSDK_CHECK_LAUNCH("upsample_add_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_upsample_nearest_add_bwd(const float* dout, int batch, int hf, int wf, int hc, int wc, int channels, float* dcoarse,
                                             void* stream) {
    SSDK_REQUIRE(dout && dcoarse && batch > 0 && hf > 0 && wf > 0 && hc > 0 && wc > 0 && channels > 0 && channels % 4 == 0, SSDK_E_INVALID,
                 "ssdk_upsample_nearest_add_bwd: bad arguments (channels %% 4 == 0)");
    const long long n4 = (long long)batch * hc * wc * channels / 4;
    hipLaunchKernelGGL(upsample_add_bwd_kernel, dim3(stream_blocks(n4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)dout, batch, hf, wf,
                       hc, wc, channels / 4, (float4*)dcoarse);
    SSDK_CHECK_LAUNCH("upsample_add_bwd_kernel");
    return SSDK_OK;
}

// ---- the same step in bilinear mode: out = [fine +] bilinear_upsample(coarse) ----------------------------------------
// Reference: bf/modules/features.py:107-108, :264-265, :371-373 with interpolation_mode='bilinear', which F.interpolate runs with
// align_corners=False.  Per axis: src = max(in / out * (dst + 0.5) - 0.5, 0), i0 = min((int)src, in - 1), i1 = i0 + (i0 < in - 1),
// l1 = clamp(src - i0, 0, 1), l0 = 1 - l1; out = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).  Any pair of sizes: upscaling,
// equal sizes (l1 == 0: the identity), downscaling (still two taps per axis, no antialiasing), in == 1 (i0 == i1 == 0).
namespace ssdk {
struct BilinearTap {
    int i0, i1;
    float l0, l1;
};

// The taps of output index `dst` along one axis.  The ONLY place they are computed: the backward kernel calls it for every candidate pixel,
// so it is the adjoint of the forward as computed, bit for bit, not of a second derivation.  (The explicit fused multiply-add keeps the
// compiler from contracting the two inlined copies differently.)
__device__ __forceinline__ BilinearTap bilinear_tap(int dst, float scale, int in) {
    const float src = fmaxf(__fmaf_rn(scale, (float)dst + 0.5f, -0.5f), 0.f);
    BilinearTap t;
    t.i0 = min((int)src, in - 1);
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
    t.l0 = 1.f - t.l1;
    return t;
}

__global__ void __launch_bounds__(256) upsample_bilinear_add_kernel(const float4* __restrict__ fine, const float4* __restrict__ coarse, int B,
                                                                    int Hf, int Wf, int Hc, int Wc, int C4, float4* __restrict__ out) {
    const long long total = (long long)B * Hf * Wf * C4;
    const float sh = (float)Hc / (float)Hf, sw = (float)Wc / (float)Wf;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long p = i / C4;
        const int x = (int)(p % Wf); p /= Wf;
        const int y = (int)(p % Hf);
        const int b = (int)(p / Hf);
        const BilinearTap ty = bilinear_tap(y, sh, Hc), tx = bilinear_tap(x, sw, Wc);
        const float4* r0 = coarse + ((long long)b * Hc + ty.i0) * Wc * C4 + c;
        const float4* r1 = coarse + ((long long)b * Hc + ty.i1) * Wc * C4 + c;
        const float4 v00 = r0[(long long)tx.i0 * C4], v01 = r0[(long long)tx.i1 * C4];
        const float4 v10 = r1[(long long)tx.i0 * C4], v11 = r1[(long long)tx.i1 * C4];
        float4 u;
        u.x = ty.l0 * (tx.l0 * v00.x + tx.l1 * v01.x) + ty.l1 * (tx.l0 * v10.x + tx.l1 * v11.x);
        u.y = ty.l0 * (tx.l0 * v00.y + tx.l1 * v01.y) + ty.l1 * (tx.l0 * v10.y + tx.l1 * v11.y);
        u.z = ty.l0 * (tx.l0 * v00.z + tx.l1 * v01.z) + ty.l1 * (tx.l0 * v10.z + tx.l1 * v11.z);
        u.w = ty.l0 * (tx.l0 * v00.w + tx.l1 * v01.w) + ty.l1 * (tx.l0 * v10.w + tx.l1 * v11.w);
        if (fine) {
            const float4 a = fine[i];
            u = make_float4(a.x + u.x, a.y + u.y, a.z + u.z, a.w + u.w);
        }
        out[i] = u;
    }
}

// First and last candidate output index that can have a tap at input index `c`: i0 == c or i1 == c needs src in (c - 1, c + 1), i.e.
// dst in ((c - 0.5) / scale - 0.5, (c + 1.5) / scale - 0.5); the clamp of src at 0 only moves pixels onto c == 0, whose window starts at 0
// anyway.  Widened by 2 on either side: the fp32 window and the fp32 src are each off by less than out * 2^-21, far below 1 for any map.
// Every candidate's taps are recomputed and tested, so a wide window costs time, never correctness.  Empty (lo > hi) when downscaling skips
// the index.
__device__ __forceinline__ void bilinear_window(int c, float scale, int out, int& lo, int& hi) {
    lo = max(0, (int)floorf(((float)c - 0.5f) / scale - 0.5f) - 2);
    hi = min(out - 1, (int)ceilf(((float)c + 1.5f) / scale - 0.5f) + 2);
}

// dcoarse[yc][xc] = sum over the fine pixels with a tap at (yc, xc) of (row weight) * (column weight) * dout -- Wy^T . G . Wx in gather
// form: rows and columns in ascending order, no atomics, every element written (zeros where the window is empty): deterministic.
__global__ void __launch_bounds__(256) upsample_bilinear_add_bwd_kernel(const float4* __restrict__ dout, int B, int Hf, int Wf, int Hc, int Wc,
                                                                        int C4, float4* __restrict__ dcoarse) {
    const long long total = (long long)B * Hc * Wc * C4;
    const float sh = (float)Hc / (float)Hf, sw = (float)Wc / (float)Wf;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long p = i / C4;
        const int xc = (int)(p % Wc); p /= Wc;
        const int yc = (int)(p % Hc);
        const int b = (int)(p / Hc);
        int y0, y1, x0, x1;
        bilinear_window(yc, sh, Hf, y0, y1);
        bilinear_window(xc, sw, Wf, x0, x1);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int y = y0; y <= y1; ++y) {
            const BilinearTap ty = bilinear_tap(y, sh, Hc);
            if (ty.i0 != yc && ty.i1 != yc) continue;
            const float wy = (ty.i0 == yc ? ty.l0 : 0.f) + (ty.i1 == yc ? ty.l1 : 0.f);   // (both at the far edge and when Hc == 1)
            const float4* row = dout + ((long long)b * Hf + y) * Wf * C4 + c;
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int x = x0; x <= x1; ++x) {
                const BilinearTap tx = bilinear_tap(x, sw, Wc);
                if (tx.i0 != xc && tx.i1 != xc) continue;
                const float wx = (tx.i0 == xc ? tx.l0 : 0.f) + (tx.i1 == xc ? tx.l1 : 0.f);
                const float4 g = row[(long long)x * C4];
                r.x += wx * g.x; r.y += wx * g.y; r.z += wx * g.z; r.w += wx * g.w;
            }
            s.x += wy * r.x; s.y += wy * r.y; s.z += wy * r.z; s.w += wy * r.w;
        }
        dcoarse[i] = s;
    }
}
}  // namespace ssdk

extern "C" int ssdk_upsample_bilinear_add_fwd(const float* fine, const float* coarse, int batch, int hf, int wf, int hc, int wc, int channels,
                                              float* out, void* stream) {
    SSDK_REQUIRE(coarse && out && batch > 0 && hf > 0 && wf > 0 && hc > 0 && wc > 0 && channels > 0 && channels % 4 == 0, SSDK_E_INVALID,
                 "ssdk_upsample_bilinear_add_fwd: bad arguments (channels %% 4 == 0)");
    const long long n4 = (long long)batch * hf * wf * channels / 4;
    hipLaunchKernelGGL(upsample_bilinear_add_kernel, dim3(stream_blocks(n4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)fine,
                       (const float4*)coarse, batch, hf, wf, hc, wc, channels / 4, (float4*)out);
    SSDK_CHECK_LAUNCH("upsample_bilinear_add_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_upsample_bilinear_add_bwd(const float* dout, int batch, int hf, int wf, int hc, int wc, int channels, float* dcoarse,
                                              void* stream) {
    SSDK_REQUIRE(dout && dcoarse && batch > 0 && hf > 0 && wf > 0 && hc > 0 && wc > 0 && channels > 0 && channels % 4 == 0, SSDK_E_INVALID,
                 "ssdk_upsample_bilinear_add_bwd: bad arguments (channels %% 4 == 0)");
    const long long n4 = (long long)batch * hc * wc * channels / 4;
    hipLaunchKernelGGL(upsample_bilinear_add_bwd_kernel, dim3(stream_blocks(n4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)dout,
                       batch, hf, wf, hc, wc, channels / 4, (float4*)dcoarse);
    SSDK_CHECK_LAUNCH("upsample_bilinear_add_bwd_kernel");
    return SSDK_OK;
}


// ---- SFAM (M2Det scale-wise feature aggregation): squeeze-excite gate ---------------------------------
// Reference: bf/modules/features.py:286-298  x = adaptive_avg_pool2d(f, 1); x = fc2(relu(fc1(x))); out = f * sigmoid(x).
// The two 1x1 "fc" convolutions run on the GEMM kernels; these are the pool and the gate (with their backward).
namespace ssdk {
// mean over the HW pixels of each image: x [B][HW][C] -> out [B][C].  One workgroup per (image, 16-float4 column block): thread
// (column q of 16, row phase r of 16); a wave instruction reads four rows x 256 contiguous bytes, four row groups are in flight per
// thread, the 16 phases are folded through LDS.  (Round 3's form -- 64 columns per workgroup, one row in flight per wave -- put M2Det's
// SFAM pool of a [16, 1024, 64, 64] map, 268 MB, on 64 workgroups: ~600 us; this one uses 256.)
constexpr int kPoolCols = 16;   // float4 columns per workgroup
__global__ void __launch_bounds__(256) avgpool_kernel(const float4* __restrict__ x, int HW, int C4, float4* __restrict__ out) {
    __shared__ float4 s_part[16][kPoolCols];
    const int b = blockIdx.y, q = threadIdx.x & (kPoolCols - 1), r = threadIdx.x / kPoolCols;
    const int c4 = blockIdx.x * kPoolCols + q;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < C4) {
        const float4* base = x + (long long)b * HW * C4 + c4;
        int p = r;
        for (; p + 48 < HW; p += 64) {   // rows p, p + 16, p + 32, p + 48: four loads in flight
            const float4 v0 = base[(long long)p * C4], v1 = base[(long long)(p + 16) * C4], v2 = base[(long long)(p + 32) * C4], v3 = base[(long long)(p + 48) * C4];
            a.x += (v0.x + v1.x) + (v2.x + v3.x); a.y += (v0.y + v1.y) + (v2.y + v3.y);
            a.z += (v0.z + v1.z) + (v2.z + v3.z); a.w += (v0.w + v1.w) + (v2.w + v3.w);
        }
        for (; p < HW; p += 16) {
            const float4 v = base[(long long)p * C4];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
    }
    s_part[r][q] = a;
    __syncthreads();
    if (r == 0 && c4 < C4) {
        float4 t = s_part[0][q];
        for (int w = 1; w < 16; ++w) { const float4 u = s_part[w][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        const float inv = 1.0f / (float)HW;
        out[(long long)b * C4 + c4] = make_float4(t.x * inv, t.y * inv, t.z * inv, t.w * inv);
    }
}
__global__ void __launch_bounds__(256) avgpool_bwd_kernel(const float4* __restrict__ dout, int B, int HW, int C4, float4* __restrict__ dx) {
    const long long total = (long long)B * HW * C4;
    const float inv = 1.0f / (float)HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        const int b = (int)(i / ((long long)HW * C4));
        const float4 g = dout[(long long)b * C4 + c];
        dx[i] = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv);
    }
}
__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + __expf(-v)); }
// out = x * sigmoid(z[b][c])
__global__ void __launch_bounds__(256) gate_kernel(const float4* __restrict__ x, const float4* __restrict__ z, int B, int HW, int C4,
                                                   float4* __restrict__ out) {
    const long long total = (long long)B * HW * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        const int b = (int)(i / ((long long)HW * C4));
        const float4 v = x[i], q = z[(long long)b * C4 + c];
        out[i] = make_float4(v.x * sigm(q.x), v.y * sigm(q.y), v.z * sigm(q.z), v.w * sigm(q.w));
    }
}
// dx = dout * sigmoid(z);  dz[b][c] = sigmoid'(z) * sum_hw dout * x   (one workgroup per (image, 16-float4 column block), as avgpool_kernel)
__global__ void __launch_bounds__(256) gate_bwd_kernel(const float4* __restrict__ x, const float4* __restrict__ z, const float4* __restrict__ dout,
                                                       int HW, int C4, float4* __restrict__ dx, float4* __restrict__ dz) {
    __shared__ float4 s_part[16][kPoolCols];
    const int b = blockIdx.y, q = threadIdx.x & (kPoolCols - 1), r = threadIdx.x / kPoolCols;
    const int c4 = blockIdx.x * kPoolCols + q;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), sg = a;
    if (c4 < C4) {
        const float4 zq = z[(long long)b * C4 + c4];
        sg = make_float4(sigm(zq.x), sigm(zq.y), sigm(zq.z), sigm(zq.w));
        const long long base = (long long)b * HW * C4 + c4;
        int p = r;
        for (; p + 16 < HW; p += 32) {   // two rows (of both operands) in flight
            const long long i0 = base + (long long)p * C4, i1 = base + (long long)(p + 16) * C4;
            const float4 g0 = dout[i0], v0 = x[i0], g1 = dout[i1], v1 = x[i1];
            dx[i0] = make_float4(g0.x * sg.x, g0.y * sg.y, g0.z * sg.z, g0.w * sg.w);
            dx[i1] = make_float4(g1.x * sg.x, g1.y * sg.y, g1.z * sg.z, g1.w * sg.w);
            a.x += g0.x * v0.x + g1.x * v1.x; a.y += g0.y * v0.y + g1.y * v1.y; a.z += g0.z * v0.z + g1.z * v1.z; a.w += g0.w * v0.w + g1.w * v1.w;
        }
        for (; p < HW; p += 16) {
            const long long i = base + (long long)p * C4;
            const float4 g = dout[i], v = x[i];
            dx[i] = make_float4(g.x * sg.x, g.y * sg.y, g.z * sg.z, g.w * sg.w);
            a.x += g.x * v.x; a.y += g.y * v.y; a.z += g.z * v.z; a.w += g.w * v.w;
        }
    }
    s_part[r][q] = a;
    __syncthreads();
    if (r == 0 && c4 < C4) {
        float4 t = s_part[0][q];
        for (int w = 1; w < 16; ++w) { const float4 u = s_part[w][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        dz[(long long)b * C4 + c4] = make_float4(t.x * sg.x * (1.f - sg.x), t.y * sg.y * (1.f - sg.y), t.z * sg.z * (1.f - sg.z), t.w * sg.w * (1.f - sg.w));
    }
}
}  // namespace ssdk

static int check_bhwc(const char* fn, int batch, int hw, int channels) {
    SSDK_REQUIRE(batch > 0 && batch <= 65535 && hw > 0 && channels > 0 && channels % 4 == 0, SSDK_E_INVALID, "%s: batch=%d hw=%d channels=%d (%% 4 == 0)", fn, batch, hw, channels);
    return SSDK_OK;
}

extern "C" int ssdk_global_avgpool_fwd(const float* x, int batch, int hw, int channels, float* out, void* stream) {
    int rc = check_bhwc("ssdk_global_avgpool_fwd", batch, hw, channels);
    if (rc) return rc;
    SSDK_REQUIRE(x && out, SSDK_E_INVALID, "ssdk_global_avgpool_fwd: null pointer");
    hipLaunchKernelGGL(avgpool_kernel, dim3(cdiv(channels / 4, ssdk::kPoolCols), batch), dim3(256), 0, (hipStream_t)stream, (const float4*)x, hw, channels / 4, (float4*)out);
    SSDK_CHECK_LAUNCH("avgpool_kernel");
    return SSDK_OK;
}
extern "C" int ssdk_global_avgpool_bwd(const float* dout, int batch, int hw, int channels, float* dx, void* stream) {
    int rc = check_bhwc("ssdk_global_avgpool_bwd", batch, hw, channels);
    if (rc) return rc;
    SSDK_REQUIRE(dout && dx, SSDK_E_INVALID, "ssdk_global_avgpool_bwd: null pointer");
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(stream_blocks((long long)batch * hw * channels / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)dout, batch, hw, channels / 4, (float4*)dx);
    SSDK_CHECK_LAUNCH("avgpool_bwd_kernel");
    return SSDK_OK;
}
extern "C" int ssdk_sigmoid_gate_fwd(const float* x, const float* z, int batch, int hw, int channels, float* out, void* stream) {
    int rc = check_bhwc("ssdk_sigmoid_gate_fwd", batch, hw, channels);
    if (rc) return rc;
    SSDK_REQUIRE(x && z && out, SSDK_E_INVALID, "ssdk_sigmoid_gate_fwd: null pointer");
    hipLaunchKernelGGL(gate_kernel, dim3(stream_blocks((long long)batch * hw * channels / 4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)x,
                       (const float4*)z, batch, hw, channels / 4, (float4*)out);
    SSDK_CHECK_LAUNCH("gate_kernel");
    return SSDK_OK;
}
extern "C" int ssdk_sigmoid_gate_bwd(const float* x, const float* z, const float* dout, int batch, int hw, int channels, float* dx, float* dz,
                                     void* stream) {
    int rc = check_bhwc("ssdk_sigmoid_gate_bwd", batch, hw, channels);
    if (rc) return rc;
    SSDK_REQUIRE(x && z && dout && dx && dz, SSDK_E_INVALID, "ssdk_sigmoid_gate_bwd: null pointer");
    hipLaunchKernelGGL(gate_bwd_kernel, dim3(cdiv(channels / 4, ssdk::kPoolCols), batch), dim3(256), 0, (hipStream_t)stream, (const float4*)x, (const float4*)z,
                       (const float4*)dout, hw, channels / 4, (float4*)dx, (float4*)dz);
    SSDK_CHECK_LAUNCH("gate_bwd_kernel");
    return SSDK_OK;
}

// ---- SFAM over PIECES ------------------------------------------------------------------------------------------------------------
// The reference concatenates the eight TUM outputs of a scale (features.py:385, torch.cat of [B, 128, H, W] maps) and hands the
// [B, 1024, H, W] map to the gate (:286-298).  The concatenated map is never needed as such: the pool and the gate read the pieces where
// they are and the gate writes the one map the heads read; the backward pass writes each piece's gradient as its own contiguous map --
// dout * sigmoid(z) + dpool / HW in ONE pass (torch.cat's backward made eight strided slices that every consumer first copied, and
// autograd added the pool's and the gate's gradient maps with one more pass).
namespace ssdk {
constexpr int kMaxPieces = 8;
struct Pieces {
    const float4* p[kMaxPieces];
    int n, Cp4;   // pieces, float4 columns per piece
};
struct PiecesOut {
    float4* p[kMaxPieces];
    int n, Cp4;
};
// mean over the pixels of every image: pieces [B][HW][Cp] -> out [B][n * Cp]   (avgpool_kernel's layout of the work)
__global__ void __launch_bounds__(256) pool_pieces_kernel(Pieces ps, int HW, float4* __restrict__ out) {
    __shared__ float4 s_part[16][kPoolCols];
    const int C4 = ps.n * ps.Cp4;
    const int b = blockIdx.y, q = threadIdx.x & (kPoolCols - 1), r = threadIdx.x / kPoolCols;
    const int c4 = blockIdx.x * kPoolCols + q;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < C4) {
        const int k = c4 / ps.Cp4, w = c4 - k * ps.Cp4;
        const int Cp4 = ps.Cp4;
        const float4* base = ps.p[k] + (long long)b * HW * Cp4 + w;
        int p = r;
        for (; p + 48 < HW; p += 64) {
            const float4 v0 = base[(long long)p * Cp4], v1 = base[(long long)(p + 16) * Cp4], v2 = base[(long long)(p + 32) * Cp4], v3 = base[(long long)(p + 48) * Cp4];
            a.x += (v0.x + v1.x) + (v2.x + v3.x); a.y += (v0.y + v1.y) + (v2.y + v3.y);
            a.z += (v0.z + v1.z) + (v2.z + v3.z); a.w += (v0.w + v1.w) + (v2.w + v3.w);
        }
        for (; p < HW; p += 16) {
            const float4 v = base[(long long)p * Cp4];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
    }
    s_part[r][q] = a;
    __syncthreads();
    if (r == 0 && c4 < C4) {
        float4 t = s_part[0][q];
        for (int w = 1; w < 16; ++w) { const float4 u = s_part[w][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        const float inv = 1.0f / (float)HW;
        out[(long long)b * C4 + c4] = make_float4(t.x * inv, t.y * inv, t.z * inv, t.w * inv);
    }
}
// out [B][HW][n * Cp] = piece * sigmoid(z[b][c])
__global__ void __launch_bounds__(256) gate_pieces_kernel(Pieces ps, const float4* __restrict__ z, int B, int HW, float4* __restrict__ out) {
    const int C4 = ps.n * ps.Cp4, Cp4 = ps.Cp4;
    const long long total = (long long)B * HW * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / C4;
        const int c = (int)(i - row * C4);
        const int b = (int)(row / HW);
        const int k = c / Cp4, w = c - k * Cp4;
        const float4 v = ps.p[k][row * Cp4 + w], q = z[(long long)b * C4 + c];
        out[i] = make_float4(v.x * sigm(q.x), v.y * sigm(q.y), v.z * sigm(q.z), v.w * sigm(q.w));
    }
}
// dz[b][c] = sigmoid'(z) * sum_hw dout * piece   (gate_bwd_kernel's reduction; the data gradient waits for dpool: gate_bwd_pieces_kernel)
__global__ void __launch_bounds__(256) gate_bwd_reduce_pieces_kernel(Pieces ps, const float4* __restrict__ z, const float4* __restrict__ dout, int HW,
                                                                     float4* __restrict__ dz) {
    __shared__ float4 s_part[16][kPoolCols];
    const int C4 = ps.n * ps.Cp4, Cp4 = ps.Cp4;
    const int b = blockIdx.y, q = threadIdx.x & (kPoolCols - 1), r = threadIdx.x / kPoolCols;
    const int c4 = blockIdx.x * kPoolCols + q;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < C4) {
        const int k = c4 / Cp4, w = c4 - k * Cp4;
        const float4* xb = ps.p[k] + (long long)b * HW * Cp4 + w;
        const float4* gb = dout + (long long)b * HW * C4 + c4;
        int p = r;
        for (; p + 16 < HW; p += 32) {
            const float4 g0 = gb[(long long)p * C4], v0 = xb[(long long)p * Cp4], g1 = gb[(long long)(p + 16) * C4], v1 = xb[(long long)(p + 16) * Cp4];
            a.x += g0.x * v0.x + g1.x * v1.x; a.y += g0.y * v0.y + g1.y * v1.y; a.z += g0.z * v0.z + g1.z * v1.z; a.w += g0.w * v0.w + g1.w * v1.w;
        }
        for (; p < HW; p += 16) {
            const float4 g = gb[(long long)p * C4], v = xb[(long long)p * Cp4];
            a.x += g.x * v.x; a.y += g.y * v.y; a.z += g.z * v.z; a.w += g.w * v.w;
        }
    }
    s_part[r][q] = a;
    __syncthreads();
    if (r == 0 && c4 < C4) {
        float4 t = s_part[0][q];
        for (int w = 1; w < 16; ++w) { const float4 u = s_part[w][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        const float4 zq = z[(long long)b * C4 + c4];
        const float4 sg = make_float4(sigm(zq.x), sigm(zq.y), sigm(zq.z), sigm(zq.w));
        dz[(long long)b * C4 + c4] = make_float4(t.x * sg.x * (1.f - sg.x), t.y * sg.y * (1.f - sg.y), t.z * sg.z * (1.f - sg.z), t.w * sg.w * (1.f - sg.w));
    }
}
// dpiece_k [B][HW][Cp] = dout[.., k * Cp + c] * sigmoid(z) + dpool[b][k * Cp + c] / HW   (the gate's and the pool's gradient in one pass)
__global__ void __launch_bounds__(256) gate_bwd_pieces_kernel(PiecesOut ds, const float4* __restrict__ z, const float4* __restrict__ dout,
                                                              const float4* __restrict__ dpool, int B, int HW) {
    const int C4 = ds.n * ds.Cp4, Cp4 = ds.Cp4;
    const long long total = (long long)B * HW * C4;
    const float inv = 1.0f / (float)HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / C4;
        const int c = (int)(i - row * C4);
        const int b = (int)(row / HW);
        const int k = c / Cp4, w = c - k * Cp4;
        const float4 g = dout[i], q = z[(long long)b * C4 + c], dp = dpool[(long long)b * C4 + c];
        ds.p[k][row * Cp4 + w] = make_float4(g.x * sigm(q.x) + dp.x * inv, g.y * sigm(q.y) + dp.y * inv, g.z * sigm(q.z) + dp.z * inv, g.w * sigm(q.w) + dp.w * inv);
    }
}
}  // namespace ssdk

static int check_pieces(const char* fn, const float* const* pieces, int n_pieces, int batch, int hw, int piece_channels) {
    SSDK_REQUIRE(pieces && n_pieces > 0 && n_pieces <= ssdk::kMaxPieces, SSDK_E_INVALID, "%s: n_pieces=%d (1..%d)", fn, n_pieces, ssdk::kMaxPieces);
    SSDK_REQUIRE(batch > 0 && batch <= 65535 && hw > 0 && piece_channels > 0 && piece_channels % 4 == 0, SSDK_E_INVALID,
                 "%s: batch=%d hw=%d piece_channels=%d (%% 4 == 0)", fn, batch, hw, piece_channels);
    for (int k = 0; k < n_pieces; ++k)
        SSDK_REQUIRE(pieces[k] && ((uintptr_t)pieces[k] & 15) == 0, SSDK_E_INVALID, "%s: piece %d is null or not 16-byte aligned", fn, k);
    return SSDK_OK;
}
extern "C" int ssdk_sfam_pool_fwd(const float* const* pieces, int n_pieces, int batch, int hw, int piece_channels, float* pooled, void* stream) {
    int rc = check_pieces("ssdk_sfam_pool_fwd", pieces, n_pieces, batch, hw, piece_channels);
    if (rc) return rc;
    SSDK_REQUIRE(pooled, SSDK_E_INVALID, "ssdk_sfam_pool_fwd: null output");
    ssdk::Pieces ps{};
    ps.n = n_pieces; ps.Cp4 = piece_channels / 4;
    for (int k = 0; k < n_pieces; ++k) ps.p[k] = (const float4*)pieces[k];
    hipLaunchKernelGGL(pool_pieces_kernel, dim3(cdiv(n_pieces * piece_channels / 4, ssdk::kPoolCols), batch), dim3(256), 0, (hipStream_t)stream, ps, hw, (float4*)pooled);
    SSDK_CHECK_LAUNCH("pool_pieces_kernel");
    return SSDK_OK;
}
extern "C" int ssdk_sfam_gate_fwd(const float* const* pieces, int n_pieces, int batch, int hw, int piece_channels, const float* z, float* out,
                                  void* stream) {
    int rc = check_pieces("ssdk_sfam_gate_fwd", pieces, n_pieces, batch, hw, piece_channels);
    if (rc) return rc;
    SSDK_REQUIRE(z && out, SSDK_E_INVALID, "ssdk_sfam_gate_fwd: null pointer");
    ssdk::Pieces ps{};
    ps.n = n_pieces; ps.Cp4 = piece_channels / 4;
    for (int k = 0; k < n_pieces; ++k) ps.p[k] = (const float4*)pieces[k];
    hipLaunchKernelGGL(gate_pieces_kernel, dim3(stream_blocks((long long)batch * hw * n_pieces * piece_channels / 4, 256)), dim3(256), 0, (hipStream_t)stream, ps,
                       (const float4*)z, batch, hw, (float4*)out);
    SSDK_CHECK_LAUNCH("gate_pieces_kernel");
    return SSDK_OK;
}
extern "C" int ssdk_sfam_gate_bwd_reduce(const float* const* pieces, int n_pieces, int batch, int hw, int piece_channels, const float* z,
                                         const float* dout, float* dz, void* stream) {
    int rc = check_pieces("ssdk_sfam_gate_bwd_reduce", pieces, n_pieces, batch, hw, piece_channels);
    if (rc) return rc;
    SSDK_REQUIRE(z && dout && dz, SSDK_E_INVALID, "ssdk_sfam_gate_bwd_reduce: null pointer");
    ssdk::Pieces ps{};
    ps.n = n_pieces; ps.Cp4 = piece_channels / 4;
    for (int k = 0; k < n_pieces; ++k) ps.p[k] = (const float4*)pieces[k];
    hipLaunchKernelGGL(gate_bwd_reduce_pieces_kernel, dim3(cdiv(n_pieces * piece_channels / 4, ssdk::kPoolCols), batch), dim3(256), 0, (hipStream_t)stream, ps,
                       (const float4*)z, (const float4*)dout, hw, (float4*)dz);
    SSDK_CHECK_LAUNCH("gate_bwd_reduce_pieces_kernel");
    return SSDK_OK;
}
extern "C" int ssdk_sfam_gate_bwd_apply(float* const* dpieces, int n_pieces, int batch, int hw, int piece_channels, const float* z, const float* dout,
                                        const float* dpool, void* stream) {
    int rc = check_pieces("ssdk_sfam_gate_bwd_apply", (const float* const*)dpieces, n_pieces, batch, hw, piece_channels);
    if (rc) return rc;
    SSDK_REQUIRE(z && dout && dpool, SSDK_E_INVALID, "ssdk_sfam_gate_bwd_apply: null pointer");
    ssdk::PiecesOut ds{};
    ds.n = n_pieces; ds.Cp4 = piece_channels / 4;
    for (int k = 0; k < n_pieces; ++k) ds.p[k] = (float4*)dpieces[k];
    hipLaunchKernelGGL(gate_bwd_pieces_kernel, dim3(stream_blocks((long long)batch * hw * n_pieces * piece_channels / 4, 256)), dim3(256), 0, (hipStream_t)stream, ds,
                       (const float4*)z, (const float4*)dout, (const float4*)dpool, batch, hw);
    SSDK_CHECK_LAUNCH("gate_bwd_pieces_kernel");
    return SSDK_OK;
}

// ---- depthwise convolution (bf/modules/conv.py:39-85) ----------------------------------------------------------------------
// HBM-bound stencils on NHWC maps: a thread owns 4 consecutive channels of one output pixel (16-byte loads / stores, the k*k
// weights of its channels in registers).  Backward-weights: every thread accumulates its pixels' products for its 4 channels,
// a workgroup reduces over its pixels through LDS and adds one partial per (channel, tap) with an atomic.
namespace ssdk {

constexpr int kDwMaxTaps = 25;   // up to 5 x 5

// One output element (4 channels of one pixel): the tap order and the fmaf chain that the single-level and the grouped kernels share.
__device__ __forceinline__ float4 dw_fwd_point(const float4* x, const float* w, const float* bias, int Hin, int Win, int C4,
                                               int ks, int taps, int stride, int pad, int Hout, int Wout, long long i) {
    const int c4 = (int)(i % C4);
    long long p = i / C4;
    const int xo = (int)(p % Wout); p /= Wout;
    const int yo = (int)(p % Hout);
    const int b = (int)(p / Hout);
    float4 acc = bias ? *reinterpret_cast<const float4*>(bias + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float* wc = w + (long long)c4 * 4 * taps;
    for (int ky = 0; ky < ks; ++ky) {
        const int iy = yo * stride - pad + ky;
        if (iy < 0 || iy >= Hin) continue;
        for (int kx = 0; kx < ks; ++kx) {
            const int ix = xo * stride - pad + kx;
            if (ix < 0 || ix >= Win) continue;
            const float4 v = x[((long long)(b * Hin + iy) * Win + ix) * C4 + c4];
            const int t = ky * ks + kx;
            acc.x = fmaf(wc[t], v.x, acc.x);
            acc.y = fmaf(wc[taps + t], v.y, acc.y);
            acc.z = fmaf(wc[2 * taps + t], v.z, acc.z);
            acc.w = fmaf(wc[3 * taps + t], v.w, acc.w);
        }
    }
    return acc;
}

__global__ void __launch_bounds__(256) dw_fwd_kernel(const float4* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int B, int Hin,
                                                     int Win, int C4, int ks, int stride, int pad, int Hout, int Wout, float4* __restrict__ y) {
    const long long total = (long long)B * Hout * Wout * C4;
    const int taps = ks * ks;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        y[i] = dw_fwd_point(x, w, bias, Hin, Win, C4, ks, taps, stride, pad, Hout, Wout, i);
}

// ---- the stencil of a depthwise Conv2dBn block (bf/modules/features.py:79-98: FeaturePyramid(use_depthwise=True) builds every
// pyramid_output block as Conv2dBn(C, C, 3, groups=C); bf/modules/conv.py:30-36: conv -> BatchNorm -> ReLU) ----
// Training: the stencil writes y and, in the same launch, adds the BatchNorm statistics of y to the layer's fp64 `sums` buffer -- the norm
// behind it is one apply launch and the statistics pass over the activation is gone.  y is dw_fwd_point's, so the same bits as dw_fwd_kernel.
//
// The grid is (row blocks) x (column slabs), slabs innermost, as bn_reduce_kernel's: a workgroup owns `slab` channel quads (a power of two,
// at most 16; the last slab of a C / 4 that slab does not divide is narrower, its spare lanes idle: C / 4 = 33) of rows_per_block output
// pixels.  Thread t owns quad t % slab of the slab and the rows t / slab, t / slab + 256 / slab, ...: its channel quad never changes, whatever
// C / 4 is, so its two fp64 accumulators are per-channel sums from the first add on (a flat grid-stride loop changes the quad from trip to
// trip unless the stride is a multiple of C / 4).  fp64 for bn_reduce_kernel<0>'s reason: the variance is E[y^2] - mean^2 and the square
// of an fp32 value is exact in fp64.  The lanes of a wave that share a quad are folded with cross-lane adds, the four waves through LDS,
// all in fp64, and the workgroup ends with ONE fp64 atomic per channel and sum.
//
// Contention rule (dw_stats_plan): the workgroups that add to one address are the ROW blocks.  A stencil point is nine independent loads
// and a store, far more work per row than a reduction's one load, and the launch needs many more workgroups than a reduction to cover the
// memory latency: the rule aims at 256 row blocks (bn_reduce_plan: 64), each a whole number of trips of its slab (256 / slab rows), one trip
// at the least -- a small map is all one-trip workgroups, as dw_fwd_kernel's one point per thread.  bn_rows_per_block's own measurement puts
// the price of the same-address atomics at 15 - 20 ns per adder (1 984 -> 256 adders: 53 -> 23 us), so 256 adders are ~5 us spread over
// the launch.  Measured (tools/bench_fpnlite.py, the neck at batch 32, forward + backward, SSDK_DW_STATS_WGS = 64 / 256 / 1024): 3.91 / 3.59 /
// 3.60 ms at 256 channels, 3.04 / 2.81 / 2.81 ms at 128 (profiles/fpnlite_bench.txt).  SSDK_DW_STATS_WGS overrides the target.
struct DwStatsPlan { int rows_per_block, slab, slabs; long long row_blocks; };
static inline DwStatsPlan dw_stats_plan(long long rows, int C4) {
    DwStatsPlan p;
    p.slab = bn_pow2_at_least(C4 < 16 ? C4 : 16);
    p.slabs = (C4 + p.slab - 1) / p.slab;
    const char* e = getenv("SSDK_DW_STATS_WGS");
    long long target = e ? atoll(e) : 256;
    if (target < 1) target = 1;
    const int rpt = 256 / p.slab;   // rows per trip of a workgroup
    long long r = (rows + target - 1) / target;
    r = (r + rpt - 1) / rpt * rpt;
    if (r < rpt) r = rpt;
    p.rows_per_block = (int)(r > (1 << 20) ? (1 << 20) : r);
    p.row_blocks = (rows + p.rows_per_block - 1) / p.rows_per_block;
    return p;
}

__global__ void __launch_bounds__(256) dw_stats_fwd_kernel(const float4* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int B,
                                                           int Hin, int Win, int C4, int ks, int stride, int pad, int Hout, int Wout, int rows_per_block,
                                                           int slab, int slabs, float4* __restrict__ y, double* __restrict__ sums) {
    __shared__ bn_acc4<double> s_part[2 * 4 * 64];   // [sum][wave][lane]
    const long long rows = (long long)B * Hout * Wout;
    const int C = C4 * 4, taps = ks * ks;
    const int my_slab = (int)(blockIdx.x % (unsigned)slabs);
    const long long r0 = (long long)(blockIdx.x / (unsigned)slabs) * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = threadIdx.x & (slab - 1), sub = threadIdx.x / slab, rpt = 256 / slab;
    const int c4 = my_slab * slab + col;
    if (blockIdx.x == 0 && threadIdx.x == 0) sums[2 * C] = (double)rows;   // (slot 2C: the count behind the sums)
    bn_acc4<double> a0 = {0, 0, 0, 0}, a1 = a0;
    if (c4 < C4) {
        for (long long r = r0 + sub; r < r1; r += rpt) {
            const long long i = r * C4 + c4;
            const float4 v = dw_fwd_point(x, w, bias, Hin, Win, C4, ks, taps, stride, pad, Hout, Wout, i);
            y[i] = v;
            const double v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
            a0.x += v0; a0.y += v1; a0.z += v2; a0.w += v3;
            a1.x += v0 * v0; a1.y += v1 * v1; a1.z += v2 * v2; a1.w += v3 * v3;
        }
    }
    // lanes col, col + slab, ... of a wave hold the same quad (slab divides 64): fold them into lane col, then the four waves through LDS
    for (int d = slab; d < 64; d <<= 1) {
        a0.x += __shfl_xor(a0.x, d, 64); a0.y += __shfl_xor(a0.y, d, 64); a0.z += __shfl_xor(a0.z, d, 64); a0.w += __shfl_xor(a0.w, d, 64);
        a1.x += __shfl_xor(a1.x, d, 64); a1.y += __shfl_xor(a1.y, d, 64); a1.z += __shfl_xor(a1.z, d, 64); a1.w += __shfl_xor(a1.w, d, 64);
    }
    s_part[(0 * 4 + wave) * 64 + lane] = a0;
    s_part[(1 * 4 + wave) * 64 + lane] = a1;
    __syncthreads();
    if (wave < 2 && lane < slab && my_slab * slab + lane < C4) {   // wave 0 folds the sums, wave 1 the sums of squares (lane < slab: col == lane)
        bn_acc4<double> t = s_part[(wave * 4 + 0) * 64 + lane];
        for (int k = 1; k < 4; ++k) { const bn_acc4<double> u = s_part[(wave * 4 + k) * 64 + lane]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        double* dst = sums + (size_t)wave * C + (size_t)(my_slab * slab + lane) * 4;
        atomicAdd(dst + 0, t.x); atomicAdd(dst + 1, t.y); atomicAdd(dst + 2, t.z); atomicAdd(dst + 3, t.w);
    }
}

// Inference: the stencil with the evaluation-mode BatchNorm (+ ReLU) in its epilogue -- one launch instead of three, the same bits as
// dw_fwd_kernel followed by bn_apply_kernel's evaluation branch (dw_fwd_point, bn_eval_consts and bn_affine4 are shared with them).  The grid
// is apply_blocks': a thread keeps its channel quad over its trips and derives the four reciprocal square roots once.
__global__ void __launch_bounds__(256) dw_norm_fwd_kernel(const float4* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int B,
                                                          int Hin, int Win, int C4, int ks, int stride, int pad, int Hout, int Wout,
                                                          const float4* __restrict__ gamma, const float4* __restrict__ beta,
                                                          const float* __restrict__ running_mean, const float* __restrict__ running_var, float eps,
                                                          int relu, float4* __restrict__ y) {
    const long long total = (long long)B * Hout * Wout * C4;
    const int taps = ks * ks;
    const long long step = (long long)gridDim.x * blockDim.x;
    const bool fixed_c = step % C4 == 0;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f), rs = m, ga = m, be = m;
    const long long i0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (fixed_c && i0 < total) bn_eval_consts(running_mean, running_var, gamma, beta, eps, (int)(i0 % C4), m, rs, ga, be);
    for (long long i = i0; i < total; i += step) {
        if (!fixed_c) bn_eval_consts(running_mean, running_var, gamma, beta, eps, (int)(i % C4), m, rs, ga, be);
        y[i] = bn_affine4(dw_fwd_point(x, w, bias, Hin, Win, C4, ks, taps, stride, pad, Hout, Wout, i), m, rs, ga, be, relu);
    }
}

// dx[b,iy,ix,c] = sum over taps with (iy + pad - ky) % stride == 0 ... of w[c][tap] * dy[b,(iy+pad-ky)/stride,(ix+pad-kx)/stride,c]
// (one input element, added to `acc`: shared by the single-level and the grouped kernels)
__device__ __forceinline__ float4 dw_dgrad_point(const float4* dy, const float* w, int Hin, int Win, int C4, int ks, int taps,
                                                 int stride, int pad, int Hout, int Wout, long long i, float4 acc) {
    const int c4 = (int)(i % C4);
    long long p = i / C4;
    const int ix = (int)(p % Win); p /= Win;
    const int iy = (int)(p % Hin);
    const int b = (int)(p / Hin);
    const float* wc = w + (long long)c4 * 4 * taps;
    for (int ky = 0; ky < ks; ++ky) {
        const int ty = iy + pad - ky;
        if (ty < 0 || ty % stride || ty / stride >= Hout) continue;
        for (int kx = 0; kx < ks; ++kx) {
            const int tx = ix + pad - kx;
            if (tx < 0 || tx % stride || tx / stride >= Wout) continue;
            const float4 v = dy[((long long)(b * Hout + ty / stride) * Wout + tx / stride) * C4 + c4];
            const int t = ky * ks + kx;
            acc.x = fmaf(wc[t], v.x, acc.x);
            acc.y = fmaf(wc[taps + t], v.y, acc.y);
            acc.z = fmaf(wc[2 * taps + t], v.z, acc.z);
            acc.w = fmaf(wc[3 * taps + t], v.w, acc.w);
        }
    }
    return acc;
}

__global__ void __launch_bounds__(256) dw_dgrad_kernel(const float4* __restrict__ dy, const float* __restrict__ w, int B, int Hin, int Win, int C4, int ks,
                                                       int stride, int pad, int Hout, int Wout, float4* __restrict__ dx, int accumulate) {
    const long long total = (long long)B * Hin * Win * C4;
    const int taps = ks * ks;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        dx[i] = dw_dgrad_point(dy, w, Hin, Win, C4, ks, taps, stride, pad, Hout, Wout, i, accumulate ? dx[i] : make_float4(0.f, 0.f, 0.f, 0.f));
}

// grid (C4 blocks of 64 channel-quads, pixel chunks): thread (cq, ps) = channel quad cq of the block, pixel phase ps of 4
__global__ void __launch_bounds__(256) dw_wgrad_kernel(const float4* __restrict__ x, const float4* __restrict__ dy, int B, int Hin, int Win, int C4, int ks,
                                                       int stride, int pad, int Hout, int Wout, int pixels_per_block, float* __restrict__ dw,
                                                       float* __restrict__ db) {
    __shared__ float s_red[4][64][4];
    const int taps = ks * ks;
    const int cq = threadIdx.x & 63, ps = threadIdx.x >> 6;
    const int c4 = blockIdx.x * 64 + cq;
    const long long M = (long long)B * Hout * Wout;
    const long long p0 = (long long)blockIdx.y * pixels_per_block, p1 = p0 + pixels_per_block < M ? p0 + pixels_per_block : M;
    float4 acc[kDwMaxTaps];
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < kDwMaxTaps; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < C4) {
        for (long long p = p0 + ps; p < p1; p += 4) {
            const int xo = (int)(p % Wout);
            const int yo = (int)((p / Wout) % Hout);
            const int b = (int)(p / ((long long)Wout * Hout));
            const float4 g = dy[p * C4 + c4];
            bsum.x += g.x; bsum.y += g.y; bsum.z += g.z; bsum.w += g.w;
#pragma unroll
            for (int t = 0; t < kDwMaxTaps; ++t) {
                if (t >= taps) break;
                const int iy = yo * stride - pad + t / ks, ix = xo * stride - pad + t % ks;
                if (iy < 0 || iy >= Hin || ix < 0 || ix >= Win) continue;
                const float4 v = x[((long long)(b * Hin + iy) * Win + ix) * C4 + c4];
                acc[t].x = fmaf(g.x, v.x, acc[t].x);
                acc[t].y = fmaf(g.y, v.y, acc[t].y);
                acc[t].z = fmaf(g.z, v.z, acc[t].z);
                acc[t].w = fmaf(g.w, v.w, acc[t].w);
            }
        }
    }
    // reduce the 4 pixel phases through LDS, one tap at a time; phase 0 adds the block's partial
    for (int t = -1; t < taps; ++t) {
        const float4 v = t < 0 ? bsum : acc[t < 0 ? 0 : t];
        __syncthreads();
        s_red[ps][cq][0] = v.x; s_red[ps][cq][1] = v.y; s_red[ps][cq][2] = v.z; s_red[ps][cq][3] = v.w;
        __syncthreads();
        if (ps == 0 && c4 < C4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float sum = s_red[0][cq][e] + s_red[1][cq][e] + s_red[2][cq][e] + s_red[3][cq][e];
                if (t < 0) { if (db) atomicAdd(db + c4 * 4 + e, sum); }
                else atomicAdd(dw + (long long)(c4 * 4 + e) * taps + t, sum);
            }
        }
    }
}

__global__ void zero_small_kernel(float* a, long long na, float* b, long long nb) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += (long long)gridDim.x * blockDim.x) {
        if (i < na) a[i] = 0.0f;
        else b[i - na] = 0.0f;
    }
}

// ---- the same stencil over up to 8 levels that share batch, channels and weight (the RetinaNet tower, predictors.py:33-35,67-68) ----
// The levels' maps are packed by value into the kernel argument (as CatPieces is): no pointer table on the device.  end[l] is the
// prefix sum of the levels' work items (float4 elements for the forward / data gradient, output pixels for the weight gradient).
constexpr int kDwMaxLevels = 8;
struct DwLevels {
    const float4* src[kDwMaxLevels];   // forward: x; data gradient: dy; weight gradient: x
    float4* dst[kDwMaxLevels];         // forward: y; data gradient: dx; weight gradient: dy (read only)
    int hin[kDwMaxLevels], win[kDwMaxLevels], hout[kDwMaxLevels], wout[kDwMaxLevels];
    long long end[kDwMaxLevels];
    int n;
};
__device__ __forceinline__ int dw_level(const DwLevels& lv, long long i) {
    int l = 0;
    while (l + 1 < lv.n && i >= lv.end[l]) ++l;
    return l;
}

__global__ void __launch_bounds__(256) dw_group_fwd_kernel(DwLevels lv, const float* __restrict__ w, const float* __restrict__ bias, int C4, int ks, int stride,
                                                           int pad) {
    const long long total = lv.end[lv.n - 1];
    const int taps = ks * ks;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int l = dw_level(lv, i);
        const long long j = i - (l ? lv.end[l - 1] : 0LL);
        lv.dst[l][j] = dw_fwd_point(lv.src[l], w, bias, lv.hin[l], lv.win[l], C4, ks, taps, stride, pad, lv.hout[l], lv.wout[l], j);
    }
}

__global__ void __launch_bounds__(256) dw_group_dgrad_kernel(DwLevels lv, const float* __restrict__ w, int C4, int ks, int stride, int pad) {
    const long long total = lv.end[lv.n - 1];
    const int taps = ks * ks;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int l = dw_level(lv, i);
        const long long j = i - (l ? lv.end[l - 1] : 0LL);
        lv.dst[l][j] = dw_dgrad_point(lv.src[l], w, lv.hin[l], lv.win[l], C4, ks, taps, stride, pad, lv.hout[l], lv.wout[l], j, make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

// Weight / bias gradient, stage 1.  grid (C4 blocks of QUADS channel quads, chunks of the concatenated output pixels); thread (cq, ps) =
// channel quad cq of the block, pixel phase ps of PHASES = 256 / QUADS.  A thread walks its pixels in ascending order (level after
// level), the workgroup adds its phases in ascending order through LDS and stores ONE partial per (chunk, tap, channel) -- row `taps`
// is the bias column -- at part[(chunk * (taps + 1) + tap) * C + c].  No atomics: the bits depend on the shapes alone.
// The kernel size is a template argument: every index of acc is then a constant and the k * k accumulators stay in registers.
template <int QUADS, int KS>
__global__ void __launch_bounds__(256) dw_group_wgrad_kernel(DwLevels lv, int C4, int stride, int pad, int pixels_per_block, float* __restrict__ part) {
    constexpr int PHASES = 256 / QUADS, taps = KS * KS;
    __shared__ __attribute__((aligned(16))) float s_red[2][PHASES][QUADS * 4];
    const int cq = threadIdx.x % QUADS, ps = threadIdx.x / QUADS;
    const int c4 = blockIdx.x * QUADS + cq;
    const long long M = lv.end[lv.n - 1];
    const long long p0 = (long long)blockIdx.y * pixels_per_block, p1 = p0 + pixels_per_block < M ? p0 + pixels_per_block : M;
    float4 acc[taps];
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < taps; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < C4 && p0 + ps < p1) {
        int l = dw_level(lv, p0 + ps);
        long long base = l ? lv.end[l - 1] : 0LL, end = lv.end[l];
        const float4* x = lv.src[l];
        const float4* dy = lv.dst[l];
        int Hin = lv.hin[l], Win = lv.win[l], Hout = lv.hout[l], Wout = lv.wout[l];
        for (long long p = p0 + ps; p < p1; p += PHASES) {
            while (p >= end) {   // (p < p1 <= M = end[n - 1]: l stays below n)
                ++l;
                base = end; end = lv.end[l];
                x = lv.src[l]; dy = lv.dst[l];
                Hin = lv.hin[l]; Win = lv.win[l]; Hout = lv.hout[l]; Wout = lv.wout[l];
            }
            const long long q = p - base;
            const int xo = (int)(q % Wout);
            const int yo = (int)((q / Wout) % Hout);
            const int b = (int)(q / ((long long)Wout * Hout));
            const float4 g = dy[q * C4 + c4];
            bsum.x += g.x; bsum.y += g.y; bsum.z += g.z; bsum.w += g.w;
#pragma unroll
            for (int t = 0; t < taps; ++t) {
                const int iy = yo * stride - pad + t / KS, ix = xo * stride - pad + t % KS;
                if (iy >= 0 && iy < Hin && ix >= 0 && ix < Win) {
                    const float4 v = x[((long long)(b * Hin + iy) * Win + ix) * C4 + c4];
                    acc[t].x = fmaf(g.x, v.x, acc[t].x);
                    acc[t].y = fmaf(g.y, v.y, acc[t].y);
                    acc[t].z = fmaf(g.z, v.z, acc[t].z);
                    acc[t].w = fmaf(g.w, v.w, acc[t].w);
                }
            }
        }
    }
    // one tap per round, two LDS buffers in turn (a round's reads end before the barrier of the next round, which precedes the writes of
    // the round after that): thread j < QUADS * 4 owns channel blockIdx.x * QUADS * 4 + j and adds the phases in ascending order
    const int C = C4 * 4, c = blockIdx.x * QUADS * 4 + (int)threadIdx.x;
    float* out = part + (long long)blockIdx.y * (taps + 1) * C;
#pragma unroll
    for (int t = 0; t <= taps; ++t) {
        *reinterpret_cast<float4*>(&s_red[t & 1][ps][cq * 4]) = t == taps ? bsum : acc[t < taps ? t : 0];
        __syncthreads();
        if (threadIdx.x < QUADS * 4 && c < C) {
            float sum = s_red[t & 1][0][threadIdx.x];
#pragma unroll
            for (int k = 1; k < PHASES; ++k) sum += s_red[t & 1][k][threadIdx.x];
            out[(long long)t * C + c] = sum;
        }
    }
}

// stage 2: thread (tap, channel) adds the chunks in ascending order; row `taps` of the partials is db
__global__ void __launch_bounds__(256) dw_group_wgrad_finish_kernel(const float* __restrict__ part, int chunks, int C, int taps, float* __restrict__ dw,
                                                                    float* __restrict__ db) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (taps + 1) * C) return;
    const int t = i / C, c = i - t * C;
    if ((t == taps && !db) || (t < taps && !dw)) return;
    float sum = part[i];
    for (int k = 1; k < chunks; ++k) sum += part[(long long)k * (taps + 1) * C + i];
    if (t == taps) db[c] = sum;
    else dw[(long long)c * taps + t] = sum;
}

}  // namespace ssdk

static int dw_check(const char* fn, int batch, int hin, int win, int channels, int ksize, int stride, int pad) {
    SSDK_REQUIRE(batch > 0 && hin > 0 && win > 0 && channels > 0 && channels % 4 == 0 && ksize >= 1 && ksize * ksize <= ssdk::kDwMaxTaps && stride >= 1 && pad >= 0 &&
                     hin + 2 * pad >= ksize && win + 2 * pad >= ksize,
                 SSDK_E_INVALID, "%s: batch=%d H=%d W=%d C=%d (%%4) k=%d stride=%d pad=%d", fn, batch, hin, win, channels, ksize, stride, pad);
    return SSDK_OK;
}

extern "C" int ssdk_depthwise_conv2d_fwd(const float* x, const float* w, const float* bias, int batch, int hin, int win, int channels, int ksize,
                                         int stride, int pad, float* y, void* stream) {
    int rc = dw_check("ssdk_depthwise_conv2d_fwd", batch, hin, win, channels, ksize, stride, pad);
    if (rc) return rc;
    SSDK_REQUIRE(x && w && y && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)bias) & 15) == 0, SSDK_E_INVALID, "ssdk_depthwise_conv2d_fwd: null or unaligned pointer");
    const int ho = (hin + 2 * pad - ksize) / stride + 1, wo = (win + 2 * pad - ksize) / stride + 1;
    const long long total = (long long)batch * ho * wo * (channels / 4);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
    hipLaunchKernelGGL(ssdk::dw_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x), w, bias, batch, hin, win,
                       channels / 4, ksize, stride, pad, ho, wo, reinterpret_cast<float4*>(y));
    SSDK_CHECK_LAUNCH("dw_fwd_kernel");
    return SSDK_OK;
}

// the forward of a training-mode depthwise Conv2dBn block: y as ssdk_depthwise_conv2d_fwd's, and sums += the statistics of y (no zero-fill:
// ssdk_batchnorm_stats_accumulate's contract), sums[2C] = the row count
extern "C" int ssdk_depthwise_conv2d_stats_fwd(const float* x, const float* w, const float* bias, int batch, int hin, int win, int channels, int ksize,
                                               int stride, int pad, float* y, double* sums, void* stream) {
    const char* fn = "ssdk_depthwise_conv2d_stats_fwd";
    int rc = dw_check(fn, batch, hin, win, channels, ksize, stride, pad);
    if (rc) return rc;
    SSDK_REQUIRE(x && w && y && sums && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)bias) & 15) == 0 && ((uintptr_t)sums & 7) == 0, SSDK_E_INVALID,
                 "%s: null or unaligned pointer (y and sums are required)", fn);
    const int ho = (hin + 2 * pad - ksize) / stride + 1, wo = (win + 2 * pad - ksize) / stride + 1, c4 = channels / 4;
    const long long rows = (long long)batch * ho * wo;
    const ssdk::DwStatsPlan p = ssdk::dw_stats_plan(rows, c4);
    SSDK_REQUIRE(p.row_blocks * p.slabs < (1ll << 31), SSDK_E_INVALID, "%s: %lld row blocks x %d slabs exceed the grid", fn, p.row_blocks, p.slabs);
    hipLaunchKernelGGL(ssdk::dw_stats_fwd_kernel, dim3((unsigned)(p.row_blocks * p.slabs)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x),
                       w, bias, batch, hin, win, c4, ksize, stride, pad, ho, wo, p.rows_per_block, p.slab, p.slabs, reinterpret_cast<float4*>(y), sums);
    SSDK_CHECK_LAUNCH("dw_stats_fwd_kernel");
    return SSDK_OK;
}

// the forward of an evaluation-mode depthwise Conv2dBn block in one launch: ssdk_depthwise_conv2d_fwd, then ssdk_batchnorm_fwd(training = 0)
extern "C" int ssdk_depthwise_conv2d_norm_fwd(const float* x, const float* w, const float* bias, int batch, int hin, int win, int channels, int ksize,
                                              int stride, int pad, const float* gamma, const float* beta, const float* running_mean,
                                              const float* running_var, float eps, int relu, float* y, void* stream) {
    const char* fn = "ssdk_depthwise_conv2d_norm_fwd";
    int rc = dw_check(fn, batch, hin, win, channels, ksize, stride, pad);
    if (rc) return rc;
    SSDK_REQUIRE(x && w && y && running_mean && running_var, SSDK_E_INVALID, "%s: null pointer (y and the running statistics are required)", fn);
    SSDK_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)running_mean | (uintptr_t)running_var) & 15) == 0,
                 SSDK_E_INVALID, "%s: unaligned pointer (16 bytes: maps, bias, gamma, beta, running statistics)", fn);
    const int ho = (hin + 2 * pad - ksize) / stride + 1, wo = (win + 2 * pad - ksize) / stride + 1, c4 = channels / 4;
    const long long total = (long long)batch * ho * wo * c4;
    hipLaunchKernelGGL(ssdk::dw_norm_fwd_kernel, dim3(ssdk::apply_blocks(total, c4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x), w, bias,
                       batch, hin, win, c4, ksize, stride, pad, ho, wo, reinterpret_cast<const float4*>(gamma), reinterpret_cast<const float4*>(beta),
                       running_mean, running_var, eps, relu, reinterpret_cast<float4*>(y));
    SSDK_CHECK_LAUNCH("dw_norm_fwd_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_depthwise_conv2d_bwd(const float* x, const float* w, const float* dy, int batch, int hin, int win, int channels, int ksize,
                                         int stride, int pad, float* dx, float* dw, float* db, int accumulate, void* stream) {
    int rc = dw_check("ssdk_depthwise_conv2d_bwd", batch, hin, win, channels, ksize, stride, pad);
    if (rc) return rc;
    SSDK_REQUIRE(x && w && dy && (dx || dw) && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0, SSDK_E_INVALID,
                 "ssdk_depthwise_conv2d_bwd: null or unaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const int ho = (hin + 2 * pad - ksize) / stride + 1, wo = (win + 2 * pad - ksize) / stride + 1, c4 = channels / 4;
    if (dx) {
        const long long total = (long long)batch * hin * win * c4;
        const unsigned blocks = (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
        hipLaunchKernelGGL(ssdk::dw_dgrad_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(dy), w, batch, hin, win, c4, ksize, stride, pad, ho,
                           wo, reinterpret_cast<float4*>(dx), accumulate);
        SSDK_CHECK_LAUNCH("dw_dgrad_kernel");
    }
    if (dw) {
        if (!accumulate) {
            hipLaunchKernelGGL(ssdk::zero_small_kernel, dim3(8), dim3(256), 0, s, dw, (long long)channels * ksize * ksize, db, db ? (long long)channels : 0LL);
            SSDK_CHECK_LAUNCH("zero_small_kernel");
        }
        const long long M = (long long)batch * ho * wo;
        int chunks = (int)((M + 255) / 256);   // >= 256 pixels per block ...
        if (chunks > 512) chunks = 512;         // ... and at most 512 partials per (channel, tap)
        if (ssdk::deterministic()) chunks = 1;  // (one workgroup per 64 channel quads walks all pixels: its single "atomic" per element adds to zero)
        const int ppb = (int)((M + chunks - 1) / chunks);
        hipLaunchKernelGGL(ssdk::dw_wgrad_kernel, dim3((unsigned)((c4 + 63) / 64), (unsigned)chunks), dim3(256), 0, s, reinterpret_cast<const float4*>(x),
                           reinterpret_cast<const float4*>(dy), batch, hin, win, c4, ksize, stride, pad, ho, wo, ppb, dw, db);
        SSDK_CHECK_LAUNCH("dw_wgrad_kernel");
    }
    return SSDK_OK;
}

// ---- grouped depthwise convolution over levels ----
struct DwGroupPlan {
    int ho[ssdk::kDwMaxLevels], wo[ssdk::kDwMaxLevels];
    long long pixels;   // output pixels of all levels
    int chunks, ppb;    // stage 1 of the weight gradient: chunks of ppb consecutive pixels (a function of the shapes only)
};
static int dw_group_check(const char* fn, const int* hs, const int* ws, int n_levels, int batch, int channels, int ksize, int stride, int pad, DwGroupPlan& plan) {
    SSDK_REQUIRE(n_levels >= 1 && n_levels <= ssdk::kDwMaxLevels && hs && ws, SSDK_E_INVALID, "%s: n_levels=%d (1..%d), hs / ws %s", fn, n_levels,
                 ssdk::kDwMaxLevels, hs && ws ? "given" : "null");
    plan.pixels = 0;
    for (int l = 0; l < n_levels; ++l) {
        char who[96];
        snprintf(who, sizeof(who), "%s: level %d", fn, l);
        int rc = dw_check(who, batch, hs[l], ws[l], channels, ksize, stride, pad);
        if (rc) return rc;
        plan.ho[l] = (hs[l] + 2 * pad - ksize) / stride + 1;
        plan.wo[l] = (ws[l] + 2 * pad - ksize) / stride + 1;
        SSDK_REQUIRE((long long)batch * hs[l] * ws[l] < (1LL << 31) / 4, SSDK_E_INVALID, "%s: level %d: batch * H * W = %lld is beyond the kernels' int row index", fn, l,
                     (long long)batch * hs[l] * ws[l]);
        plan.pixels += (long long)batch * plan.ho[l] * plan.wo[l];
    }
    long long chunks = plan.pixels / 256;   // >= 256 pixels per chunk ...
    if (chunks < 1) chunks = 1;
    if (chunks > 512) chunks = 512;         // ... and at most 512 partials per (channel, tap)
    const long long ppb = (plan.pixels + chunks - 1) / chunks;
    SSDK_REQUIRE(ppb < (1LL << 31), SSDK_E_INVALID, "%s: %lld output pixels are beyond the chunked reduction", fn, plan.pixels);
    plan.ppb = (int)ppb;
    plan.chunks = (int)((plan.pixels + ppb - 1) / ppb);
    return SSDK_OK;
}
static inline unsigned dw_group_blocks(long long total) { return (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535); }

extern "C" long long ssdk_depthwise_conv2d_group_workspace_bytes(const int* hs, const int* ws, int n_levels, int batch, int channels, int ksize, int stride,
                                                                 int pad) {
    DwGroupPlan plan;
    int rc = dw_group_check("ssdk_depthwise_conv2d_group_workspace_bytes", hs, ws, n_levels, batch, channels, ksize, stride, pad, plan);
    if (rc) return rc;
    return (long long)plan.chunks * (ksize * ksize + 1) * channels * (long long)sizeof(float);
}

extern "C" int ssdk_depthwise_conv2d_group_fwd(const float* const* xs, const int* hs, const int* ws, int n_levels, const float* w, const float* bias, int batch,
                                               int channels, int ksize, int stride, int pad, float* const* ys, void* stream) {
    const char* fn = "ssdk_depthwise_conv2d_group_fwd";
    DwGroupPlan plan;
    int rc = dw_group_check(fn, hs, ws, n_levels, batch, channels, ksize, stride, pad, plan);
    if (rc) return rc;
    SSDK_REQUIRE(xs && ys && w && (((uintptr_t)w | (uintptr_t)bias) & 15) == 0, SSDK_E_INVALID, "%s: null xs / ys / w, or unaligned w / bias", fn);
    ssdk::DwLevels lv = {};
    const int c4 = channels / 4;
    long long total = 0;
    for (int l = 0; l < n_levels; ++l) {
        SSDK_REQUIRE(xs[l] && ys[l] && (((uintptr_t)xs[l] | (uintptr_t)ys[l]) & 15) == 0, SSDK_E_INVALID, "%s: level %d: null or unaligned x / y", fn, l);
        lv.src[l] = reinterpret_cast<const float4*>(xs[l]);
        lv.dst[l] = reinterpret_cast<float4*>(ys[l]);
        lv.hin[l] = hs[l]; lv.win[l] = ws[l]; lv.hout[l] = plan.ho[l]; lv.wout[l] = plan.wo[l];
        total += (long long)batch * plan.ho[l] * plan.wo[l] * c4;
        lv.end[l] = total;
    }
    lv.n = n_levels;
    hipLaunchKernelGGL(ssdk::dw_group_fwd_kernel, dim3(dw_group_blocks(total)), dim3(256), 0, (hipStream_t)stream, lv, w, bias, c4, ksize, stride, pad);
    SSDK_CHECK_LAUNCH("dw_group_fwd_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_depthwise_conv2d_group_bwd(const float* const* xs, const int* hs, const int* ws, int n_levels, const float* w, const float* const* dys, int batch,
                                               int channels, int ksize, int stride, int pad, float* const* dxs, float* dw, float* db, void* workspace,
                                               long long workspace_bytes, void* stream) {
    const char* fn = "ssdk_depthwise_conv2d_group_bwd";
    DwGroupPlan plan;
    int rc = dw_group_check(fn, hs, ws, n_levels, batch, channels, ksize, stride, pad, plan);
    if (rc) return rc;
    SSDK_REQUIRE(xs && dys && w && (((uintptr_t)w | (uintptr_t)dw | (uintptr_t)db) & 3) == 0, SSDK_E_INVALID, "%s: null xs / dys / w, or unaligned w / dw / db", fn);
    const int c4 = channels / 4, taps = ksize * ksize;
    const long long need = (long long)plan.chunks * (taps + 1) * channels * (long long)sizeof(float);
    const bool wgrad = dw || db;
    SSDK_REQUIRE(!wgrad || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0), SSDK_E_INVALID,
                 "%s: workspace of %lld bytes (%s), ssdk_depthwise_conv2d_group_workspace_bytes says %lld", fn, workspace_bytes,
                 workspace ? "given" : "null", need);
    ssdk::DwLevels dg = {}, wg = {};
    long long dg_total = 0, wg_total = 0;
    for (int l = 0; l < n_levels; ++l) {
        SSDK_REQUIRE(xs[l] && dys[l] && (((uintptr_t)xs[l] | (uintptr_t)dys[l] | (uintptr_t)(dxs ? dxs[l] : nullptr)) & 15) == 0, SSDK_E_INVALID,
                     "%s: level %d: null or unaligned x / dy / dx", fn, l);
        wg.src[l] = reinterpret_cast<const float4*>(xs[l]);
        wg.dst[l] = const_cast<float4*>(reinterpret_cast<const float4*>(dys[l]));   // (read only in the weight gradient)
        wg.hin[l] = hs[l]; wg.win[l] = ws[l]; wg.hout[l] = plan.ho[l]; wg.wout[l] = plan.wo[l];
        wg_total += (long long)batch * plan.ho[l] * plan.wo[l];
        wg.end[l] = wg_total;
        if (dxs && dxs[l]) {   // the data gradient runs over the levels that ask for one
            const int k = dg.n++;
            dg.src[k] = reinterpret_cast<const float4*>(dys[l]);
            dg.dst[k] = reinterpret_cast<float4*>(dxs[l]);
            dg.hin[k] = hs[l]; dg.win[k] = ws[l]; dg.hout[k] = plan.ho[l]; dg.wout[k] = plan.wo[l];
            dg_total += (long long)batch * hs[l] * ws[l] * c4;
            dg.end[k] = dg_total;
        }
    }
    wg.n = n_levels;
    hipStream_t s = (hipStream_t)stream;
    if (dg.n) {
        hipLaunchKernelGGL(ssdk::dw_group_dgrad_kernel, dim3(dw_group_blocks(dg_total)), dim3(256), 0, s, dg, w, c4, ksize, stride, pad);
        SSDK_CHECK_LAUNCH("dw_group_dgrad_kernel");
    }
    if (wgrad) {
        float* part = reinterpret_cast<float*>(workspace);
        // the workgroup's split of its 256 threads: full at C4 = 16 (64 channels) and 32 (128 channels), dw_wgrad_kernel's from there on
        const int quads = c4 <= 16 ? 16 : c4 <= 32 ? 32 : 64;
        const dim3 grid((unsigned)((c4 + quads - 1) / quads), (unsigned)plan.chunks);
        void (*kernel)(ssdk::DwLevels, int, int, int, int, float*) = nullptr;
#define SSDK_DW_GROUP_WGRAD(K) \
    case K: kernel = quads == 16 ? ssdk::dw_group_wgrad_kernel<16, K> : quads == 32 ? ssdk::dw_group_wgrad_kernel<32, K> : ssdk::dw_group_wgrad_kernel<64, K>; break;
        switch (ksize) {
            SSDK_DW_GROUP_WGRAD(1) SSDK_DW_GROUP_WGRAD(2) SSDK_DW_GROUP_WGRAD(3) SSDK_DW_GROUP_WGRAD(4) SSDK_DW_GROUP_WGRAD(5)
        }
#undef SSDK_DW_GROUP_WGRAD
        SSDK_REQUIRE(kernel, SSDK_E_INVALID, "%s: k=%d", fn, ksize);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, wg, c4, stride, pad, plan.ppb, part);
        SSDK_CHECK_LAUNCH("dw_group_wgrad_kernel");
        const int n = (taps + 1) * channels;
        hipLaunchKernelGGL(ssdk::dw_group_wgrad_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, plan.chunks, channels, taps, dw, db);
        SSDK_CHECK_LAUNCH("dw_group_wgrad_finish_kernel");
    }
    return SSDK_OK;
}

// ---- depthwise feature pyramid (Tiny-DSOD D-FPN, bf/modules/features.py:123-212) -------------------------------------------
// The three ops of the D-FPN neck that the kernels above do not cover: the zero-padded 2x2 max-pool of the downsample path's first
// branch (:188-195), the channel concatenation of the two branches (:198), and the up path's depthwise 3x3 convolution of a
// nearest-upsampled map (:203-205; the upsampled map is never built).  NHWC fp32, a thread owns 4 consecutive channels (float4).
// Every reduction below except the weight gradient is a gather (no atomics); the weight gradient follows dw_wgrad_kernel.
namespace ssdk {

// The 2x2 window (yo, xo) of the zero-padded map: rows 2yo, 2yo+1 and columns 2xo, 2xo+1; a row >= H or a column >= W is the pad
// and reads 0.0 (features.py:188-192 pads with F.pad's zeros, a real value that takes part in the max).
__device__ __forceinline__ void mp_window(const float4* __restrict__ x, int b, int yo, int xo, int H, int W, int C4, int c4, float4 (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = 2 * yo + (k >> 1), xx = 2 * xo + (k & 1);
        v[k] = (y < H && xx < W) ? x[(((long long)b * H + y) * W + xx) * C4 + c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// torch's CPU max-pool rule over the window order (0,0), (0,1), (1,0), (1,1): `val > max || isnan(val)` -- the first maximum wins a tie,
// a NaN wins.  Returns the window position of the maximum.
__device__ __forceinline__ int mp_arg(float a0, float a1, float a2, float a3, float& m) {
    int k = 0;
    m = a0;
    if (a1 > m || a1 != a1) { m = a1; k = 1; }
    if (a2 > m || a2 != a2) { m = a2; k = 2; }
    if (a3 > m || a3 != a3) { m = a3; k = 3; }
    return k;
}

__global__ void __launch_bounds__(256) maxpool2x2_kernel(const float4* __restrict__ x, int B, int H, int W, int C4, int Ho, int Wo,
                                                         float4* __restrict__ y) {
    const long long total = (long long)B * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long long p = i / C4;
        const int xo = (int)(p % Wo); p /= Wo;
        const int yo = (int)(p % Ho);
        const int b = (int)(p / Ho);
        float4 v[4], m;
        mp_window(x, b, yo, xo, H, W, C4, c4, v);
        mp_arg(v[0].x, v[1].x, v[2].x, v[3].x, m.x);
        mp_arg(v[0].y, v[1].y, v[2].y, v[3].y, m.y);
        mp_arg(v[0].z, v[1].z, v[2].z, v[3].z, m.z);
        mp_arg(v[0].w, v[1].w, v[2].w, v[3].w, m.w);
        y[i] = m;
    }
}

// Gather form of the backward: the windows do not overlap, so the thread of window (yo, xo) writes every input cell of it -- dy where the
// cell is the window's maximum (recomputed from x, no stored indices), 0 elsewhere; a maximum that sits in the pad drops its gradient.
// The last window row / column also writes the input rows / columns no window covers (odd H or W without a pad): zeros.
__global__ void __launch_bounds__(256) maxpool2x2_bwd_kernel(const float4* __restrict__ x, const float4* __restrict__ dy, int B, int H, int W,
                                                             int C4, int Ho, int Wo, float4* __restrict__ dx) {
    const long long total = (long long)B * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long long p = i / C4;
        const int xo = (int)(p % Wo); p /= Wo;
        const int yo = (int)(p % Ho);
        const int b = (int)(p / Ho);
        float4 v[4];
        float m;
        mp_window(x, b, yo, xo, H, W, C4, c4, v);
        const int kx = mp_arg(v[0].x, v[1].x, v[2].x, v[3].x, m), ky = mp_arg(v[0].y, v[1].y, v[2].y, v[3].y, m);
        const int kz = mp_arg(v[0].z, v[1].z, v[2].z, v[3].z, m), kw = mp_arg(v[0].w, v[1].w, v[2].w, v[3].w, m);
        const float4 g = dy[i];
        const int y1 = yo == Ho - 1 ? H : 2 * yo + 2, x1 = xo == Wo - 1 ? W : 2 * xo + 2;
        for (int yy = 2 * yo; yy < y1; ++yy) {
            for (int xx = 2 * xo; xx < x1; ++xx) {
                const int k = (yy - 2 * yo < 2 && xx - 2 * xo < 2) ? (yy - 2 * yo) * 2 + (xx - 2 * xo) : -1;
                dx[(((long long)b * H + yy) * W + xx) * C4 + c4] = make_float4(k == kx ? g.x : 0.f, k == ky ? g.y : 0.f, k == kz ? g.z : 0.f,
                                                                                k == kw ? g.w : 0.f);
            }
        }
    }
}

// torch.cat(pieces, dim=1) of NHWC maps with `rows` pixels each, and its split (the gradient of every piece as its own contiguous map).
struct CatPieces {
    float4* p[kMaxPieces];
    int c4[kMaxPieces];         // float4 columns of piece k
    int off4[kMaxPieces + 1];   // its first column in the concatenated row; off4[n] = the row length
    int n;
};
__device__ __forceinline__ int cat_piece(const CatPieces& ps, int c) {
    int k = 0;
    while (k + 1 < ps.n && c >= ps.off4[k + 1]) ++k;
    return k;
}
__global__ void __launch_bounds__(256) concat_kernel(CatPieces ps, long long rows, float4* __restrict__ out) {
    const int C4 = ps.off4[ps.n];
    const long long total = rows * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / C4;
        const int c = (int)(i - row * C4);
        const int k = cat_piece(ps, c);
        out[i] = ps.p[k][row * ps.c4[k] + (c - ps.off4[k])];
    }
}
__global__ void __launch_bounds__(256) split_kernel(const float4* __restrict__ dout, long long rows, CatPieces ds) {
    const int C4 = ds.off4[ds.n];
    const long long total = rows * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / C4;
        const int c = (int)(i - row * C4);
        const int k = cat_piece(ds, c);
        ds.p[k][row * ds.c4[k] + (c - ds.off4[k])] = dout[i];
    }
}

// y[b,yo,xo,c] = bias[c] + sum_tap w[c][tap] * up[b, yo - 1 + ky, xo - 1 + kx, c],  up = nearest(coarse -> Hf x Wf), zero outside the map:
// the 3 x 3 depthwise convolution (pad 1, stride 1) of features.py:203-205 reads the coarse map through nearest_src, the index map of
// ssdk_upsample_nearest_add (torch's), so the padding is that of the fine resolution.
constexpr int kDwUpTaps = 9;
__global__ void __launch_bounds__(256) dwup_fwd_kernel(const float4* __restrict__ coarse, const float* __restrict__ w, const float* __restrict__ bias,
                                                       int B, int Hc, int Wc, int Hf, int Wf, int C4, float4* __restrict__ y) {
    const long long total = (long long)B * Hf * Wf * C4;
    const float sh = (float)Hc / (float)Hf, sw = (float)Wc / (float)Wf;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long long p = i / C4;
        const int xo = (int)(p % Wf); p /= Wf;
        const int yo = (int)(p % Hf);
        const int b = (int)(p / Hf);
        float4 acc = bias ? *reinterpret_cast<const float4*>(bias + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float* wc = w + (long long)c4 * 4 * kDwUpTaps;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = yo - 1 + ky;
            if (iy < 0 || iy >= Hf) continue;
            const long long rowc = ((long long)b * Hc + nearest_src(iy, sh, Hc)) * Wc;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = xo - 1 + kx;
                if (ix < 0 || ix >= Wf) continue;
                const float4 v = coarse[(rowc + nearest_src(ix, sw, Wc)) * C4 + c4];
                const int t = ky * 3 + kx;
                acc.x = fmaf(wc[t], v.x, acc.x);
                acc.y = fmaf(wc[kDwUpTaps + t], v.y, acc.y);
                acc.z = fmaf(wc[2 * kDwUpTaps + t], v.z, acc.z);
                acc.w = fmaf(wc[3 * kDwUpTaps + t], v.w, acc.w);
            }
        }
        y[i] = acc;
    }
}

// dcoarse[b,yc,xc,c] = sum over the fine pixels (y, x) whose nearest source is (yc, xc) of sum_tap w[c][tap] * dy[b, y + 1 - ky, x + 1 - kx, c]
// (gather form, the candidate rows / columns of upsample_add_bwd_kernel: deterministic)
__global__ void __launch_bounds__(256) dwup_dgrad_kernel(const float4* __restrict__ dy, const float* __restrict__ w, int B, int Hc, int Wc, int Hf,
                                                         int Wf, int C4, float4* __restrict__ dcoarse) {
    const long long total = (long long)B * Hc * Wc * C4;
    const float sh = (float)Hc / (float)Hf, sw = (float)Wc / (float)Wf;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long long p = i / C4;
        const int xc = (int)(p % Wc); p /= Wc;
        const int yc = (int)(p % Hc);
        const int b = (int)(p / Hc);
        const int y0 = max(0, (int)floorf((float)yc / sh) - 2), y1 = min(Hf - 1, (int)ceilf((float)(yc + 1) / sh) + 2);
        const int x0 = max(0, (int)floorf((float)xc / sw) - 2), x1 = min(Wf - 1, (int)ceilf((float)(xc + 1) / sw) + 2);
        const float* wc = w + (long long)c4 * 4 * kDwUpTaps;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int yy = y0; yy <= y1; ++yy) {
            if (nearest_src(yy, sh, Hc) != yc) continue;
            for (int xx = x0; xx <= x1; ++xx) {
                if (nearest_src(xx, sw, Wc) != xc) continue;
                for (int ky = 0; ky < 3; ++ky) {
                    const int oy = yy + 1 - ky;
                    if (oy < 0 || oy >= Hf) continue;
                    for (int kx = 0; kx < 3; ++kx) {
                        const int ox = xx + 1 - kx;
                        if (ox < 0 || ox >= Wf) continue;
                        const float4 g = dy[(((long long)b * Hf + oy) * Wf + ox) * C4 + c4];
                        const int t = ky * 3 + kx;
                        s.x = fmaf(wc[t], g.x, s.x);
                        s.y = fmaf(wc[kDwUpTaps + t], g.y, s.y);
                        s.z = fmaf(wc[2 * kDwUpTaps + t], g.z, s.z);
                        s.w = fmaf(wc[3 * kDwUpTaps + t], g.w, s.w);
                    }
                }
            }
        }
        dcoarse[i] = s;
    }
}

// dw[c][tap] = sum over the fine pixels of dy * up (and db[c] = sum dy): dw_wgrad_kernel's layout of the work -- grid (C4 blocks of 64
// channel quads, pixel chunks), 4 pixel phases reduced through LDS, one partial per block and (channel, tap) added with an atomic
// (one chunk in deterministic mode: the single partial adds to zero)
__global__ void __launch_bounds__(256) dwup_wgrad_kernel(const float4* __restrict__ coarse, const float4* __restrict__ dy, int B, int Hc, int Wc, int Hf,
                                                         int Wf, int C4, int pixels_per_block, float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float s_red[4][64][4];
    const int cq = threadIdx.x & 63, ps = threadIdx.x >> 6;
    const int c4 = blockIdx.x * 64 + cq;
    const long long M = (long long)B * Hf * Wf;
    const long long p0 = (long long)blockIdx.y * pixels_per_block, p1 = p0 + pixels_per_block < M ? p0 + pixels_per_block : M;
    const float sh = (float)Hc / (float)Hf, sw = (float)Wc / (float)Wf;
    float4 acc[kDwUpTaps];
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < kDwUpTaps; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < C4) {
        for (long long p = p0 + ps; p < p1; p += 4) {
            const int xo = (int)(p % Wf);
            const int yo = (int)((p / Wf) % Hf);
            const int b = (int)(p / ((long long)Wf * Hf));
            const float4 g = dy[p * C4 + c4];
            bsum.x += g.x; bsum.y += g.y; bsum.z += g.z; bsum.w += g.w;
#pragma unroll
            for (int t = 0; t < kDwUpTaps; ++t) {
                const int iy = yo - 1 + t / 3, ix = xo - 1 + t % 3;
                if (iy < 0 || iy >= Hf || ix < 0 || ix >= Wf) continue;
                const float4 v = coarse[(((long long)b * Hc + nearest_src(iy, sh, Hc)) * Wc + nearest_src(ix, sw, Wc)) * C4 + c4];
                acc[t].x = fmaf(g.x, v.x, acc[t].x);
                acc[t].y = fmaf(g.y, v.y, acc[t].y);
                acc[t].z = fmaf(g.z, v.z, acc[t].z);
                acc[t].w = fmaf(g.w, v.w, acc[t].w);
            }
        }
    }
    for (int t = -1; t < kDwUpTaps; ++t) {
        const float4 v = t < 0 ? bsum : acc[t < 0 ? 0 : t];
        __syncthreads();
        s_red[ps][cq][0] = v.x; s_red[ps][cq][1] = v.y; s_red[ps][cq][2] = v.z; s_red[ps][cq][3] = v.w;
        __syncthreads();
        if (ps == 0 && c4 < C4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float sum = s_red[0][cq][e] + s_red[1][cq][e] + s_red[2][cq][e] + s_red[3][cq][e];
                if (t < 0) { if (db) atomicAdd(db + c4 * 4 + e, sum); }
                else atomicAdd(dw + (long long)(c4 * 4 + e) * kDwUpTaps + t, sum);
            }
        }
    }
}

}  // namespace ssdk

static int mp_check(const char* fn, int batch, int h, int w, int channels, int pad_bottom, int pad_right) {
    SSDK_REQUIRE(batch > 0 && h > 0 && w > 0 && channels > 0 && channels % 4 == 0 && (pad_bottom == 0 || pad_bottom == 1) &&
                     (pad_right == 0 || pad_right == 1),
                 SSDK_E_INVALID, "%s: batch=%d H=%d W=%d C=%d (%% 4 == 0) pad_bottom=%d pad_right=%d (0 or 1)", fn, batch, h, w, channels,
                 pad_bottom, pad_right);
    SSDK_REQUIRE((h + pad_bottom) / 2 > 0 && (w + pad_right) / 2 > 0, SSDK_E_INVALID,
                 "%s: a %d x %d map padded by (%d, %d) has no 2 x 2 window (zero-sized pooled output; torch's max_pool2d refuses it too)", fn, h,
                 w, pad_bottom, pad_right);
    return SSDK_OK;
}

extern "C" int ssdk_maxpool2x2_fwd(const float* x, int batch, int h, int w, int channels, int pad_bottom, int pad_right, float* y, void* stream) {
    int rc = mp_check("ssdk_maxpool2x2_fwd", batch, h, w, channels, pad_bottom, pad_right);
    if (rc) return rc;
    SSDK_REQUIRE(x && y && (((uintptr_t)x | (uintptr_t)y) & 15) == 0, SSDK_E_INVALID, "ssdk_maxpool2x2_fwd: null or unaligned pointer");
    const int ho = (h + pad_bottom) / 2, wo = (w + pad_right) / 2;
    hipLaunchKernelGGL(ssdk::maxpool2x2_kernel, dim3(stream_blocks((long long)batch * ho * wo * (channels / 4), 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(x), batch, h, w, channels / 4, ho, wo, reinterpret_cast<float4*>(y));
    SSDK_CHECK_LAUNCH("maxpool2x2_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_maxpool2x2_bwd(const float* x, const float* dy, int batch, int h, int w, int channels, int pad_bottom, int pad_right, float* dx,
                                   void* stream) {
    int rc = mp_check("ssdk_maxpool2x2_bwd", batch, h, w, channels, pad_bottom, pad_right);
    if (rc) return rc;
    SSDK_REQUIRE(x && dy && dx && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0, SSDK_E_INVALID,
                 "ssdk_maxpool2x2_bwd: null or unaligned pointer");
    const int ho = (h + pad_bottom) / 2, wo = (w + pad_right) / 2;
    hipLaunchKernelGGL(ssdk::maxpool2x2_bwd_kernel, dim3(stream_blocks((long long)batch * ho * wo * (channels / 4), 256)), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(dy), batch, h, w, channels / 4, ho, wo,
                       reinterpret_cast<float4*>(dx));
    SSDK_CHECK_LAUNCH("maxpool2x2_bwd_kernel");
    return SSDK_OK;
}

static int cat_pieces(const char* fn, const float* const* pieces, const int* piece_channels, int n_pieces, long long rows, ssdk::CatPieces& ps) {
    SSDK_REQUIRE(pieces && piece_channels && n_pieces > 0 && n_pieces <= ssdk::kMaxPieces && rows > 0, SSDK_E_INVALID,
                 "%s: n_pieces=%d (1..%d) rows=%lld", fn, n_pieces, ssdk::kMaxPieces, rows);
    ps = ssdk::CatPieces{};
    ps.n = n_pieces;
    for (int k = 0; k < n_pieces; ++k) {
        SSDK_REQUIRE(piece_channels[k] > 0 && piece_channels[k] % 4 == 0, SSDK_E_INVALID, "%s: piece %d has %d channels (%% 4 == 0)", fn, k,
                     piece_channels[k]);
        SSDK_REQUIRE(pieces[k] && ((uintptr_t)pieces[k] & 15) == 0, SSDK_E_INVALID, "%s: piece %d is null or not 16-byte aligned", fn, k);
        ps.p[k] = (float4*)pieces[k];
        ps.c4[k] = piece_channels[k] / 4;
        ps.off4[k + 1] = ps.off4[k] + ps.c4[k];
    }
    return SSDK_OK;
}

extern "C" int ssdk_concat_channels_fwd(const float* const* pieces, const int* piece_channels, int n_pieces, long long rows, float* out, void* stream) {
    ssdk::CatPieces ps;
    int rc = cat_pieces("ssdk_concat_channels_fwd", pieces, piece_channels, n_pieces, rows, ps);
    if (rc) return rc;
    SSDK_REQUIRE(out && ((uintptr_t)out & 15) == 0, SSDK_E_INVALID, "ssdk_concat_channels_fwd: null or unaligned output");
    hipLaunchKernelGGL(ssdk::concat_kernel, dim3(stream_blocks(rows * ps.off4[n_pieces], 256)), dim3(256), 0, (hipStream_t)stream, ps, rows,
                       reinterpret_cast<float4*>(out));
    SSDK_CHECK_LAUNCH("concat_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_concat_channels_bwd(const float* dout, const int* piece_channels, int n_pieces, long long rows, float* const* dpieces,
                                        void* stream) {
    ssdk::CatPieces ds;
    int rc = cat_pieces("ssdk_concat_channels_bwd", (const float* const*)dpieces, piece_channels, n_pieces, rows, ds);
    if (rc) return rc;
    SSDK_REQUIRE(dout && ((uintptr_t)dout & 15) == 0, SSDK_E_INVALID, "ssdk_concat_channels_bwd: null or unaligned dout");
    hipLaunchKernelGGL(ssdk::split_kernel, dim3(stream_blocks(rows * ds.off4[n_pieces], 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(dout), rows, ds);
    SSDK_CHECK_LAUNCH("split_kernel");
    return SSDK_OK;
}

static int dwup_check(const char* fn, int batch, int hc, int wc, int hf, int wf, int channels) {
    SSDK_REQUIRE(batch > 0 && hc > 0 && wc > 0 && hf > 0 && wf > 0 && channels > 0 && channels % 4 == 0, SSDK_E_INVALID,
                 "%s: batch=%d coarse %d x %d fine %d x %d C=%d (%% 4 == 0)", fn, batch, hc, wc, hf, wf, channels);
    return SSDK_OK;
}

extern "C" int ssdk_depthwise_upsample_conv2d_fwd(const float* coarse, const float* w, const float* bias, int batch, int hc, int wc, int hf, int wf,
                                                  int channels, float* y, void* stream) {
    int rc = dwup_check("ssdk_depthwise_upsample_conv2d_fwd", batch, hc, wc, hf, wf, channels);
    if (rc) return rc;
    SSDK_REQUIRE(coarse && w && y && (((uintptr_t)coarse | (uintptr_t)y | (uintptr_t)bias) & 15) == 0, SSDK_E_INVALID,
                 "ssdk_depthwise_upsample_conv2d_fwd: null or unaligned pointer");
    hipLaunchKernelGGL(ssdk::dwup_fwd_kernel, dim3(stream_blocks((long long)batch * hf * wf * (channels / 4), 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(coarse), w, bias, batch, hc, wc, hf, wf, channels / 4, reinterpret_cast<float4*>(y));
    SSDK_CHECK_LAUNCH("dwup_fwd_kernel");
    return SSDK_OK;
}

extern "C" int ssdk_depthwise_upsample_conv2d_bwd(const float* coarse, const float* w, const float* dy, int batch, int hc, int wc, int hf, int wf,
                                                  int channels, float* dcoarse, float* dw, float* db, void* stream) {
    int rc = dwup_check("ssdk_depthwise_upsample_conv2d_bwd", batch, hc, wc, hf, wf, channels);
    if (rc) return rc;
    SSDK_REQUIRE(coarse && w && dy && (dcoarse || dw) && (((uintptr_t)coarse | (uintptr_t)dy | (uintptr_t)dcoarse) & 15) == 0, SSDK_E_INVALID,
                 "ssdk_depthwise_upsample_conv2d_bwd: null or unaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const int c4 = channels / 4;
    if (dcoarse) {
        hipLaunchKernelGGL(ssdk::dwup_dgrad_kernel, dim3(stream_blocks((long long)batch * hc * wc * c4, 256)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(dy), w, batch, hc, wc, hf, wf, c4, reinterpret_cast<float4*>(dcoarse));
        SSDK_CHECK_LAUNCH("dwup_dgrad_kernel");
    }
    if (dw) {
        hipLaunchKernelGGL(ssdk::zero_small_kernel, dim3(8), dim3(256), 0, s, dw, (long long)channels * ssdk::kDwUpTaps, db, db ? (long long)channels : 0LL);
        SSDK_CHECK_LAUNCH("zero_small_kernel");
        const long long M = (long long)batch * hf * wf;
        int chunks = (int)((M + 255) / 256);   // dw_wgrad_kernel's partials: >= 256 pixels per block, at most 512 per (channel, tap) ...
        if (chunks > 512) chunks = 512;
        if (ssdk::deterministic()) chunks = 1;  // ... and one in deterministic mode
        const int ppb = (int)((M + chunks - 1) / chunks);
        hipLaunchKernelGGL(ssdk::dwup_wgrad_kernel, dim3((unsigned)((c4 + 63) / 64), (unsigned)chunks), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(coarse), reinterpret_cast<const float4*>(dy), batch, hc, wc, hf, wf, c4, ppb, dw, db);
        SSDK_CHECK_LAUNCH("dwup_wgrad_kernel");
    }
    return SSDK_OK;
}
