// conv_plan.h -- which kernel instantiation a grouped GEMM launch of conv.hip runs, and how the launch is cut up: ONE pure function.
//
// Host only: no HIP header, compiles with plain g++ -std=c++17.  plan_launch() reads no environment, no global and no device; everything
// it depends on is in its arguments (the problems, the request, the knob values), so the library's entry points, the host-only query
// ssdk_debug_conv2d_plan and the tests all ask the same code.  conv.hip includes this file, builds requests, and launches from plans.
#pragma once

#include <stdint.h>

#include <algorithm>

namespace ssdk {

// ---- the knob table: every environment switch of conv.hip --------------------------------------------------------------------------------
// read: 'P' = once per process (at the first call that needs it; later changes of the environment are not seen), 'C' = on every call.
// The one getenv of conv.hip is conv_knob() there; the values the launch plan depends on travel in PlanKnobs (read_plan_knobs()).
enum ConvKnob {
    K_CONV_OLD_SPLIT, K_CONV_NO_SPLIT_UPTO, K_CONV_SPLIT_WIDE, K_CONV_STREAMK_GENERIC, K_CONV_STREAMK_BWD, K_CONV_NARROW_TO,
    K_SK_MINRANGE, K_CONV_NO_STREAMK, K_CONV_NO_HALF_TILE, K_CONV_NO_DMA, K_CONV_BK16, K_CONV_TN6, K_CONV_W8, K_CONV_NO_NARROW,
    K_CONV_NO_3STAGE, K_HEADS_NO_SPLITK, K_CONV_FORCE,
    K_ENABLE_FAULT_INJECTION, K_FAST_MIN_FLOPS, K_WGRAD_PER_PROBLEM, K_WGRAD_BUDGET, K_WGRAD_MIN_CHAIN, K_HEADS_T_DIV, K_HEADS_BWD_LEGACY,
    K_HEADS_BWD_MODE, K_ANCHOR_WGRAD_SLICES, K_PACK_SCAN, K_RG_PROBE, K_CONV_STRIDED_ORDERED,
    K_COUNT
};
struct ConvKnobInfo { const char* name; char read; const char* dflt; const char* meaning; };
constexpr ConvKnobInfo kConvKnobs[K_COUNT] = {
    {"SSDK_CONV_OLD_SPLIT", 'P', "unset", "set: the K-split rules before round 4's sweep (measurement knob)"},
    {"SSDK_CONV_NO_SPLIT_UPTO", 'P', "8", "K chains of at most this many slices are never split (atoi; measurement knob)"},
    {"SSDK_CONV_SPLIT_WIDE", 'P', "256", "row tiles x column tiles up to which 9..32 row tiles take the 32-column split rule (atoi)"},
    {"SSDK_CONV_STREAMK_GENERIC", 'P', "unset", "generic launches in stream-K form: unset = two rounds and more with a tail, 1 = all that qualify, 0 = none"},
    {"SSDK_CONV_STREAMK_BWD", 'P', "0", "non-zero: the mirrored-tap data gradient may take stream-K"},
    {"SSDK_CONV_NARROW_TO", 'P', "256", "workgroups up to which a small launch halves its column blocks (v > 0, else the default)"},
    {"SSDK_SK_MINRANGE", 'C', "24", "shortest stream-K range of a generic launch in units (v > 0, else 6 * kMaxTN)"},
    {"SSDK_CONV_NO_STREAMK", 'C', "unset", "set: no launch takes the stream-K form"},
    {"SSDK_CONV_NO_HALF_TILE", 'C', "unset", "set: a last column tile of <= 16 columns is computed as a whole 32-column tile"},
    {"SSDK_CONV_NO_DMA", 'C', "unset", "set: register-staged kernels instead of LDS-DMA (also: legacy heads backward, staged weight gradient)"},
    {"SSDK_CONV_BK16", 'C', "unset", "set: 16-float K slices for the plain forward launch (experiment)"},
    {"SSDK_CONV_TN6", 'C', "unset", "set: 192-column workgroups for the plain forward launch (experiment)"},
    {"SSDK_CONV_W8", 'C', "unset", "set: 8-wave / 256-pixel tiling for launches of >= 384 such workgroups (experiment)"},
    {"SSDK_CONV_NO_NARROW", 'C', "unset", "set: a launch smaller than the chip keeps its 128-column blocks"},
    {"SSDK_CONV_NO_3STAGE", 'C', "unset", "set: one-tile launches run the two-stage instantiation"},
    {"SSDK_HEADS_NO_SPLITK", 'C', "unset", "set: small heads launches never split K"},
    {"SSDK_CONV_FORCE", 'C', "unset", "\"<column blocks>,<K splits>\" for every problem of ssdk_conv2d_fwd (not in deterministic mode; tools/conv_decomp_sweep.py)"},
    {"SSDK_ENABLE_FAULT_INJECTION", 'C', "0", "non-zero: ssdk_debug_streamk_fault is honoured (tests only)"},
    {"SSDK_FAST_MIN_FLOPS", 'C', "1e9", "fast mode: launches below this many FLOPs stay fp32 (atof)"},
    {"SSDK_WGRAD_PER_PROBLEM", 'P', "unset", "set: grouped weight gradients are sized per problem, not launch-wide"},
    {"SSDK_WGRAD_BUDGET", 'P', "512", "workgroups of a launch-wide sized weight-gradient launch (v > 0, else the default)"},
    {"SSDK_WGRAD_MIN_CHAIN", 'P', "8", "shortest K chain of the same, in slices (v > 0, else the default)"},
    {"SSDK_HEADS_T_DIV", 'P', "4", "the anchor-row T buffer holds 1 / this of a level's anchors (d >= 1, else the default)"},
    {"SSDK_HEADS_BWD_LEGACY", 'C', "unset", "set: the legacy (atomic) heads backward instead of the ordered pipeline"},
    {"SSDK_HEADS_BWD_MODE", 'C', "unset", "force the form of the heads backward: 0 dense, 1 pixel rows (legacy only), 2 anchor rows (ordered only)"},
    {"SSDK_ANCHOR_WGRAD_SLICES", 'P', "64", "32-row slices per K split of the anchor-row weight gradient (v > 0, else the default)"},
    {"SSDK_PACK_SCAN", 'C', "unset", "set: the ordered heads backward always scans the packed rows"},
    {"SSDK_RG_PROBE", 'C', "0", "measurement probe of the anchor row GEMM (atoi; 1: T stores dropped)"},
    {"SSDK_CONV_STRIDED_ORDERED", 'P', "unset", "set: strided data gradients take the ordered (rows + sum) form everywhere"},
};

// ---- tile constants and the kernels' argument structs (kernel ABI: fields are never reordered, added or dropped) ----------------------------
constexpr int kBM = 128;        // output pixels per workgroup
constexpr int kBK = 32;         // K slice
constexpr int kMaxTN = 4;       // 32-wide column tiles per workgroup
constexpr int kConvThreads = 256;
constexpr int kMaxProblems = 8;

struct ConvProblem {
    // A operand rows [pixel][channel], one segment
    const float* a;
    long long a_bstride;  // per-image stride (floats)
    int a_pstride;        // per-pixel stride (floats)
    int Cc;               // channels (K per tap)
    int B, Hout, Wout, Hin, Win, ksize, stride, pad;
    // W rows: n < n0 -> w0[n][taps*Cc], else w1[n-n0][taps*Cc]
    const float* w0;
    const float* w1;
    const float* bias0;
    const float* bias1;
    int n0, n1;
    // output: element (image b, pixel p, channel n) at o0 + b*ob0 + p*os0 + n (n < n0) / o1 + b*ob1 + p*os1 + (n-n0)
    float* o0;
    float* o1;
    long long ob0, ob1;
    int os0, os1;
    int tiles_n, n_blocks, m_tiles;
    int m_tiles256;   // M tiles of the 8-wave (256-pixel) tiling
    int k_splits;     // > 1: the K slices are divided over k_splits workgroups that atomically add into a zeroed output
    int block_begin;  // first workgroup of this problem in the grouped grid
    int relu;
    // device-side mode switch (sparse backward): the launch is a no-op for this problem unless *mode == want_mode
    const int* mode;
    int want_mode;
    // SCATTER instantiation: rows are the entries of row_list (pixel ids with a non-zero gradient row), *row_count of them
    const int* row_list;
    const int* row_count;
    int sc_cin;  // scatter: output channels per tap (n = tap * sc_cin + c)
    // column index space: [0, n0) = rows of w0, [n0, n0_pad) unused, [n0_pad, n0_pad + n1) = rows of w1.  n0_pad = n0 except for
    // the LDS-DMA kernel, which rounds it up to 8 so that every 8-row DMA piece reads ONE weight tensor (one descriptor)
    int n0_pad;
    unsigned w0_bytes, w1_bytes;   // LDS-DMA kernel: sizes of the two weight tensors (buffer descriptors)
    int forced;   // n_blocks / k_splits were set by a split rule or SSDK_CONV_FORCE: the narrowing steps of plan_launch keep them
    // The last 32-column tile holds at most 16 columns (N = 104 of the 21-class heads: 3 tiles + 8 columns): it is computed as a 16-column
    // tile by v_mfma_f32_16x16x1_4b_f32 at half the cycles of a 32 x 32 x 2 (dma_tile, forward LDS-DMA form only; set by plan_launch)
    int half_last;
    // BatchNorm statistics of the output, fused into the epilogue (forward, one output, not split over K): per-column sums of the
    // stored values and of their squares are ADDED into stats[0 .. n0) / stats[n0 .. 2 n0) (fp64), stats[2 n0] = rows.  NULL: none.
    double* stats;
};

// ---- request and plan ------------------------------------------------------------------------------------------------------------------
enum ConvForm { kFormPlain, kFormGeneric, kFormMirror, kFormScatter };   // plain = the heads' forward launch
// Who may split K: nobody (whole K chains: the heads' backward launches, the scatter and row GEMMs), the heads' forward rule (only
// while the launch has at most kStreamKWgs 128-column workgroups), or the convolutions' rule (every problem is asked).
enum ConvSplit { kSplitNone, kSplitHeads, kSplitConv };

struct PlanKnobs {   // the values plan_launch depends on (conv.hip: read_plan_knobs)
    bool old_split; int no_split_upto; int split_wide; int streamk_generic; bool streamk_bwd; long long narrow_to;   // once per process
    long long sk_minrange;                                                                                          // per call, below too
    bool no_streamk, no_half_tile, no_dma, bk16, tn6, w8, no_narrow, no_3stage, heads_no_splitk;
};
struct PlanRequest {
    ConvForm form;
    bool vtab;            // scatter over a device-built tile list (sparse heads backward)
    bool ws;              // a stream-K workspace is available
    int ws_wgs;           // ... laid out for / capped at this many workgroups
    ConvSplit split;
    int force_nb, force_ks;   // SSDK_CONV_FORCE for every problem, 0 = none
    bool det;             // deterministic mode: no K split (its sums are fp32 atomics in hardware order)
    PlanKnobs knobs;
};

// one value per instantiation that is launched
enum ConvKernel {
    kDmaW8Mirror, kDmaW8Generic, kDmaW8Plain, kDmaScatterVtab, kStreamKMirror, kStreamK,
    kDmaScatterOne, kDmaMirrorOne, kDmaGenericOne, kDmaScatter, kDmaMirror, kDmaGeneric, kDmaBk16, kDmaTn6, kDmaPlain,
    kStagedScatter4, kStagedMirrorStrided4, kStagedMirrorStrided1, kStagedMirror4, kStagedMirror1, kStagedGeneric4, kStagedGeneric1,
    kStagedPlain4, kStagedPlain1
};
static inline const char* conv_kernel_name(ConvKernel k) {
    static const char* const names[] = {
        "dma w8 mirror", "dma w8 generic", "dma w8 plain", "dma scatter vtab", "streamk mirror", "streamk",
        "dma scatter one-tile", "dma mirror one-tile", "dma generic one-tile", "dma scatter", "dma mirror", "dma generic", "dma plain bk16",
        "dma plain tn6", "dma plain",
        "staged<4> scatter", "staged<4> mirror strided", "staged<1> mirror strided", "staged<4> mirror", "staged<1> mirror", "staged<4> generic",
        "staged<1> generic", "staged<4> plain", "staged<1> plain"};
    return names[k];
}
enum ConvPlanError { kPlanOk, kPlanVtabNeedsCounts, kPlanScatterUnaligned };

struct ConvPlan {
    ConvKernel kernel;
    int grid, threads;                // of the launch
    int total_blocks;                 // workgroups of the whole-tile partition (= grid except for a tile-list or a stream-K launch)
    int streamk_wgs;                  // > 0: the stream-K form with this many persistent workgroups; 0: whole tiles
    long long unit_begin[kMaxProblems + 1];   // stream-K: prefix of the half-tile units over the problems in launch order
    int count;
    int order[kMaxProblems];          // launch order: the i-th problem of the launch is p[order[i]]
    ConvProblem p[kMaxProblems];      // the caller's problems in the caller's order, finished: n0_pad, tiles_n, n_blocks, k_splits, half_last,
                                      // block_begin, w0_bytes, w1_bytes; stats dropped where the epilogue cannot keep them
    bool zero_first[kMaxProblems];    // the output is added to with atomics (split K): the caller zeroes it before the launch
    ConvPlanError error;
    bool stats_in_epilogue(int i) const { return p[i].stats != nullptr; }
    int blocks_of(int i) const { return (threads == 512 ? (p[i].m_tiles256 + 7) / 8 : (p[i].m_tiles + 7) / 8) * 8 * p[i].n_blocks * p[i].k_splits; }
};

static inline int plan_cdiv(int a, int b) { return (a + b - 1) / b; }

// 16-byte rows and operands everywhere (the float4 kernels; the LDS-DMA kernel asks more, see plan_launch); any strided problem
struct RowForm { bool vec4, strided; };
static inline RowForm row_form(const ConvProblem* probs, int count) {
    RowForm rf = {true, false};
    for (int i = 0; i < count; ++i) {
        const ConvProblem& g = probs[i];
        if (g.Cc % 4 || g.a_pstride % 4 || g.a_bstride % 4 || ((uintptr_t)g.a & 15) || ((uintptr_t)g.w0 & 15) || (g.w1 && ((uintptr_t)g.w1 & 15))) rf.vec4 = false;
        rf.strided = rf.strided || g.stride != 1;
    }
    return rf;
}
static inline void finish_problem(ConvProblem& g) {
    g.n0_pad = g.n0;
    const int N = g.n0 + g.n1;
    g.tiles_n = plan_cdiv(N, 32);
    g.n_blocks = plan_cdiv(g.tiles_n, kMaxTN);
    g.m_tiles = plan_cdiv(g.B * g.Hout * g.Wout, kBM);
    g.m_tiles256 = plan_cdiv(g.B * g.Hout * g.Wout, 256);
    g.k_splits = 1;
}
static inline long long problem_block_work(const ConvProblem& g) {
    const int chunks = plan_cdiv(g.Cc, kBK);
    return (long long)g.ksize * g.ksize * chunks * plan_cdiv(g.tiles_n, g.n_blocks) / g.k_splits;
}
// small GEMMs (pyramid tail): too few output tiles to fill 256 CUs -> split K, add partial tiles atomically (the
// caller zeroes the output first).  Not with a fused ReLU (needs the complete sum).
static inline void split_k_any(ConvProblem& g, const PlanKnobs& kn) {
    const int blocks = plan_cdiv(g.m_tiles, 8) * 8 * g.n_blocks;
    const int slices = g.ksize * g.ksize * plan_cdiv(g.Cc, kBK);
    // A K chain of eight slices is not worth cutting: a split saves at most ~3 us of it and costs a zero-fill launch, an atomic epilogue
    // and -- for a convolution in front of a BatchNorm -- the statistics pass that a complete tile does in its epilogue
    // (tools/conv_decomp_sweep.py m2det: 1 x 1 256 -> 256 at 16 x 16, batch 16: 19.4 -> 13.6 us with 32-column workgroups and no split)
    // (SSDK_CONV_NO_SPLIT_UPTO: 16 and 24 measured within noise of 8 on SSD-300 / SSD-512 / M2Det)
    if (g.relu || blocks >= 256 || slices < (kn.old_split ? 8 : kn.no_split_upto + 1)) return;
    // Many row tiles, few column blocks (the SSD-300 tail's 1 x 1 512 -> 256 at 18 x 18, batch 32: 81 x 2 tiles of 128 x 128): 64-column
    // workgroups fill the chip WITHOUT splitting K -- no atomic epilogue (3 x the output through 1.3 TB/s of atomics), no zero-fill
    // launch: 57 -> 44 us (tools/conv_decomp_sweep.py; the other tail layers stay within 15 % of their best split)
    if (g.tiles_n >= 4 && g.tiles_n % 2 == 0 && (long long)g.m_tiles * (g.tiles_n / 2) >= 256 && slices <= 32) {
        g.n_blocks = g.tiles_n / 2;
        g.forced = 1;
        return;
    }
    // Few row tiles and a deep K (the 3 x 3 / 2 layers on 16 x 16 .. 4 x 4 maps: M <= 1 024 rows, 36 .. 72 slices): 32-column workgroups
    // first, then only as many K splits as bring the launch to ~256 workgroups with at least 8 slices each -- the rule below split the
    // M2Det TUM's 256 -> 256 layer at 16 x 16 eighteen ways (49 us; 26 us with 8 column blocks x 4 splits), tools/conv_decomp_sweep.py
    // (round 4: up to 32 row tiles when tiles x column tiles still fit one per CU -- the M2Det TUM's 256 -> 256 layer at 32 x 32 -> 16 x 16,
    // batch 16, took the rule below: 2 column blocks x 8 splits, 73.5 us; 8 column blocks x 2 splits: 52.6)
    if (g.m_tiles >= 3 && (g.m_tiles <= 8 || (!kn.old_split && g.m_tiles <= 32 && g.m_tiles * g.tiles_n <= kn.split_wide)) && slices >= 32) {   // (one or two row tiles: the rule below measured as good or better)
        g.n_blocks = g.tiles_n;
        int ks = std::max(2, 256 / std::max(1, g.m_tiles * g.n_blocks));
        ks = std::min(ks, slices / 8);
        if (!kn.old_split && g.m_tiles > 8 && g.m_tiles * g.n_blocks * ks > 512) ks = 512 / (g.m_tiles * g.n_blocks);   // (never more than two workgroups per CU)
        if (!kn.old_split && g.m_tiles > 8 && ks < 2) { g.forced = 1; return; }   // one 32-column workgroup per tile, whole K: no atomics, statistics in the epilogue
        if (ks >= 2) {
            g.k_splits = ks;
            g.forced = 1;
            return;
        }
        g.n_blocks = plan_cdiv(g.tiles_n, kMaxTN);
    }
    int ks = plan_cdiv(512, blocks);
    if (ks > slices / 4) ks = slices / 4;
    if (ks < 2) return;
    g.k_splits = ks;
}
static inline void split_k(ConvProblem& g, bool det, const PlanKnobs& kn) {
    if (!det) { split_k_any(g, kn); return; }
    // deterministic mode: a K split adds its partial tiles with fp32 atomics in hardware order -- never taken (the column-block choices
    // that come without a split are kept)
    ConvProblem t = g;
    split_k_any(t, kn);
    if (t.k_splits == 1) g = t;
}
// Atomic epilogues (split K, scatter) leave a CU at about one 256-byte wave instruction per 50 ns (MI355X_MICROARCH.md, Global
// float atomics): the 256 of a 128-column tile take 13 us -- phase stamps of the pyramid tail's convolutions showed 3 us of
// prologue, 8 us of K loop and 13 us of epilogue.  While the launch is smaller than the chip, halve the columns per workgroup
// instead: twice the workgroups, each with half the atomics, on CUs that were idle.
static inline void narrow_for_atomics(ConvProblem& g) {
    while (g.n_blocks < g.tiles_n && (long long)g.m_tiles * g.n_blocks * g.k_splits <= 256) g.n_blocks = std::min(g.tiles_n, g.n_blocks * 2);
}

constexpr int kStreamKWgs = 512;   // two 64 KB-LDS workgroups per CU x 256 CUs: the most a stream-K launch uses, and the size its workspace is laid out for
// does a column space of N end in a tile of at most 16 columns?
static inline bool half_tile_of(int N) { return N % 32 != 0 && N % 32 <= 16; }
constexpr long long kStreamKMinRange = 24 * kMaxTN;
constexpr int kStreamKMinWgs = 256;
// generic convolutions (pyramid tail, tower, necks): the launches stream-K helps are ONE to two rounds of tiles on 256 CUs (the SSD-300
// tail's 1 x 1 512 -> 256 at 18 x 18: 162 tiles of 128 x 128, split over K three ways with an atomic epilogue before), so their ranges are
// shorter than the heads': 6 K slices of a 128-column block (PlanKnobs::sk_minrange, SSDK_SK_MINRANGE: measurement knob)

// Decides the K splits, the kernel (LDS-DMA or register staged; 128- or 256-pixel tiles; whole tiles or stream-K), narrows the column
// blocks, orders the problems by decreasing work per workgroup (longest first) and assigns their block ranges.
static inline ConvPlan plan_launch(const ConvProblem* problems, int count, const PlanRequest& rq) {
    ConvPlan pl;
    const PlanKnobs& kn = rq.knobs;
    const bool mirror = rq.form == kFormMirror, scatter = rq.form == kFormScatter;
    // (the data gradient asks for stream-K with the generic convolutions' rules: it is the same layers' launch)
    const bool generic = rq.form == kFormGeneric || (mirror && rq.ws);
    ConvProblem* const probs = pl.p;
    pl.count = count;
    pl.error = kPlanOk;
    pl.streamk_wgs = 0;
    for (int i = 0; i < count; ++i) {
        probs[i] = problems[i];
        finish_problem(probs[i]);
    }
    // One or two rounds of whole tiles on 256 CUs (the big layers of a pyramid tail, the heads): stream-K over all the launch's K slices
    // instead of splitting K with an atomic epilogue into a zeroed output -- no zero-fill launch, no atomics, BatchNorm statistics still in
    // the epilogue.
    // Step 1 of the stream-K decision: would the launch run these problems in stream-K form?  Asked BEFORE K is split (a split launch never
    // does), of the problems as finish_problem left them and as the LDS-DMA kernel will lay their columns out.  Step 2, below, decides from
    // the launch as it then is; the two agree wherever step 1 says yes except under SSDK_CONV_W8 (no half tile there) and under a workgroup
    // cap below kStreamKWgs (ssdk_heads_fwd_ex: step 2 compares the grid with the CAPPED count), so both are kept, in this order.
    // Only a caller that may split K asks: the others never hand a workspace on.
    const bool takes = rq.ws && rq.split != kSplitNone && [&]() {
        // generic convolutions: OFF unless asked for (SSDK_CONV_STREAMK_GENERIC=1).  Measured on the SSD-300 tail at batch 32
        // (tools/r03_sk_sweep.sh): the 1 x 1 512 -> 256 layer 56 -> 92-115 us and the 3 x 3 / 2 256 -> 512 layer 85 -> 140 us with ranges of
        // 8 .. 32 units -- a launch of ONE round has no tail to even out, and every workgroup then parks and fixes up a 64 KB partial tile
        // Round 4: launches of TWO rounds of tiles and more do take it (the RetinaNet tower's grouped launches: 2 664 tiles of 128 x 128 on 512
        // slots -- the last, partly filled round is what stream-K evens out: 46.40 -> 45.94 ms per step); SSDK_CONV_STREAMK_GENERIC=1: every
        // generic launch that qualifies like a heads launch, =0: none
        // Round 5: the mirrored-tap data gradient can take it too (igemm_streamk_kernel<true>), but does not by default: on the RetinaNet towers'
        // grouped launch (2 688 tiles on 512 slots, 8 launches per step) it measured 1 475 us per launch against 1 478 us for the whole-tile
        // launch and 46.13 / 46.11 against 46.12 / 46.22 ms per step -- nothing to show for the spin-waits.  SSDK_CONV_STREAMK_BWD=1 turns it on.
        if (kn.no_streamk || (generic && kn.streamk_generic == 0) || (mirror && !kn.streamk_bwd)) return false;
        long long units = 0, blocks = 0;
        for (int i = 0; i < count; ++i) {
            const ConvProblem& g = probs[i];
            if (g.Cc % kBK || g.mode) return false;
            const int N = (g.n1 > 0 ? plan_cdiv(g.n0, 8) * 8 : g.n0) + g.n1, tiles_n = plan_cdiv(N, 32);
            const int half = (!mirror && !g.stats && half_tile_of(N) && !kn.no_half_tile) ? 1 : 0;   // (as half_last will be set below)
            units += (long long)g.m_tiles * g.ksize * g.ksize * (g.Cc / kBK) * (2 * tiles_n - half);           // half-tile units, as StreamK counts
            blocks += (long long)plan_cdiv(g.m_tiles, 8) * 8 * plan_cdiv(tiles_n, kMaxTN);
        }
        const long long min_range = generic ? kn.sk_minrange : kStreamKMinRange;
        const long long nwg = std::min<long long>(512, units / (2 * min_range) / 8 * 8);
        // (two rounds and more, the last one at most three quarters full: a launch of whole rounds -- the M2Det neck's 2 048- and 3 584-tile
        // layers -- has no tail to even out and measured 0.1 ms slower per step with the fix-up traffic)
        if (generic && kn.streamk_generic < 0 && (blocks < 2 * kStreamKWgs || blocks % kStreamKWgs == 0 || blocks % kStreamKWgs > 3 * kStreamKWgs / 4)) return false;
        return nwg >= kStreamKMinWgs && blocks <= 16 * nwg;
    }();
    if (rq.split == kSplitConv && !takes) {
        for (int i = 0; i < count; ++i) split_k(probs[i], rq.det, kn);
    } else if (rq.split == kSplitHeads) {
        // Small batches: a level has a handful of row tiles, each with a K chain of 9 * Cin / 32 slices (1.5 us apiece) -- ssd_mb2_voc at batch
        // 2 spent 534 us in 24 workgroups.  While the launch is too small for stream-K (at most one workgroup per slot), the K slices of such
        // a level are divided over several workgroups that add into the zeroed outputs, like the pyramid tail's convolutions.
        long long blocks = 0;
        for (int i = 0; i < count; ++i) blocks += (long long)plan_cdiv(probs[i].m_tiles, 8) * 8 * probs[i].n_blocks;
        if (blocks <= kStreamKWgs && !takes && !kn.heads_no_splitk)
            for (int i = 0; i < count; ++i) split_k(probs[i], rq.det, kn);
    }
    if (rq.force_nb > 0 && rq.force_ks > 0 && !takes) {   // measurement knob (tools/conv_decomp_sweep.py): "<column blocks>,<K splits>"
        for (int i = 0; i < count; ++i) {
            ConvProblem& g = probs[i];
            g.n_blocks = std::min(rq.force_nb, g.tiles_n);
            g.k_splits = (g.relu || rq.force_ks < 2) ? 1 : rq.force_ks;
            g.forced = 1;
        }
    }
    for (int i = 0; i < count; ++i) {
        pl.zero_first[i] = probs[i].k_splits > 1;
        if (pl.zero_first[i]) probs[i].stats = nullptr;   // (in the epilogue otherwise; a split-K output is only complete after the launch: a pass of its own)
    }
    // the heads' forward launch hands its workspace on whatever step 1 said (step 2 decides alone); the convolutions only after a yes
    const bool skws = rq.split == kSplitHeads ? rq.ws : takes;
    const bool vtab = rq.vtab;

    const RowForm rf = row_form(probs, count);
    const bool vec4 = rf.vec4, strided = rf.strided;
    // LDS-DMA kernel: 16-byte rows, whole 32-channel chunks, stride-1 taps when mirrored, all byte offsets below 2^31
    bool dma = vec4 && !(mirror && strided) && !kn.no_dma;
    for (int i = 0; i < count && dma; ++i) {
        ConvProblem& g = probs[i];
        const long long span_a = ((long long)g.B * g.a_bstride + (long long)(g.ksize + g.pad) * ((long long)g.Win + 1) * g.a_pstride) * 4;
        const long long w0_bytes = (long long)g.n0 * (scatter ? 1 : g.ksize * g.ksize) * g.Cc * 4, w1_bytes = (long long)g.n1 * g.ksize * g.ksize * g.Cc * 4;
        if (g.Cc % kBK || span_a >= (1LL << 31) - 4096 || w0_bytes >= (1LL << 31) - 4096 || w1_bytes >= (1LL << 31) - 4096) { dma = false; break; }
        g.w0_bytes = (unsigned)w0_bytes;
        g.w1_bytes = (unsigned)w1_bytes;
    }
    const bool plain = rq.form == kFormPlain;
    // 16-float K slices (3 workgroups per CU): opt-in experiment for the plain forward launch
    const bool bk16 = dma && plain && kn.bk16;
    // 192-column workgroups (6 column tiles) for the plain forward launch: opt-in experiment
    const bool tn6 = dma && plain && !bk16 && kn.tn6;
    for (int i = 0; i < count; ++i) {   // column space of the chosen kernel (see ConvProblem::n0_pad)
        ConvProblem& g = probs[i];
        g.n0_pad = (dma && g.n1 > 0) ? plan_cdiv(g.n0, bk16 ? 16 : 8) * (bk16 ? 16 : 8) : g.n0;
        g.tiles_n = plan_cdiv(g.n0_pad + g.n1, 32);
        g.half_last = (dma && !mirror && !scatter && !bk16 && !tn6 && !g.stats && half_tile_of(g.n0_pad + g.n1) && !kn.w8 && !kn.no_half_tile) ? 1 : 0;
        if (!g.forced) {
            g.n_blocks = plan_cdiv(g.tiles_n, tn6 ? 6 : kMaxTN);
            if (!vtab && (scatter || g.k_splits > 1)) narrow_for_atomics(g);
        }
    }
    // A launch smaller than the chip, whatever its epilogue: halve the columns per workgroup while the workgroups still fit one per CU.
    // A 128 x 128 x 32 slice is 1.7 us of MFMA on one CU, so the 1 x 1 data gradients of the pyramid tail (K = 128: 4 slices, 6 .. 100
    // workgroups of 128 columns) spent 9 us in the K loop and 6.6 us storing four column tiles on a chip that was 60-98 % idle
    // (tools/phase_conv.py bwd); at 32 columns a slice costs its DMA latency (~0.85 us) instead.  The column partition does not change
    // any sum's order: same bits.
    // (not for the heads' forward launch: its stream-K partition is sized from the 128-column blocks)
    if (!vtab && !skws && !kn.no_narrow) {
        const long long fill = kn.narrow_to;
        long long total = 0;
        for (int i = 0; i < count; ++i) total += (long long)probs[i].m_tiles * probs[i].n_blocks * probs[i].k_splits;
        for (bool again = true; again && total < fill;) {
            again = false;
            for (int i = 0; i < count; ++i) {
                ConvProblem& g = probs[i];
                if (g.forced || g.n_blocks >= g.tiles_n) continue;
                const int nb = std::min(g.tiles_n, g.n_blocks * 2);
                const long long grown = total + (long long)g.m_tiles * (nb - g.n_blocks) * g.k_splits;
                if (grown > fill) continue;
                g.n_blocks = nb;
                total = grown;
                again = true;
            }
        }
    }
    // 8-wave / 256-pixel tiling: measured 3 % (B=128) to 14 % (B=32) MORE cycles than two 4-wave workgroups per CU on the
    // SSD-300 heads (one barrier stalls all eight waves of the CU at once) -- kept as an opt-in experiment only
    bool w8 = false;
    if (dma && !scatter && kn.w8) {
        long long blocks256 = 0;
        for (int i = 0; i < count; ++i) blocks256 += (long long)probs[i].m_tiles256 * probs[i].n_blocks * probs[i].k_splits;
        w8 = blocks256 >= 384;
    }
    int* const order = pl.order;
    for (int i = 0; i < count; ++i) order[i] = i;
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j)
            if (problem_block_work(probs[order[j]]) > problem_block_work(probs[order[i]])) { int t = order[i]; order[i] = order[j]; order[j] = t; }
    int begin = 0;
    for (int i = 0; i < count; ++i) {
        ConvProblem& g = probs[order[i]];
        g.block_begin = begin;
        begin += plan_cdiv(w8 ? g.m_tiles256 : g.m_tiles, 8) * 8 * g.n_blocks * g.k_splits;
    }
    pl.grid = pl.total_blocks = begin;
    pl.threads = kConvThreads;
    const int v = vec4 ? 0 : 1;   // (the scalar instantiation follows the float4 one in ConvKernel)
    if (dma && w8) {
        pl.threads = 512;
        pl.kernel = mirror ? kDmaW8Mirror : rq.form == kFormGeneric ? kDmaW8Generic : kDmaW8Plain;
    } else if (dma && scatter && vtab) {
        // sparse backward: only the row tiles that exist (listed on the device), walked by a fixed grid of 8 workgroups per CU
        for (int i = 0; i < count; ++i)
            if (!probs[i].row_count || probs[i].k_splits != 1) pl.error = kPlanVtabNeedsCounts;
        pl.kernel = kDmaScatterVtab;
        pl.grid = 2048;
    } else if (dma && skws && !scatter && !bk16 && !tn6 && !kn.no_streamk) {
        // Step 2 of the stream-K decision.  Stream-K only where it pays: a launch of a few rounds of whole tiles (its last round is then a
        // large share of the time), and every range at least as long as the longest tile (a tile is cut at most once)
        int nwg = rq.ws_wgs;
        long long total_units = 0;
        for (int i = 0; i < count; ++i) {
            const ConvProblem& g = probs[order[i]];
            const long long slices = (long long)g.ksize * g.ksize * (g.Cc / kBK);
            pl.unit_begin[i] = total_units;
            total_units += (long long)g.m_tiles * slices * (2 * g.tiles_n - g.half_last);
            if (g.k_splits != 1 || g.mode) nwg = 0;
        }
        pl.unit_begin[count] = total_units;
        // Not for launches of many rounds (the tail is then a small share and whole tiles need no fix-up).  Otherwise as many workgroups as
        // leave each a range of at least kStreamKMinRange units (24 K slices of a 128-column block): a tile longer than a range is cut
        // several times and its owner adds all the parked parts.  Below 256 workgroups the split-K path of the caller does as well (measured on ssd_mb2_voc).
        if (nwg > 0 && begin > 16 * nwg) nwg = 0;
        const long long min_range = generic ? kn.sk_minrange : kStreamKMinRange;
        if (nwg > 0) nwg = (int)std::min<long long>(nwg, total_units / (2 * min_range) / 8 * 8);   // (min_range counts whole tiles)
        if (nwg >= kStreamKMinWgs) {
            pl.streamk_wgs = nwg;
            pl.grid = nwg;
            pl.kernel = mirror ? kStreamKMirror : kStreamK;
        } else {
            pl.kernel = mirror ? kDmaMirror : rq.form == kFormGeneric ? kDmaGeneric : kDmaPlain;
        }
    } else if (dma) {
        // every workgroup of the launch owns ONE 32-column tile (the launches narrowed above, the atomic-epilogue launches of the small
        // maps): the three-stage instantiation -- its K loop does not wait for a DMA issued one slice earlier but two
        bool one_tile = !bk16 && !tn6 && !kn.no_3stage;
        for (int i = 0; i < count && one_tile; ++i) one_tile = probs[i].n_blocks == probs[i].tiles_n && !probs[i].half_last;
        if (one_tile && scatter) pl.kernel = kDmaScatterOne;
        else if (one_tile && mirror) pl.kernel = kDmaMirrorOne;
        else if (one_tile && rq.form == kFormGeneric) pl.kernel = kDmaGenericOne;
        else if (scatter) pl.kernel = kDmaScatter;
        else if (mirror) pl.kernel = kDmaMirror;
        else if (rq.form == kFormGeneric) pl.kernel = kDmaGeneric;
        else if (bk16) pl.kernel = kDmaBk16;
        else if (tn6) pl.kernel = kDmaTn6;
        else pl.kernel = kDmaPlain;
    } else if (scatter) {
        if (!vec4) pl.error = kPlanScatterUnaligned;
        pl.kernel = kStagedScatter4;
    } else if (mirror && strided) {
        pl.kernel = (ConvKernel)(kStagedMirrorStrided4 + v);
    } else if (mirror) {
        pl.kernel = (ConvKernel)(kStagedMirror4 + v);
    } else if (rq.form == kFormGeneric) {  // same code, separate instantiation: profiles list the extras/tower convs apart from the heads
        pl.kernel = (ConvKernel)(kStagedGeneric4 + v);
    } else {
        pl.kernel = (ConvKernel)(kStagedPlain4 + v);
    }
    return pl;
}

}  // namespace ssdk
